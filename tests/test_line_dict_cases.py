"""The benchmark cases really have the structure the tables of distinct lines rely on: on a uniform mesh with Dirichlet
sides, lines with equal material sequences have bit-equal factors, and the cores the project measures are built from a few assembly
types and axial zones, so only a handful of the lines of a direction differ.  Counted here with numpy on the cross-sections; this
guards the gain against a change of the case generators and tests no kernel.

Bar: at most 1/8 of the lines of a direction and group are distinct.  At 256^3 the IAEA-3D resampling has 12 / 12 / 3 distinct D
sequences of 65 536 lines (x / y / z); a coarser resampling of the same 19^3 assemblies can only merge sequences, never split them."""
import numpy as np
import pytest

from neutfem_amd import cases


def _distinct(a, axis):
    """distinct sequences along `axis` of a (nz, ny, nx) array, compared by bit pattern"""
    lines = np.moveaxis(a, axis, -1).reshape(-1, a.shape[axis])
    return len(np.unique(np.ascontiguousarray(lines).view(np.uint64), axis=0)), lines.shape[0]


def _counts(case):
    out = {}
    for g in range(int(case["ng"])):
        for name, axis in (("x", 2), ("y", 1), ("z", 0)):
            out[(g, name)] = _distinct(case["D"][g], axis)
        # the x table also carries the C diagonal: removal cross-section next to D
        both = np.stack([case["D"][g], case["SigR"][g]], axis=-1).reshape(case["D"][g].shape[:2] + (-1,))
        out[(g, "x+SigR")] = _distinct(both, 2)
    return out


@pytest.mark.parametrize("name", ["iaea3d_64", "checkerboard_48"])
def test_few_distinct_lines(name):
    case = cases.iaea3d_resampled(64) if name == "iaea3d_64" else cases.synthetic_checkerboard(48, ng=2)
    for axis in ("x_breaks", "y_breaks", "z_breaks"):
        h = np.diff(case[axis])
        assert np.all(h == h[0]), (axis, "uniform widths: equal material sequences give bit-equal factors")
    assert sorted(a for a, t in case["bc"] if t == 0) == [1, 2, 3, 4, 5, 6]
    for (g, d), (n, of) in _counts(case).items():
        print(f"{name} group {g} {d}: {n} distinct of {of} lines")
        assert n * 8 <= of, (name, g, d, n, of)


def test_iaea3d_64_is_no_richer_than_the_benchmark_size():
    """the figures of the 256^3 benchmark mesh bound every coarser resampling"""
    c = _counts(cases.iaea3d_resampled(64))
    for g in range(2):
        assert c[(g, "x")][0] <= 12 and c[(g, "y")][0] <= 12 and c[(g, "z")][0] <= 3
    assert c[(0, "x+SigR")][0] <= 12 and c[(1, "x+SigR")][0] <= 18
