"""Whole-tile form of the two benchmark passes (FULL = 1 of the staged k_schur_s and of the table-backed early-load k_schur_c in
neutfem_amd/csrc/nf_kernels.h, option "tile_full").

Where the tile grid of a pass has no partial tile -- the tile width divides nx, a line is a whole number of segments (of chunks), the block
has one thread per (column, segment) -- the host takes an instantiation whose per-access predicates are true at compile time: loads and
stores are straight-line and addressed by 32-bit byte offsets.  Values and arithmetic are those of the predicated body, so the bar between
the two is np.array_equal.  Every case first asserts through the launch-plan report (HipSolver.apply_plan: "full", "family", "TX", "NSEG",
"stage" per pass), outside and inside CG, that the form under test engages -- or is refused, where the case says so -- and only then checks
numbers on the same inputs:

  apply        max |y - y_oracle| <= 1e-12 max |y_oracle| on every group (the bar of tests/test_gpu_line_dict.py), bit-equal to a handle
               with tile_full = 0
  solve_group  tolerance 1e-30 (out of CG's reach), 12 iterations: solution, iteration count and final residual bit-equal to tile_full = 0
  fixed work   solve_keff with FIXED: k-history, CG counts and flux bit-equal to tile_full = 0; k-history 1e-9 and flux 1e-8 against the oracle
  rho          one shape on the filler-contrast inputs of tests/apply_exact.py: per-component error against the extended-precision
               apply, bar K_APPLY x 2^-53 (that file's)

Shapes (k_schur_s staged with s_stage = 1, s_long = 0; k_schur_c with s_long = 1):
  s3      (64, 8, 24), 3 blocks    8 z tiles as 3 / 3 / 2 per block: what is formed once per thread must hold from tile to tile; the y pass
                                   (one segment per line, 24 tiles) takes the form too
  s64     (64, 8, 24), 64 blocks   more blocks than tiles: a block without a second tile
  sxcd    (128, 8, 16), 5 blocks   16 z tiles in the XCD-contiguous order: the tile origin changes inside the loop
  s256z   (32, 2, 256), 1 block    32 segments on 32 columns, 1024 threads: the benchmark's z tile
  s256y   (32, 256, 2), 2 blocks   the same in the y direction
  sodd    (130, 8, 16)             nx is no multiple of the tile width: not staged, "full" reads 0
  s21     (64, 9, 21), 2 blocks    lines off the segment grid (9 and 21 cells): staged, "full" reads 0, the predicated body runs
  c32     (32, 32, 32)             k_schur_c on y and z, NS = 2: one wavefront per block
  c256y   (32, 256, 2)             NS = 16, 512 threads: the benchmark's y tile;  c256z (32, 2, 256) the same on z lines
  c512y   (32, 512, 2)             NS = 32, 1024 threads: the longest chunked line of bench.py --full (its C5 leg);  c512z (32, 2, 512) on z lines
  c250    (32, 250, 2)             a line off the chunk grid: refused;  c144 (32, 144, 4): 288 threads in a block of 320: refused
  codd    (130, 32, 4)             nx is no multiple of the tile width: refused
Each shape runs with the lean CG of small meshes and with cg_lean = 0, split_dot = 2 (the z.w instantiations, and k_schur_c inside CG).

Mutation check (run once on an MI355X, not part of the suite): a library whose whole-tile staged pass hands the tile body the
origin of the block's PREVIOUS tile from the second tile on fails 8 of the 33 tests -- s3, sxcd and s256z in both modes (apply error 0.65 of
max |y| on s3), the default-options test and rho on s256z: every test in which a block walks a second tile.  The 25 that pass have one tile
per block (s64, s256y), are refused the form, or run k_schur_c, which has no tile loop."""
import functools

import numpy as np
import pytest

from apply_exact import EPS, K_APPLY, exact_apply, f6_block_inputs, input_vector, rho
from helpers import make_hip, make_oracle, rel_l2
from test_gpu_line_dict import FIXED, OPTS, _applies, _oracle_applies, _same_bits, _set, block_inputs

pytestmark = pytest.mark.gpu

SPLIT = dict(cg_lean=0, split_dot=2)
MODES = {"lean": {}, "split": SPLIT}
GROUP_TOL, GROUP_ITS = 1e-30, 12
STAGED = dict(s_long=0, s_stage=1)
# name: shape, block of the inputs, options, {direction: (family, TX, NSEG, stage, full)} expected
CASES = {
    "s3": ((64, 8, 24), (8, 4, 8), dict(STAGED, s_stage_grid=3), dict(y=("s", 64, 1, 1, 1), z=("s", 64, 3, 1, 1))),
    "s64": ((64, 8, 24), (8, 4, 8), dict(STAGED, s_stage_grid=64), dict(y=("s", 64, 1, 1, 1), z=("s", 64, 3, 1, 1))),
    "sxcd": ((128, 8, 16), (16, 4, 8), dict(STAGED, s_stage_grid=5, xcd=2), dict(y=("s", 64, 1, 1, 1), z=("s", 64, 2, 1, 1))),
    "s256z": ((32, 2, 256), (8, 2, 8), dict(STAGED, s_stage_grid=1), dict(z=("s", 32, 32, 1, 1))),
    "s256y": ((32, 256, 2), (8, 8, 2), dict(STAGED, s_stage_grid=2), dict(y=("s", 32, 32, 1, 1))),
    "sodd": ((130, 8, 16), (13, 4, 8), dict(STAGED), dict(y=("s", 64, 1, 0, 0), z=("s", 64, 2, 0, 0))),
    "s21": ((64, 9, 21), (8, 3, 7), dict(STAGED, s_stage_grid=2), dict(y=("s", 64, 2, 1, 0), z=("s", 64, 3, 1, 0))),
    "c32": ((32, 32, 32), (8, 8, 8), dict(s_long=1), dict(y=("c", 32, 2, 0, 1), z=("c", 32, 2, 0, 1))),
    "c256y": ((32, 256, 2), (8, 8, 2), dict(s_long=1, s_long_dirs=1), dict(y=("c", 32, 16, 0, 1))),
    "c256z": ((32, 2, 256), (8, 2, 8), dict(s_long=1, s_long_dirs=2), dict(z=("c", 32, 16, 0, 1))),
    "c512y": ((32, 512, 2), (8, 8, 2), dict(s_long=1, s_long_dirs=1), dict(y=("c", 32, 32, 0, 1))),
    "c512z": ((32, 2, 512), (8, 2, 8), dict(s_long=1, s_long_dirs=2), dict(z=("c", 32, 32, 0, 1))),
    "c250": ((32, 250, 2), (8, 10, 2), dict(s_long=1, s_long_dirs=1), dict(y=("c", 32, 16, 0, 0))),
    "c144": ((32, 144, 4), (8, 8, 4), dict(s_long=1, s_long_dirs=1), dict(y=("c", 32, 9, 0, 0))),
    "codd": ((130, 32, 4), (13, 8, 4), dict(s_long=1, s_long_dirs=1), dict(y=("c", 32, 2, 0, 0))),
}


@functools.lru_cache(maxsize=None)
def _ref(shape, block):
    """inputs and oracle side of one shape, computed once and shared by the cases on it"""
    inp = block_inputs(shape, block)
    xs, ys = _oracle_applies(inp)
    o = make_oracle(inp); o.set_tol(*FIXED); o.SolveKeff(); h = o.history()
    assert h["n_outer"] == FIXED[3]
    return dict(inp=inp, x=xs, y=ys, hk=h["k"].copy(), phi=o.phi_dofs().copy())


def _check_plan(s, want, on, split):
    """the passes named in `want` run their family on the expected tile, table-backed, with "full" as given (0 everywhere under tile_full = 0).
    k_schur_c leaves its share of x.y in the z.w form only: the last pass of a CG without the split dot product stays on k_schur_s"""
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        for d, (family, tx, nseg, stage, full) in want.items():
            p = plan[d]
            if family == "c" and in_cg and not split and d == "z":
                assert p["family"] == "s" and p["full"] == 0, (in_cg, d, p)
                continue
            assert (p["family"], p["TX"], p["NSEG"], p["stage"], p["dict"]) == (family, tx, nseg, stage, 1), (in_cg, d, p)
            assert p["full"] == (full if on else 0), (in_cg, d, p)
            if family == "s":                                       # the form is no part of the instantiation's name
                assert p["variant"] == "+".join(["nt"] + ["zw"] * p["zw"] + ["dict"] + ["stage"] * stage), (in_cg, d, p)
            else:
                assert p["early"] == 2, (in_cg, d, p)
        assert "full" not in plan["x"], plan["x"]
        if split:
            assert plan["lean"] == 0 and (not plan["in_cg"] or plan["split_dot"] == 1), plan


def _group_solves(s, xs):
    return [s.solve_group(g, np.abs(x), GROUP_TOL, GROUP_ITS) for g, x in enumerate(xs)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_whole_tile_form(name, mode):
    shape, block, opts, want = CASES[name]
    ref = _ref(shape, block)
    split = mode == "split"
    out = {}
    for on in (1, 0):                                             # a fresh handle each: the form on (where eligible), then off
        s = make_hip(ref["inp"]); _set(s, dict(OPTS, **opts, **MODES[mode], tile_full=on)); s.set_tol(*FIXED)
        _check_plan(s, want, on, split)
        y = _applies(s, ref["x"], ref["y"], f"{name} {mode} tile_full={on}")
        gs = _group_solves(s, ref["x"])
        k, n = s.solve_keff(); h = s.history()
        assert n == FIXED[3] and s.info("last_path") == 0
        out[on] = dict(y=y, gs=gs, k=k, hk=h["k"].copy(), cg=h["cg"].copy(), phi=s.get_phi().copy())
        s.close()
    a, b = out[1], out[0]
    errs = np.abs(a["hk"] / ref["hk"] - 1).max(), rel_l2(a["phi"].ravel(), ref["phi"].ravel())
    print(f"fixed work {name} {mode}: k-history {errs[0]:.3e} (bar 1e-9), flux {errs[1]:.3e} (bar 1e-8)")
    np.testing.assert_allclose(a["hk"], ref["hk"], rtol=1e-9)
    assert errs[1] < 1e-8
    _same_bits(a["y"], b["y"], name)
    for g, ((x1, i1, r1), (x0, i0, r0)) in enumerate(zip(a["gs"], b["gs"])):
        print(f"solve_group {name} {mode} g={g}: {i1} iterations, residual {r1:.6e}")
        assert i1 == i0 == GROUP_ITS and r1 == r0 and np.array_equal(x1, x0), (name, g, i1, i0, r1, r0, float(np.abs(x1 - x0).max()))
    assert a["k"] == b["k"] and np.array_equal(a["hk"], b["hk"]) and np.array_equal(a["cg"], b["cg"]) and np.array_equal(a["phi"], b["phi"])


def test_default_is_on_and_the_wavefront_scan_keeps_the_predicated_body():
    """tile_full = -1 (the default) takes the form wherever it is eligible; a pass whose summaries are scanned by whole wavefronts is not"""
    shape, block, opts, want = CASES["s3"]
    ref = _ref(shape, block)
    s = make_hip(ref["inp"]); _set(s, dict(OPTS, **opts))
    _check_plan(s, want, 1, False)
    s.set_option("s_wsmin", 3)                                    # the 3 summaries of a z line scanned by wavefronts; a y line has one
    plan = s.apply_plan(False)
    assert (plan["y"]["full"], plan["z"]["full"], plan["z"]["stage"]) == (1, 0, 1), plan
    _applies(s, ref["x"], ref["y"], "wavefront scan")
    s.close()


@pytest.mark.parametrize("name", ["s256z", "c256y"])
def test_per_component_error_at_the_benchmark_contrast(name):
    """the benchmark's tiles on the filler-contrast inputs: rho of the apply against the extended-precision apply, tests/apply_exact.py's bar"""
    shape, block, opts, want = CASES[name]
    inp = f6_block_inputs(shape, block)
    s = make_hip(inp); _set(s, dict(OPTS, **opts, tile_full=1))
    _check_plan(s, want, 1, False)
    for g in range(int(inp["ng"])):
        x = input_vector(s.n_phi, g)
        y, sc = exact_apply(inp, g, x)
        r = rho(s.schur_apply(g, x), y, sc)
        print(f"rho {name} g={g}: {r / EPS:.2f} x 2^-53 (bar {K_APPLY})")
        assert r <= K_APPLY * EPS, (g, r / EPS)
    s.close()
