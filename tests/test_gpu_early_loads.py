"""Early vector loads of the table-backed chunked y / z pass (k_schur_c EARLY in neutfem_amd/csrc/nf_kernels.h, option "c_early").

Level 1 requests x of chunk 1 behind chunk 0's loads, level 2 also y of chunk 1 ahead of chunk 1's forward sweep and y of chunk 0 ahead of
the backward half.  Only loads move, under the predicates they had: the bar between the levels is np.array_equal, not a tolerance.  Every
case first asserts through the launch-plan report (HipSolver.apply_plan) that the y and z passes are the chunked kernel on its tables at
the level under test ("family" c, "dict" 1, "early" level), outside and inside CG, and only then checks numbers:

  apply        one Schur apply per group: bit-equal to the same handle under c_early = 0, max |y - y_oracle| <= 1e-12 max |y_oracle|
  fixed work   (first three shapes) solve_keff, tol (0, 1e-11, 1e-11, 6, 3000), CG with the split dot product (cg_lean = 0): k-history, CG
               counts and flux bit-equal between c_early 0 and the level

Inputs: the block-structured cross-sections of tests/test_gpu_line_dict.py; the chunked kernel is forced onto every line length (s_long = 1).
Shapes (nx, ny, nz) / blocks -- each way a hoisted load can go wrong occurs once:

  (33, 2, 17)   / (11, 2, 17)  y lines of 2 cells: chunk 1 lies wholly beyond the line, every hoisted load is predicated off; z lines of 17: chunk 1
                               holds one cell; nx is no multiple of the tile width
  (40, 23, 40)  / (8, 23, 8)   chunk 1 partly filled and the last segment ragged, on y and on z
  (35, 17, 33)  / (7, 17, 11)  odd lengths in every direction
  (13, 130, 8)  / (13, 26, 4)  long y lines with nx below a tile (lanes outside the mesh)
  (70, 24, 260) / (10, 6, 52)  z lines beyond 256 cells: 17 segments per chunk"""
import functools

import numpy as np
import pytest

from helpers import make_hip, make_oracle, synthetic_inputs
from test_gpu_line_dict import FIXED, OPTS, block_inputs, distinct_lines

pytestmark = pytest.mark.gpu

LONG = dict(OPTS, s_long=1, cg_lean=0)      # cg_lean = 0: inside CG the passes give their shares of p.q (split dot product), which the chunked kernel needs
SHAPES = {"y2_z17": ((33, 2, 17), (11, 2, 17)), "ragged": ((40, 23, 40), (8, 23, 8)), "odd": ((35, 17, 33), (7, 17, 11)),
          "narrow": ((13, 130, 8), (13, 26, 4)), "z260": ((70, 24, 260), (10, 6, 52))}
SOLVED = ("y2_z17", "ragged", "odd")
LEVELS = (1, 2)


def _set(s, opts):
    for k, v in opts.items():
        s.set_option(k, v)


def _vectors(n_phi, ng):
    rng = np.random.default_rng(3)
    xs = []
    for g in range(ng):
        x = rng.standard_normal(n_phi); x[rng.random(n_phi) < 0.1] *= 1e-12
        x.setflags(write=False); xs.append(x)
    return xs


def _check_plan(s, level, dict_on=1, counts=None):
    """y and z of the next apply, outside and inside CG: the chunked kernel, on its tables (or not), at this level of early loads"""
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        for d in "yz":
            p = plan[d]
            assert (p["family"], p["dict"], p["early"]) == ("c", dict_on, level), (in_cg, d, p, plan["line_dict"])
        assert plan["x"]["early"] == 0, plan["x"]
        if in_cg:
            assert plan["lean"] == 0 and plan["split_dot"] == 1 and plan["y"]["zw"] == 1 and plan["z"]["zw"] == 1, plan
        if counts is not None:
            assert {d: plan["line_dict"][d] for d in "yz"} == {d: counts[d] for d in "yz"}, (plan["line_dict"], counts)


def _applies(s, xs):
    ys = [s.schur_apply(g, x) for g, x in enumerate(xs)]
    for y in ys:
        y.setflags(write=False)
    return ys


def _solve(inp, level, counts):
    s = make_hip(inp); _set(s, dict(LONG, c_early=level)); s.set_tol(*FIXED)
    _check_plan(s, level, counts=counts)
    k, n = s.solve_keff(); h = s.history()
    out = dict(k=k, n=n, hk=h["k"].copy(), cg=h["cg"].copy(), phi=s.get_phi().copy())
    assert n == FIXED[3] and s.info("last_path") == 0
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs, the oracle's applies, and what c_early = 0 gives (applies; the fixed-work solve on the first three shapes): computed once"""
    shape, block = SHAPES[name]
    inp = block_inputs(shape, block)
    counts = distinct_lines(inp)
    o = make_oracle(inp)
    xs = _vectors(o.n_phi, int(inp["ng"]))
    yo = [o.schur_apply(g, x) for g, x in enumerate(xs)]
    s = make_hip(inp); _set(s, dict(LONG, c_early=0))
    _check_plan(s, 0, counts=counts)
    y0 = _applies(s, xs)
    s.close()
    solve0 = _solve(inp, 0, counts) if name in SOLVED else None
    return dict(inp=inp, n=counts, x=xs, yo=yo, y0=y0, solve0=solve0)


def _against_oracle(ys, yo, label):
    for g, (y, ref) in enumerate(zip(ys, yo)):
        err = np.abs(y - ref).max() / np.abs(ref).max()
        print(f"apply {label} g={g}: max-abs error / max|y_oracle| = {err:.3e} (bar 1e-12)")
        assert np.isfinite(y).all() and err <= 1e-12, (label, g, err)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_apply(name, level):
    ref = _case(name)
    print(f"{name}: distinct lines {ref['n']}")
    _against_oracle(ref["y0"], ref["yo"], f"{name} c_early=0")
    s = make_hip(ref["inp"]); _set(s, dict(LONG, c_early=level))
    _check_plan(s, level, counts=ref["n"])
    ys = _applies(s, ref["x"])
    _against_oracle(ys, ref["yo"], f"{name} c_early={level}")
    for g, (u, v) in enumerate(zip(ys, ref["y0"])):
        assert np.array_equal(u, v), (name, level, g, float(np.abs(u - v).max()))
    s.set_option("c_early", 0)                                      # the same handle, back at level 0: the plan follows, the bits stay
    _check_plan(s, 0, counts=ref["n"])
    for g, (u, v) in enumerate(zip(_applies(s, ref["x"]), ys)):
        assert np.array_equal(u, v), (name, level, g, "same handle under c_early = 0")
    s.close()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", SOLVED)
def test_fixed_work_solve(name, level):
    ref = _case(name)
    a, b = ref["solve0"], _solve(ref["inp"], level, ref["n"])
    print(f"fixed work {name} c_early={level}: k {b['k']!r} vs {a['k']!r}, CG iterations {int(b['cg'].sum())} vs {int(a['cg'].sum())}")
    assert a["k"] == b["k"] and a["n"] == b["n"]
    assert np.array_equal(a["hk"], b["hk"]) and np.array_equal(a["cg"], b["cg"]) and np.array_equal(a["phi"], b["phi"])


def test_lines_that_do_not_repeat_report_no_early_loads():
    """no table, no early loads: the streaming instantiation has no registers for them, whatever the option says"""
    inp = synthetic_inputs(35, 17, 33, 2, seed=5)
    o = make_oracle(inp)
    xs = _vectors(o.n_phi, int(inp["ng"]))
    yo = [o.schur_apply(g, x) for g, x in enumerate(xs)]
    s = make_hip(inp); _set(s, dict(LONG, c_early=2))
    _check_plan(s, 0, dict_on=0)
    assert s.apply_plan(False)["line_dict"] == dict(x=0, y=0, z=0)
    _against_oracle(_applies(s, xs), yo, "no repeats c_early=2")
    s.close()
