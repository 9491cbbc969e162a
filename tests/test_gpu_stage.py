"""Staged form of the table-backed y / z passes (k_schur_s SV_STAGE in neutfem_amd/csrc/nf_kernels.h, options "s_stage", "s_stage_grid").

A block of the staged pass walks several tiles and copies the NEXT tile's vector into LDS while it scans the current one; the values it
then reads are the ones the unstaged pass loads, and every operation behind that read is the unstaged pass's.  So the bar between the two
is np.array_equal.  Every case first asserts through the launch-plan report (HipSolver.apply_plan: "stage", "blocks", "family",
"variant" per pass) what engages, outside and inside CG, and only then checks numbers:

  apply        max |y - y_oracle| <= 1e-12 max |y_oracle| on every group (the bar of tests/test_gpu_line_dict.py), bit-equal to the same
               handle under s_stage = 0
  solve_group  tolerance 1e-30 (out of CG's reach), 12 iterations: solution, iteration count and final residual bit-equal to s_stage = 0 --
               the per-tile partial sums go through alpha and beta into every later iterate
  fixed work   solve_keff, tol (0, 1e-11, 1e-11, 6, 3000): k-history, CG counts and flux bit-equal to s_stage = 0; k-history 1e-9 and flux 1e-8
               against the oracle
  rho          one shape on the filler-contrast inputs of tests/apply_exact.py: per-component error against the extended-precision apply,
               bar K_APPLY x 2^-53 (that file's)

Shapes: the smallest at which the tile loop can go wrong (a tile is TX = 64 columns wide here).
  z3     (64, 8, 24), 3 blocks     8 z tiles as 3 / 3 / 2 per block: first, middle and last tile, a block whose last tile fetches nothing;
                                   the same launch option makes the y pass (8 cells per line, one segment, 24 tiles) a staged one: "y3" checks it
  z64    (64, 8, 24), 64 blocks    more blocks than tiles: nothing is prefetched, still staged
  ragged (64, 9, 21), 2 blocks     last segment of 5 cells, odd row count: the last copy instruction of a tile is half switched off
  xcd    (128, 8, 16), 5 blocks    16 z tiles in the XCD-contiguous order (option xcd = 2): the permutation runs inside the loop
  odd    (130, 8, 16), s_stage 1   nx is no multiple of the tile width: refused, the unstaged kernel runs
Each shape runs with the lean CG of small meshes and with cg_lean = 0, split_dot = 2 (the z.w instantiation, "nt+zw+dict+stage", inside CG).

Mutation check (run once on an MI355X, not part of the suite): a library that stages tile t + blocks + 1 instead of t + blocks fails this
file -- see DESIGN.md 6d for the outcome."""
import functools

import numpy as np
import pytest

from apply_exact import EPS, K_APPLY, exact_apply, f6_block_inputs, input_vector, rho
from helpers import make_hip, make_oracle, rel_l2
from test_gpu_line_dict import FIXED, OPTS, _applies, _oracle_applies, _same_bits, _set, block_inputs

pytestmark = pytest.mark.gpu

SPLIT = dict(cg_lean=0, split_dot=2)
# name: shape, block of the inputs, options, {direction: (stage, blocks, tiles)} expected
CASES = {
    "z3": ((64, 8, 24), (8, 4, 8), dict(s_stage=1, s_stage_grid=3), dict(z=(1, 3, 8))),
    "z64": ((64, 8, 24), (8, 4, 8), dict(s_stage=1, s_stage_grid=64), dict(z=(1, 8, 8), y=(1, 24, 24))),
    "ragged": ((64, 9, 21), (8, 3, 7), dict(s_stage=1, s_stage_grid=2), dict(z=(1, 2, 9), y=(1, 2, 21))),
    "y3": ((64, 8, 24), (8, 4, 8), dict(s_stage=1, s_stage_grid=3), dict(y=(1, 3, 24))),
    "xcd": ((128, 8, 16), (16, 4, 8), dict(s_stage=1, s_stage_grid=5, xcd=2), dict(z=(1, 5, 16), y=(1, 5, 32))),
    "odd": ((130, 8, 16), (13, 4, 8), dict(s_stage=1), dict(z=(0, 24, 24), y=(0, 48, 48))),
}
MODES = {"lean": {}, "split": SPLIT}
GROUP_TOL, GROUP_ITS = 1e-30, 12


@functools.lru_cache(maxsize=None)
def _ref(shape, block):
    """inputs and oracle side of one shape, computed once and shared by the cases on it"""
    inp = block_inputs(shape, block)
    xs, ys = _oracle_applies(inp)
    o = make_oracle(inp); o.set_tol(*FIXED); o.SolveKeff(); h = o.history()
    assert h["n_outer"] == FIXED[3]
    return dict(inp=inp, x=xs, y=ys, hk=h["k"].copy(), phi=o.phi_dofs().copy())


def _check_plan(s, want, split, on=True):
    """the passes named in `want` report stage / blocks / grid as expected, run k_schur_s and name their instantiation accordingly"""
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        for d, (stage, blocks, tiles) in want.items():
            p = plan[d]
            stage, blocks = (stage, blocks) if on else (0, tiles)
            assert p["family"] == "s" and p["nt"] == 1 and p["dict"] == 1, (in_cg, d, p)
            assert p["grid"][0] * p["grid"][1] == tiles and p["grid"][2] == 1, (in_cg, d, p)     # "grid" stays the tile grid
            assert p["stage"] == stage and p["blocks"] == blocks, (in_cg, d, p)
            if split:
                assert p["zw"] == (1 if in_cg else 0), (in_cg, d, p)
            assert p["variant"] == "+".join(["nt"] + ["zw"] * p["zw"] + ["dict"] + ["stage"] * stage), (in_cg, d, p)
        if split:
            assert plan["lean"] == 0 and (not plan["in_cg"] or plan["split_dot"] == 1), plan
    return plan


def _group_solves(s, xs):
    return [s.solve_group(g, np.abs(x), GROUP_TOL, GROUP_ITS) for g, x in enumerate(xs)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_staged_pass(name, mode):
    shape, block, opts, want = CASES[name]
    ref = _ref(shape, block)
    split = mode == "split"
    s = make_hip(ref["inp"]); _set(s, dict(OPTS, **opts, **MODES[mode])); s.set_tol(*FIXED)
    plan = _check_plan(s, want, split)
    if name == "xcd":
        assert plan["z"]["xcd_order"] == 1 and plan["z"]["xcd_permutes"] == 1, plan["z"]
    if name == "odd":
        assert all(plan[d]["TX"] == 64 for d in "yz") and shape[0] % 64 != 0
    on = _applies(s, ref["x"], ref["y"], f"{name} {mode}")
    gs_on = _group_solves(s, ref["x"])
    k1, n1 = s.solve_keff(); h1 = s.history(); hk1, cg1, phi1 = h1["k"].copy(), h1["cg"].copy(), s.get_phi().copy()
    assert n1 == FIXED[3] and s.info("last_path") == 0
    errs = np.abs(hk1 / ref["hk"] - 1).max(), rel_l2(phi1.ravel(), ref["phi"].ravel())
    print(f"fixed work {name} {mode}: k-history {errs[0]:.3e} (bar 1e-9), flux {errs[1]:.3e} (bar 1e-8)")
    np.testing.assert_allclose(hk1, ref["hk"], rtol=1e-9)
    assert errs[1] < 1e-8
    s.close()
    # a fresh handle with the staged form off: the same bits everywhere
    s = make_hip(ref["inp"]); _set(s, dict(OPTS, **opts, **MODES[mode])); s.set_option("s_stage", 0); s.set_tol(*FIXED)
    _check_plan(s, want, split, on=False)
    _same_bits(on, _applies(s, ref["x"], ref["y"], f"{name} {mode} s_stage=0"), name)
    for g, ((x1, i1, r1), (x0, i0, r0)) in enumerate(zip(gs_on, _group_solves(s, ref["x"]))):
        print(f"solve_group {name} {mode} g={g}: {i1} iterations, residual {r1:.6e}")
        assert i1 == i0 == GROUP_ITS and r1 == r0 and np.array_equal(x1, x0), (name, g, i1, i0, r1, r0, float(np.abs(x1 - x0).max()))
    k0, n0 = s.solve_keff(); h0 = s.history()
    assert k0 == k1 and n0 == n1 and np.array_equal(h0["k"], hk1) and np.array_equal(h0["cg"], cg1) and np.array_equal(s.get_phi(), phi1)
    s.close()


def test_per_component_error_at_the_benchmark_contrast():
    """z3's launch on the filler-contrast inputs: rho of the staged apply against the extended-precision apply, tests/apply_exact.py's bar"""
    shape, _, opts, want = CASES["z3"]
    inp = f6_block_inputs(shape, (8, 4, 8))
    s = make_hip(inp); _set(s, dict(OPTS, **opts))
    _check_plan(s, dict(want, y=CASES["y3"][3]["y"]), False)
    for g in range(int(inp["ng"])):
        x = input_vector(s.n_phi, g)
        y, sc = exact_apply(inp, g, x)
        r = rho(s.schur_apply(g, x), y, sc)
        print(f"rho g={g}: {r / EPS:.2f} x 2^-53 (bar {K_APPLY})")
        assert r <= K_APPLY * EPS, (g, r / EPS)
    s.close()


def test_automatic_mode_needs_a_next_tile():
    """s_stage = -1 (the default): a mesh whose passes have fewer than two tiles per block keeps the unstaged launches"""
    ref = _ref(*CASES["z3"][:2])
    s = make_hip(ref["inp"]); _set(s, OPTS)
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        assert all(plan[d]["stage"] == 0 and plan[d]["blocks"] == plan[d]["grid"][0] * plan[d]["grid"][1] for d in "yz"), plan
    s.set_option("s_stage_grid", 4)                               # 8 z tiles on 4 blocks: z (the direction that ships enabled) engages, y does not
    plan = s.apply_plan(False)
    assert (plan["z"]["stage"], plan["z"]["blocks"], plan["y"]["stage"]) == (1, 4, 0), plan
    _applies(s, ref["x"], ref["y"], "automatic, 4 blocks")
    s.close()
