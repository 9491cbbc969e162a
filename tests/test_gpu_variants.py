"""Every launch variant of the Schur apply at a small shape where it really engages.

The launch code (launch_x / launch_s / team_endpoint_phase in neutfem_amd/csrc/neutfem_hip.hip) picks among dozens of kernel
instantiations from the mesh size and the nf_set_option knobs.  Forcing a big-mesh variant onto a small mesh proves nothing when the
small mesh makes the variant a no-op (an XCD tile order over 6 tiles is skipped, over exactly 8 it is the identity), so every case
here first asserts through the read-only launch-plan report (nf_apply_plan, HipSolver.apply_plan) that the variant under test is what
the next apply launches, and only then checks numbers, at the project's usual bars:

  apply        max |y - y_oracle| <= 1e-12 max |y_oracle| on every group, input with 10 % of its entries scaled by 1e-12
  twins        variants that differ in loads, block order or readback only (partials stored by position): bit-equal
  other order  variants with another summation order: rel_l2 < 1e-13
  inside CG    solve_group against the oracle's: equal iteration counts, rel_l2 < 1e-10 (on a conditioned twin of the mesh, see CG_TOL)
  fixed work   solve_keff, tol (0, 1e-11, 1e-11, 6, 3000): k-history 1e-9, flux 1e-8 against the oracle

Shapes (RT0-P0 unless said; x grids: 4 lines per block): A (130, 8, 16): y tiles 3 x 16, z tiles 3 x 8, x grid 32, chunked kernel 5 x 16 and 5 x 8, two chunks per
lane on the x lines -- every tile count a multiple of 8 with a gridDim.x that is no power of two; B (70, 24, 4): 2 x 4 (exactly 8: the
identity) and 2 x 24; C (130, 9, 7): no y / z tile count divisible by 8, the remap must fall back to the natural order; R (70, 8, 8) RT1-P1:
2 x 8 tiles and four transverse modes in gridDim.z (the slot of a partial uses blockIdx.z)."""
import functools
import math

import numpy as np
import pytest

from helpers import make_hip, make_oracle, rel_l2, synthetic_inputs
from neutfem_amd.capi import HipTeam

pytestmark = pytest.mark.gpu

A, B, C_, R = ((130, 8, 16), 0), ((70, 24, 4), 0), ((130, 9, 7), 0), ((70, 8, 8), 1)
CLASSIC = dict(resident=0, cg_fuse3=0, cg_xcd=0)                  # the four-launch CG: every pass through launch_x / launch_s
FIXED = (0.0, 1e-11, 1e-11, 6, 3000)                              # tol_keff = 0: exactly 6 outers, inner CG converged
# solve_group against the oracle's CG asks for EQUAL iteration counts and rel_l2 < 1e-10.  Both hold together only on a well-conditioned
# operator with the CG converged: the stop test then fires while the residual still falls steeply, and the two rounding histories have had
# few iterations to drift apart.  Measured on an MI355X with synthetic_inputs as it comes (cell volumes from 0.125 to 15.6, absorbers):
# 350 - 430 iterations to 1e-11, counts 1 - 4 apart (also between two GPU variants) with the solutions 4e-14 apart; the same without
# absorbers stopped at 1e-8: equal counts (147), but the unconverged iterates 2.0e-10 apart.  So the CG checks -- and only they -- run on
# a conditioned twin of the mesh: uniform, without absorbers, the removal cross-section scaled to 0.5 ... 10 per cm.  S stays the same
# operator (the line solves carry about half of every row), its condition number drops to a few tens, and CG to 1e-11 takes 40 iterations
# (RT1-P1: 110); two builds of the oracle, with and without FMA contraction, then agree in every count and to 2e-14 in the solution.
# The applies, their twins and the fixed-work solves keep synthetic_inputs as it comes.
CG_TOL, CG_MAX = 1e-11, 5000


# ---- references: computed once per mesh, shared, never modified ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(shape, ng=2, conditioned=False):
    nx, ny, nz = shape
    seed = nx + 7 * ny + 13 * nz
    if not conditioned:
        return synthetic_inputs(nx, ny, nz, ng, seed=seed)
    inp = synthetic_inputs(nx, ny, nz, ng, seed=seed, nonuniform=False, void_frac=0.0)
    inp["SigR"] = 50.0 * inp["SigR"]
    return inp


@functools.lru_cache(maxsize=None)
def _ref(shape, rt, ng=2):
    """oracle side of the applies: inputs (10 % of the entries scaled by 1e-12) and outputs per group, on synthetic_inputs as it comes"""
    o = make_oracle(_inputs(shape, ng), rt, rt)
    rng = np.random.default_rng(3)
    xs, ys = [], []
    for g in range(ng):
        x = rng.standard_normal(o.n_phi)
        x[rng.random(o.n_phi) < 0.1] *= 1e-12
        xs.append(x); ys.append(o.schur_apply(g, x))
    for a in xs + ys:
        a.setflags(write=False)
    return dict(x=xs, y=ys, ng=ng)


@functools.lru_cache(maxsize=None)
def _ref_cg(shape, rt, ng=2):
    """oracle side of the CG checks: the solve of one right-hand side per group on the conditioned twin of the mesh"""
    o = make_oracle(_inputs(shape, ng, True), rt, rt)
    rng = np.random.default_rng(5)
    rhs, sol, its = [], [], []
    o.set_tol(1e-5, CG_TOL, CG_TOL, 200, CG_MAX)
    for g in range(ng):
        b = np.abs(rng.standard_normal(o.n_phi))
        xo, _, n = o.solve_group(g, b, with_J=False)
        rhs.append(b); sol.append(xo); its.append(n)
    for a in rhs + sol:
        a.setflags(write=False)
    return dict(rhs=rhs, sol=sol, its=its, ng=ng)


@functools.lru_cache(maxsize=None)
def _ref_keff(shape, rt, ng=2, tol=FIXED, diag=False):
    o = make_oracle(_inputs(shape, ng), rt, rt); o.set_tol(*tol)
    o.SolveKeff(False, (), diag); h = o.history()
    assert h["n_outer"] == tol[3]
    return dict(hk=h["k"].copy(), cg=h["cg"].copy(), phi=o.phi_dofs().copy(), J=o.J_dofs().copy())


def _solver(shape, rt, opts, ng=2, conditioned=False):
    s = make_hip(_inputs(shape, ng, conditioned), rt, rt)
    _set(s, opts)
    return s


class _Pair:
    """a mesh and its conditioned twin under the same options: applies go to the first, CG solves to the second; the launch plan depends on
    shape and options only and must be the same for both"""

    def __init__(self, shape, rt, opts, ng=2):
        self.a, self.c = make_hip(_inputs(shape, ng), rt, rt), make_hip(_inputs(shape, ng, True), rt, rt)
        _set(self, opts)

    def set_option(self, k, v):
        self.a.set_option(k, v); self.c.set_option(k, v)

    def apply_plan(self, in_cg=False):
        plan = self.a.apply_plan(in_cg)
        assert plan == self.c.apply_plan(in_cg)
        return plan

    def schur_apply(self, g, x): return self.a.schur_apply(g, x)
    def solve_group(self, g, rhs, tol, maxit): return self.c.solve_group(g, rhs, tol, maxit)

    def close(self):
        self.a.close(); self.c.close()


def _set(s, opts):
    for k, v in opts.items():
        s.set_option(k, v)


def _applies(s, ref, label=""):
    """the apply on every group against the oracle (printed, then asserted); returns the outputs"""
    out = []
    for g in range(ref["ng"]):
        y = s.schur_apply(g, ref["x"][g])
        err = np.abs(y - ref["y"][g]).max() / np.abs(ref["y"][g]).max()
        print(f"apply {label} g={g}: max-abs error / max|y| = {err:.3e} (bar 1e-12)")
        assert np.isfinite(y).all() and err <= 1e-12, (label, g, err)
        out.append(y)
    return out


def _solves(s, ref, label="", groups=None):
    """solve_group on every group against the oracle's CG: equal iteration counts, rel_l2 < 1e-10; returns (solutions, counts)"""
    xs, ns = [], []
    for g in (range(ref["ng"]) if groups is None else groups):
        x, n, res = s.solve_group(g, ref["rhs"][g], CG_TOL, CG_MAX)
        err = rel_l2(x, ref["sol"][g])
        print(f"solve_group {label} g={g}: its {n} (oracle {ref['its'][g]}), rel_l2 = {err:.3e} (bar 1e-10)")
        assert res < CG_TOL and n == ref["its"][g], (label, g, n, ref["its"][g])
        assert err < 1e-10, (label, g, err)
        xs.append(x); ns.append(n)
    return xs, ns


def _same_bits(a, b, label):
    for g, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (label, g, float(np.abs(u - v).max()))


# ---- (a) XCD-contiguous tile order ------------------------------------------------------------------------------------------------
def _expect_xcd(shape, rt, xcd, plan):
    """what "xcd" must do on this mesh with streaming loads on: bit 0 = y passes, bit 1 = z passes, bit 2 = x pass (RT0-P0 streaming
    instantiations only); -1 = the y passes.  It permutes where the tile count is a multiple of 8 beyond 8."""
    want = dict(y=xcd < 0 or bool(xcd & 1), z=xcd >= 0 and bool(xcd & 2), x=xcd >= 0 and bool(xcd & 4) and rt == 0)
    for d in "xyz":
        p = plan[d]
        tiles = p["grid"][0] if d == "x" else p["grid"][0] * p["grid"][1]
        assert p["family"] == ("x" if d == "x" else "s"), (d, p)
        assert p["nt"] == (1 if rt == 0 else 0), (d, p)              # streaming loads: RT0-P0 instantiations
        if d != "x" and rt != 0:
            assert p["variant"] == "", (d, p)                        # higher orders: the base kernel, whatever the options ask for
        assert p["xcd_order"] == int(want[d]), (d, xcd, p)
        assert p["xcd_permutes"] == int(want[d] and tiles % 8 == 0 and tiles > 8), (d, xcd, p)
    return want


GRIDS = {A: dict(x=[32, 1, 1], y=[3, 16, 1], z=[3, 8, 1]), B: dict(x=[24, 1, 1], y=[2, 4, 1], z=[2, 24, 1]),
         C_: dict(x=[16, 1, 1], y=[3, 7, 1], z=[3, 9, 1]), R: dict(x=[16, 4, 1], y=[2, 8, 4], z=[2, 8, 4])}
# directions whose tiles must really move under "xcd" = 7
MOVES = {A: "xyz", B: "xz", C_: "x", R: "yz"}


@functools.lru_cache(maxsize=None)
def _xcd_baseline(mesh):
    """"xcd" = 0 with the streaming instantiations: the twin every tile order must reproduce to the bit"""
    (shape, rt) = mesh
    ref, cg = _ref(shape, rt), _ref_cg(shape, rt)
    s = _Pair(shape, rt, dict(CLASSIC, nt_min_cells=0, xcd=0))
    for d in "xyz":
        assert s.apply_plan()[d]["xcd_order"] == 0 and s.apply_plan(True)[d]["xcd_order"] == 0
    out = dict(y=_applies(s, ref, "xcd=0"))
    for lean in (1, 0):
        s.set_option("cg_lean", lean)
        out["lean%d" % lean] = _solves(s, cg, "xcd=0 lean=%d" % lean)[0]
    s.close()
    return out


@pytest.mark.parametrize("xcd", [1, 2, 3, 4, 7, -1])
@pytest.mark.parametrize("mesh", [A, B, C_, R], ids=["A", "B", "C", "R"])
def test_xcd_tile_order(mesh, xcd):
    (shape, rt) = mesh
    ref, cg, base = _ref(shape, rt), _ref_cg(shape, rt), _xcd_baseline(mesh)
    s = _Pair(shape, rt, dict(CLASSIC, nt_min_cells=0, xcd=xcd))
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        for d in "xyz":
            assert plan[d]["grid"] == GRIDS[mesh][d], (d, plan[d])
        want = _expect_xcd(shape, rt, xcd, plan)
        if xcd == 7:
            assert "".join(d for d in "xyz" if plan[d]["xcd_permutes"]) == MOVES[mesh], plan["passes"]
        if mesh == C_:
            assert not any(plan[d]["xcd_permutes"] for d in "yz") and any(want.values())   # requested, and must fall back to the natural order
    _same_bits(_applies(s, ref, "xcd=%d" % xcd), base["y"], "apply")
    for lean in (1, 0):
        s.set_option("cg_lean", lean)
        assert s.apply_plan(True)["lean"] == lean
        _same_bits(_solves(s, cg, "xcd=%d lean=%d" % (xcd, lean))[0], base["lean%d" % lean], "solve_group lean=%d" % lean)
    s.close()


# ---- (b) x pass, the retired two load phases --------------------------------------------------------------------------------------------------
def test_x_pass_two_load_phases():
    """The x pass once had a form with its loads in two phases around the deferred CG update (option x_two_phase): bit-equal to the one-phase
    pass and no faster, so it is gone (docs/HISTORY.md).  The key is still accepted: the plan reports no "p2" and the results do not move."""
    (shape, rt) = A
    ref, cg = _ref(shape, rt), _ref_cg(shape, rt)
    res = {}
    for p2 in (1, 0):
        s = _Pair(shape, rt, dict(CLASSIC, x_two_phase=p2, nt_min_cells=0, cg_fuse=1))
        assert s.apply_plan(True)["fused"] == 1 and s.apply_plan(True)["x"]["NCH"] == 2 and s.apply_plan(True)["x"]["nt"] == 1
        assert "p2" not in s.apply_plan(True)["x"] and "p2" not in s.apply_plan(False)["x"]
        _applies(s, ref, "x_two_phase=%d" % p2)
        res[p2] = _solves(s, cg, "x_two_phase=%d" % p2)
        s.set_option("cg_fuse", 0)
        assert "p2" not in s.apply_plan(True)["x"]
        s.close()
    assert res[1][1] == res[0][1]
    _same_bits(res[1][0], res[0][0], "x_two_phase")


# ---- (c) chunked kernel with streaming loads and XCD order ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_chunk_apply(mesh):
    (shape, rt) = mesh
    s = _solver(shape, rt, dict(s_long=0))
    assert s.apply_plan()["y"]["family"] == "s" and s.apply_plan()["z"]["family"] == "s"
    y = _applies(s, _ref(shape, rt), "s_long=0")
    s.close()
    return y


@pytest.mark.parametrize("dirs", [1, 2, 3])
@pytest.mark.parametrize("mesh", [A, C_], ids=["A", "C"])
def test_chunked_kernel_streaming_and_xcd(mesh, dirs):
    (shape, rt) = mesh
    ref, cg = _ref(shape, rt), _ref_cg(shape, rt)
    s = _Pair(shape, rt, dict(CLASSIC, s_long=1, nt_min_cells=0, s_long_dirs=dirs))
    fam = dict(y="c" if dirs & 1 else "s", z="c" if dirs & 2 else "s")
    cgrid = dict(y=[5, shape[2], 1], z=[5, shape[1], 1])
    res = {}
    for xcd in (0, -1, 3):
        _set(s, dict(xcd=xcd, cg_lean=1, split_dot=1))
        plan = s.apply_plan()
        for d in "yz":
            p = plan[d]
            assert p["family"] == fam[d] and p["nt"] == 1, (d, p)
            if fam[d] == "c":
                assert p["NCH"] == 2 and p["grid"] == cgrid[d], p
            order = xcd == 3 or (xcd == -1 and d == "y")
            tiles = p["grid"][0] * p["grid"][1]
            assert p["xcd_order"] == int(order) and p["xcd_permutes"] == int(order and tiles % 8 == 0 and tiles > 8), (d, xcd, p)
            if mesh == A and order:
                assert p["xcd_permutes"] == 1, p
        ya = _applies(s, ref, "s_long_dirs=%d xcd=%d" % (dirs, xcd))
        for u, v in zip(ya, _one_chunk_apply(mesh)):                  # another kernel, another summation order
            assert rel_l2(u, v) < 1e-13
        # inside CG the chunked kernel gives its share of p.q in the z.w form only: the split dot product of the big meshes
        _set(s, dict(cg_lean=0, split_dot=2))
        plan = s.apply_plan(True)
        assert plan["lean"] == 0 and plan["split_dot"] == 1
        for d in "yz":
            assert plan[d]["family"] == fam[d] and plan[d]["zw"] == 1, (d, plan[d])
            if fam[d] == "s":
                assert plan[d]["variant"] == ("nt+zw+dict" if plan[d]["dict"] else "nt+zw"), (d, plan[d])
        res[xcd] = (ya, _solves(s, cg, "s_long_dirs=%d xcd=%d" % (dirs, xcd))[0])
    for xcd in (-1, 3):                                            # the tile order moves no partial: stored by position
        _same_bits(res[xcd][0], res[0][0], "apply xcd=%d" % xcd)
        _same_bits(res[xcd][1], res[0][1], "solve_group xcd=%d" % xcd)
    s.close()


@pytest.mark.parametrize("shape,long_dir", [((9, 300, 4), "y"), ((9, 4, 300), "z")])
def test_chunked_kernel_thresholds_select_per_direction(shape, long_dir):
    """s_long = -1 (automatic): s_long_min_y / s_long_min are the line lengths beyond which the y / z passes take the chunked kernel.  On a
    mesh with long lines in one direction only, that direction's knob moves it across the threshold both ways and the other knob leaves it
    alone.  The short direction shows one side only: below 1024 tiles chunk_plan leaves lines of at most 256 cells to the one-chunk kernel
    whatever the threshold says, so lowering its knob to 1 must change nothing there."""
    ref = _ref(shape, 0, 1)
    other = "z" if long_dir == "y" else "y"
    mine, theirs = ("s_long_min_y", "s_long_min") if long_dir == "y" else ("s_long_min", "s_long_min_y")
    s = _solver(shape, 0, dict(s_long=-1, s_long_min_y=4, s_long_min=4), ng=1)
    y_auto = None
    for opts, fam in [({}, "c"), ({mine: 300}, "s"), ({mine: 299}, "c"), ({mine: 299, theirs: 1000000}, "c"), ({theirs: 1}, "c"), ({mine: 1000000, theirs: 4}, "s")]:
        _set(s, dict({"s_long_min_y": 4, "s_long_min": 4}, **opts))
        plan = s.apply_plan()
        assert plan[long_dir]["family"] == fam and plan[other]["family"] == "s", (opts, plan["passes"])
        y = _applies(s, ref, "%s %s" % (shape, opts))
        if fam == "c":
            if y_auto is None: y_auto = y
            _same_bits(y, y_auto, "same kernel, same launch")
        else:
            assert rel_l2(y[0], y_auto[0]) < 1e-13
    s.close()


# ---- (d) slab z passes and k_endpoint_w across several x tiles ------------------------------------------------------------------------
SLAB_SHAPE = (130, 8, 24)


def _team(inp, planes, opts):
    t = HipTeam(0, 0, int(inp["ng"]), inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], planes)
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    t.build()
    _set(t.head, opts)
    return t


@functools.lru_cache(maxsize=None)
def _undivided_apply(shape):
    s = _solver(shape, 0, {})
    y = _applies(s, _ref(shape, 0))
    s.close()
    return y


def _team_apply_matches(t, shape, label):
    ref, und = _ref(shape, 0), _undivided_apply(shape)
    nx, ny, nz = shape
    out = []
    for g in range(2):
        y = t.schur_apply(g, ref["x"][g].reshape(nz, ny, nx)).ravel()
        err = rel_l2(y, und[g])
        print(f"team apply {label} g={g}: rel_l2 against the undivided apply = {err:.3e} (bar 1e-12)")
        assert err < 1e-12, (label, g, err)
        out.append(y)
    return out


@pytest.mark.parametrize("nt_min", [None, 0])
@pytest.mark.parametrize("planes", [[(0, 12), (12, 24)], [(0, 8), (8, 16), (16, 24)]], ids=["2slabs", "3slabs"])
def test_slab_z_passes_and_endpoint_weights(planes, nt_min):
    inp = _inputs(SLAB_SHAPE)
    ref = _ref_keff(SLAB_SHAPE, 0)
    opts = {} if nt_min is None else dict(nt_min_cells=nt_min)
    nt = 0 if nt_min is None else 1
    def var(*bits):                                                # the k_schur_s variant: streaming loads ride along with whatever the pass carries
        return "+".join(b for b in ("fuse", "nt", "sr") if b in bits or (b == "nt" and nt))
    # default options: the XCD order of the z passes of small slabs is on by itself and, with 3 x 8 tiles, really permutes
    t = _team(inp, planes, opts)
    y_def = _team_apply_matches(t, SLAB_SHAPE, "default")          # prepares the team: the report needs its separator sweeps and weights
    for x in t.slabs:
        for in_cg in (False, True):
            plan = x.apply_plan(in_cg)
            assert plan["slab"] == 1
            for m in ("z1", "z2") if not in_cg else ("z2",):        # inside CG the endpoint pass is k_endpoint_w by default: below
                p = plan[m]
                assert p["family"] == "s" and p["grid"] == [3, 8, 1] and p["nt"] == nt and p["xcd_order"] == 1 and p["xcd_permutes"] == 1, (m, p)
                # outside CG both passes are the base kernel; inside, the accumulation pass leaves the three sums of the single-reduction CG
                assert p["variant"] == (var("sr") if in_cg and plan["single_reduce"] else var()), (m, in_cg, p)
    t.head.set_option("xcd", 0)
    assert all(x.apply_plan()[m]["xcd_order"] == 0 for x in t.slabs for m in ("z1", "z2"))
    _same_bits(_team_apply_matches(t, SLAB_SHAPE, "xcd=0"), y_def, "team apply, natural tile order")
    # x || y on small slabs: the y pass on its own stream into a buffer that the accumulation pass adds (another summation order)
    t.head.set_option("xcd", -1)
    assert t.head.apply_plan()["xy_overlap"] == 1
    t.head.set_option("xy_overlap_max_cells", 0)
    assert t.head.apply_plan()["xy_overlap"] == 0
    _team_apply_matches(t, SLAB_SHAPE, "xy_overlap_max_cells=0")
    t.close()
    # single-reduction CG with the endpoint pass as weighted sums: k_endpoint_w over 3 x tiles; separators folded into the accumulation pass or not
    res = {}
    for fold in (1, 0):
        t = _team(inp, planes, dict(opts, cg_single_reduce=1, endpoint_weights=1, sep_fold=fold)); t.set_tol(*FIXED)
        _team_apply_matches(t, SLAB_SHAPE, "sep_fold=%d" % fold)
        sweeps = t.head.timers()["separator_sweeps"]
        for x in t.slabs:
            plan = x.apply_plan(True)
            assert plan["single_reduce"] == 1 and plan["fused"] == 1
            assert plan["z1"]["family"] == "endpoint_w" and plan["z1"]["grid"] == [3, 8, 1], plan["z1"]
            assert plan["z2"]["family"] == "s" and plan["z2"]["nt"] == nt and plan["z2"]["xcd_permutes"] == 1, plan["z2"]
            assert plan["z2"]["fold"] == int(fold == 1 and sweeps == 0) and plan["z2"]["variant"] == var("sr"), plan["z2"]
            assert x.apply_plan(False)["z1"]["family"] == "s" and x.apply_plan(False)["z1"]["variant"] == var()   # outside CG: the chain solve, base kernel
        k, n = t.solve_keff()
        assert n == 6 and t.head.info("cg_reductions") == 1 and t.head.info("endpoint_weights") == 1
        h = t.history()
        res[fold] = (h["k"].copy(), t.get_phi_local().ravel().copy(), int(h["cg"].sum()))
        errs = (np.abs(h["k"] / ref["hk"] - 1).max(), rel_l2(res[fold][1], ref["phi"].ravel()))
        print(f"team fixed work sep_fold={fold} sweeps={sweeps}: k-history {errs[0]:.3e} (bar 1e-9), flux {errs[1]:.3e} (bar 1e-8)")
        np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
        assert errs[1] < 1e-8
        t.close()
    (h1, p1, c1), (h0, p0, c0) = res[1], res[0]
    np.testing.assert_allclose(h1, h0, rtol=1e-11)
    assert rel_l2(p1, p0) < 1e-9 and abs(c1 - c0) <= 0.02 * c0
    # the same CG with the endpoint pass as a chain solve: k_schur_s carries the fused update and r -= alpha q (fuse + sr), same bars
    t = _team(inp, planes, dict(opts, cg_single_reduce=1, endpoint_weights=0)); t.set_tol(*FIXED)
    _team_apply_matches(t, SLAB_SHAPE, "endpoint_weights=0")
    for x in t.slabs:
        plan = x.apply_plan(True)
        assert plan["single_reduce"] == 1 and plan["fused"] == 1
        assert plan["z1"]["family"] == "s" and plan["z1"]["variant"] == var("fuse", "sr") and plan["z1"]["nt"] == nt, plan["z1"]
        assert plan["z2"]["family"] == "s" and plan["z2"]["variant"] == var("sr"), plan["z2"]
        assert x.apply_plan(False)["z1"]["variant"] == var()
    k, n = t.solve_keff()
    assert n == 6 and t.head.info("cg_reductions") == 1 and t.head.info("endpoint_weights") == 0
    h = t.history()
    errs = (np.abs(h["k"] / ref["hk"] - 1).max(), rel_l2(t.get_phi_local().ravel(), ref["phi"].ravel()))
    print(f"team fixed work endpoint_weights=0: k-history {errs[0]:.3e} (bar 1e-9), flux {errs[1]:.3e} (bar 1e-8)")
    np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
    assert errs[1] < 1e-8
    t.close()


def test_slab_separator_fold_engages_on_thick_slabs():
    """sep_fold acts where no separator sweeps run (thick slabs): there the report must show the accumulation pass folding the separators, the
    knob must switch it off, and both forms give the undivided apply and the same fixed-work solve.  cg_single_reduce_max_cells: the cell
    bound of the automatic single-reduction CG (cg_single_reduce = -1)."""
    shape = (20, 8, 72)
    inp, ref = _inputs(shape), _ref_keff(shape, 0)
    res = {}
    for fold, max_cells in [(1, None), (0, None), (1, 0), (1, 1 << 30)]:
        t = _team(inp, [(0, 36), (36, 72)], dict(sep_fold=fold, **({} if max_cells is None else dict(cg_single_reduce_max_cells=max_cells)))); t.set_tol(*FIXED)
        _team_apply_matches(t, shape, "thick slabs sep_fold=%d" % fold)
        assert t.head.timers()["separator_sweeps"] == 0
        assert all(x.apply_plan(c)["z2"]["fold"] == fold for x in t.slabs for c in (False, True))
        sr = 1 if max_cells is None else int(max_cells > 0)
        assert t.head.apply_plan(True)["single_reduce"] == sr
        k, n = t.solve_keff()
        assert n == 6 and t.head.info("cg_reductions") == (1 if sr else 2)
        h = t.history()
        res[fold, max_cells] = (h["k"].copy(), t.get_phi_local().ravel().copy(), int(h["cg"].sum()))
        np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
        assert rel_l2(res[fold, max_cells][1], ref["phi"].ravel()) < 1e-8
        t.close()
    (h1, p1, c1), (h0, p0, c0) = res[1, None], res[0, None]
    np.testing.assert_allclose(h1, h0, rtol=1e-11)
    assert rel_l2(p1, p0) < 1e-9 and abs(c1 - c0) <= 0.02 * c0
    assert np.array_equal(res[1, 1 << 30][0], h1) and np.array_equal(res[1, 1 << 30][1], p1)      # the same launches as the default bound


# ---- (e) CG plumbing knobs that must not change the iterates ----------------------------------------------------------------------------
def test_cg_batch_does_not_change_the_iterates():
    """cg_batch: how many iterations are launched between two looks at the stop flag.  Iterations queued behind a converged solve exit at once."""
    (shape, rt) = B
    ref = _ref_cg(shape, rt)
    for lean in (1, 0):
        s = _solver(shape, rt, dict(CLASSIC, cg_lean=lean), conditioned=True)
        assert s.apply_plan(True)["lean"] == lean
        base = _solves(s, ref, "cg_batch default lean=%d" % lean)
        for batch in (1, 3, 1000):
            s.set_option("cg_batch", batch)
            x, n = _solves(s, ref, "cg_batch=%d lean=%d" % (batch, lean))
            assert n == base[1]
            _same_bits(x, base[0], "cg_batch=%d" % batch)
        s.close()


def test_lean_cg_size_bound_and_partial_grid():
    (shape, rt) = B
    ref = _ref_cg(shape, rt)
    s = _solver(shape, rt, dict(CLASSIC, cg_lean=0), conditioned=True)
    assert s.apply_plan(True)["lean"] == 0
    off = _solves(s, ref, "cg_lean=0")
    _set(s, dict(cg_lean=1, cg_lean_max_cells=0))                  # the mesh is beyond the bound: the same launches as cg_lean = 0
    assert s.apply_plan(True)["lean"] == 0
    _same_bits(_solves(s, ref, "cg_lean_max_cells=0")[0], off[0], "cg_lean_max_cells=0")
    s.set_option("cg_lean_max_cells", 1 << 30)
    for grid in (1, 7, 1024):                                      # number of |r|^2 partials of k_cg_rupdate: another summation order each
        s.set_option("cg_lean_grid", grid)
        assert s.apply_plan(True)["lean"] == 1
        _solves(s, ref, "cg_lean_grid=%d" % grid)
    s.close()


@pytest.mark.parametrize("path", [dict(CLASSIC), dict(resident=0, cg_fuse3=1, cg_fuse3_max_cells=4 << 20, cg_xcd=0)], ids=["classic", "fuse3"])
def test_profiled_solve_equals_unprofiled(path):
    """bench.py takes its timed steps with profile = True: event records around every prof_every-th apply and nothing else.  cg_batch = 1
    launches no iteration past convergence, so the applies of the solve are the CG iterations of its history, one tick each."""
    (shape, rt) = B
    ref = _ref_keff(shape, rt)
    s = _solver(shape, rt, dict(path, cg_batch=1)); s.set_tol(*FIXED)
    k0, n0 = s.solve_keff(); h0 = s.history(); phi0 = s.get_phi().copy()
    assert s.info("last_path") == 0 and s.profile("schur_apply")[0] == 0
    np.testing.assert_allclose(h0["k"], ref["hk"], rtol=1e-9)
    assert rel_l2(phi0.ravel(), ref["phi"].ravel()) < 1e-8
    s.close()
    for every in (1, 8):
        s = _solver(shape, rt, dict(path, cg_batch=1, prof_every=every)); s.set_tol(*FIXED)
        k, n = s.solve_keff(profile=True); h = s.history()
        assert s.info("last_path") == 0
        assert k == k0 and n == n0 and np.array_equal(h["k"], h0["k"]) and np.array_equal(h["cg"], h0["cg"]) and np.array_equal(s.get_phi(), phi0)
        tm = s.timers()["schur_apply"]
        count, ms = s.profile("schur_apply")
        total = int(h["cg"].sum())
        print(f"prof_every={every}: {count} timed applies + {tm['skipped_noop']} no-ops of {total} CG iterations, {ms:.3f} ms")
        assert count == tm["count"] > 0 and ms > 0
        assert count + tm["skipped_noop"] == math.ceil(total / every), (count, tm, total, every)
        s.close()


# ---- (f) one-XCD and resident kernels off their default sizing -------------------------------------------------------------------------
WINDOW = [((30, 28, 9), 0), ((14, 12, 6), 1)]                      # 7 560 and 8 064 unknowns per group: inside the one-XCD window


@pytest.mark.parametrize("groups", [1, 8, 24])
@pytest.mark.parametrize("mesh", WINDOW, ids=["rt0", "rt1"])
def test_one_xcd_kernels_with_other_workgroup_counts(mesh, groups):
    """cg_xcd_groups: workgroups per XCD of k_cg_xcd / k_keff_xcd (default 32).  The tasks of a solve are dealt to however many there are."""
    (shape, rt) = mesh
    ref = _ref_keff(shape, rt, tol=(0.0, 1e-11, 1e-11, 6, 5000))
    for whole in (1, 0):                                           # k_keff_xcd (the whole power iteration), k_cg_xcd under the host's outer loop
        s = _solver(shape, rt, dict(cg_xcd_groups=groups, keff_xcd=whole)); s.set_tol(0.0, 1e-11, 1e-11, 6, 5000)
        k, n = s.solve_keff(); h = s.history()
        assert n == 6 and s.info("last_path") == (3 if whole else 0)
        assert s.info("xcd_solves") == 12 and s.info("xcd_refused") == 0, (s.info("xcd_solves"), s.info("xcd_refused"))
        errs = (np.abs(h["k"] / ref["hk"] - 1).max(), rel_l2(s.get_phi().ravel(), ref["phi"].ravel()), rel_l2(s.get_J().ravel(), ref["J"].ravel()))
        print(f"cg_xcd_groups={groups} keff_xcd={whole}: k-history {errs[0]:.3e} (1e-9), flux {errs[1]:.3e} (1e-8), currents {errs[2]:.3e} (1e-7)")
        np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
        assert errs[1] < 1e-8 and errs[2] < 1e-7
        s.close()


@pytest.mark.parametrize("mesh", [((12, 11, 10), 0), ((6, 5, 4), 1)], ids=["rt0", "rt1"])
def test_resident_kernel_without_lds_staging(mesh):
    """resident_lds = 0: the one-workgroup solve keeps its vectors in global memory (and leaves the line-per-lane variant, which needs LDS)"""
    (shape, rt) = mesh
    ref = _ref_keff(shape, rt)
    res = {}
    for lds in (1, 0):
        s = _solver(shape, rt, dict(resident=1, resident_max_dofs=100000, resident_lds=lds)); s.set_tol(*FIXED)
        k, n = s.solve_keff(); h = s.history()
        assert n == 6 and s.info("last_path") == 2 and s.info("last_resident_serial") == lds
        np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
        assert rel_l2(s.get_phi().ravel(), ref["phi"].ravel()) < 1e-8
        res[lds] = (k, s.get_phi().copy())
        s.close()
    assert abs(res[0][0] - res[1][0]) / res[1][0] < 1e-10 and rel_l2(res[0][1], res[1][1]) < 1e-9


def test_diagonal_path_outer_loop_on_host_and_device():
    """outer_dev: the diagonal solver's power iteration as one device-side loop (last_path 1) or driven from the host (last_path 0)"""
    shape = (24, 20, 6)
    ref = _ref_keff(shape, 0, diag=True)
    res = {}
    for dev in (1, 0):
        s = _solver(shape, 0, dict(outer_dev=dev)); s.set_tol(*FIXED)
        k, n = s.solve_keff(False, (), True); h = s.history()
        assert n == 6 and s.info("last_path") == dev
        np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
        assert rel_l2(s.get_phi().ravel(), ref["phi"].ravel()) < 1e-8
        res[dev] = h["k"].copy()
        s.close()
    np.testing.assert_allclose(res[0], res[1], rtol=1e-9)
