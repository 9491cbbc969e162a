"""More GPU parity cases: many groups with up-scatter (SURVEY C5 at a size the oracle handles), one group, natural
(mirror) boundaries everywhere, re-build with changed cross sections, and the error behaviour of the C ABI."""
import numpy as np
import pytest

from helpers import degenerate_inputs, make_hip, make_oracle, rel_l2, solved_oracle, synthetic_inputs

pytestmark = pytest.mark.gpu


def _from_case(c):
    return dict(x_breaks=c["x_breaks"], y_breaks=c["y_breaks"], z_breaks=c["z_breaks"], D=c["D"], SigR=c["SigR"], NSF=c["NSF"], Chi=c["Chi"],
                SigS=c["SigS"], bc_attr=np.array([a for a, _ in c["bc"]]), bc_type=np.array([t for _, t in c["bc"]]), ng=c["ng"],
                coarse_factors=np.array(c["coarse_factors"]))


CHECKER_TOL = (1e-11, 1e-11, 1e-11, 1200, 3000)


def test_checkerboard_8_groups_with_upscatter():
    """SURVEY 8d C5 (512^3 x 8 groups, closed-form XS) at 24^3: Gauss-Seidel sweep over 8 groups, 8 scatter blocks"""
    from neutfem_amd import cases
    inp = _from_case(cases.synthetic_checkerboard(24, 8))
    s = make_hip(inp)
    # the 1e-8 flux bar needs both runs converged beyond it: a power iteration stopped at dphi < tol is only converged to about
    # tol / (1 - dominance ratio), ~50 tol here, so the stop tests sit at 1e-11 (at 1e-9 the two runs agreed to 5e-8, no better)
    tol = CHECKER_TOL
    o = solved_oracle(inp, 0, 0, tol, coarse=[2, 2, 2], want_J=False)       # 40 s of one core when computed live: committed (helpers.solved_oracle)
    s.set_tol(*tol)
    ko = o.k; ks, n = s.solve_keff(True, [2, 2, 2])
    assert abs(ks - ko) / ko < 1e-10 and abs(n - o.n_outer) <= 2
    assert rel_l2(s.get_phi().ravel(), o.phi_dofs().ravel()) < 1e-8
    s.close()


@pytest.mark.parametrize("ng,dirichlet", [(1, (1, 2, 3, 4, 5, 6)), (3, ()), (2, (5,))])
def test_groups_and_natural_boundaries(ng, dirichlet):
    inp = synthetic_inputs(18, 11, 13, ng, seed=40 + ng, dirichlet=dirichlet)
    o, s = make_oracle(inp), make_hip(inp)
    x = np.random.default_rng(1).standard_normal(o.n_phi)
    assert rel_l2(s.schur_apply(ng - 1, x), o.schur_apply(ng - 1, x)) < 1e-12
    tol = (1e-10, 1e-10, 1e-10, 1500, 2000)
    o.set_tol(*tol); s.set_tol(*tol)
    ko = o.SolveKeff(); ks, _ = s.solve_keff()
    assert abs(ks - ko) / ko < 1e-9
    assert rel_l2(s.get_phi().ravel(), o.phi_dofs().ravel()) < 1e-8
    s.close()


def test_rebuild_with_changed_xs_keeps_warm_start():
    """BuildMatrices does not reset has_valid_keff_ / the flux (src/NeutFEM.cpp:454-456 invalidates caches only)"""
    inp = synthetic_inputs(16, 14, 1, 2, seed=8)
    o, s = make_oracle(inp), make_hip(inp)
    tol = (1e-9, 1e-9, 1e-9, 800, 2000)
    o.set_tol(*tol); s.set_tol(*tol)
    o.SolveKeff(); s.solve_keff()
    inp["SigR"] = inp["SigR"] * 1.05
    o.get_SigR()[...] = inp["SigR"]; o.BuildMatrices()
    s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); s.build()
    ko = o.SolveKeff(); ks, n = s.solve_keff()
    assert abs(ks - ko) / ko < 1e-9 and n == o.info("last_outer")
    assert s.history()["k"][0] == pytest.approx(o.history()["k"][0], rel=1e-8) and s.history()["k"][0] != 1.0   # started from last k
    s.close()


def test_error_behaviour():
    from neutfem_amd.capi import HipSolver
    inp = synthetic_inputs(8, 6, 5, 2, seed=1)
    s = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    with pytest.raises(RuntimeError, match="nf_upload_xs first"):
        s.build()
    with pytest.raises(RuntimeError, match="nf_build first"):
        s.solve_keff()
    s.upload_xs(inp["D"], inp["SigR"], 0.0 * inp["NSF"], inp["Chi"], inp["SigS"]); s.build()
    with pytest.raises(RuntimeError, match="diverged"):            # no fission: prod_old = 0 -> k is NaN
        s.solve_keff()
    with pytest.raises(RuntimeError, match="bad arguments"):
        s.schur_apply(7, np.zeros(s.n_phi))
    bad = inp["D"].copy(); bad[1, 2, 3, 4] = 0.0                   # 1/D = inf
    with pytest.raises(RuntimeError, match="invalid cross sections: D"):
        s.upload_xs(bad, inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    bad = inp["SigS"].copy(); bad[0, 1, 0, 0, 0] = np.nan
    with pytest.raises(RuntimeError, match="invalid cross sections: SigS"):
        s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], bad)
    # a refused upload leaves the handle un-built (stale line factors must not be used with the overwritten D)
    with pytest.raises(RuntimeError, match="nf_upload_xs first"):
        s.build()
    with pytest.raises(RuntimeError, match="nf_build first"):
        s.solve_keff()
    s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); s.build()
    for key, bad_v in (("s_tx", 4), ("s_tx", 24), ("s_tx", -8), ("s_seg", 2), ("s_seg", 12)):
        with pytest.raises(RuntimeError, match=key):
            s.set_option(key, bad_v)
    s.set_option("s_tx", 8); s.set_option("s_seg", 4)               # valid overrides still give the same operator
    x = np.random.default_rng(0).standard_normal(s.n_phi)
    y8 = s.schur_apply(0, x); s.set_option("s_tx", 0); s.set_option("s_seg", 0)
    assert np.abs(y8 - s.schur_apply(0, x)).max() <= 1e-12 * np.abs(y8).max()
    s.close()
    with pytest.raises(RuntimeError, match="2 y breaks"):          # dim = 3 with a 1-entry y_breaks: the reference reads y_breaks(1)
        HipSolver(0, 0, 2, inp["x_breaks"], np.array([0.0]), inp["z_breaks"])
    with pytest.raises(RuntimeError, match="strictly increasing"):
        HipSolver(0, 0, 2, np.array([0.0, 1.0, 1.0, 2.0]), inp["y_breaks"], inp["z_breaks"])
    with pytest.raises(RuntimeError, match="out of range"):
        HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], device=99)
    long_x = np.linspace(0, 1, 4100)                               # beyond the 4096-cell x-line limit of the RT0 kernel
    t = HipSolver(0, 0, 1, long_x, np.linspace(0, 1, 3), np.array([0.0]))
    t.upload_xs(np.ones((1, 2, 4099)), np.ones((1, 2, 4099)), np.ones((1, 2, 4099)), np.ones((1, 2, 4099)), np.zeros((1, 1, 2, 4099)))
    t.build()
    with pytest.raises(RuntimeError, match="x-line kernel limit"):
        t.schur_apply(0, np.zeros(t.n_phi))
    t.close()


def test_long_segments():
    """s_seg = 16 / 32 (RT0-P0 only): the long-segment instantiations of the one-chunk kernel, base variant, against the oracle's apply"""
    inp = synthetic_inputs(20, 40, 9, 2, seed=5)
    o, s = make_oracle(inp), make_hip(inp)
    x = np.random.default_rng(2).standard_normal(o.n_phi); y = o.schur_apply(1, x)
    s.set_option("s_long", 0)                                      # the one-chunk kernel whatever the environment forces (the chunked one has no s_seg)
    for seg in (16, 32):
        s.set_option("s_seg", seg)
        plan = s.apply_plan()
        assert all(plan[d]["family"] == "s" and plan[d]["SEG"] == seg and plan[d]["variant"] == "" for d in "yz"), plan
        assert rel_l2(s.schur_apply(1, x), y) < 1e-12
    s.close()


@pytest.mark.parametrize("nx,rt", [(1500, 0), (2100, 0), (3000, 0), (700, 1)])
def test_long_x_lines(nx, rt):
    """x lines beyond 1024 cells (NCH = 16 / 32 chunks per lane; RT1 up to 1024): apply and group solve against the oracle"""
    inp = synthetic_inputs(nx, 3, 1, 1, seed=nx, dirichlet=(1, 2, 3))
    o, s = make_oracle(inp, rt, rt), make_hip(inp, rt, rt)
    x = np.random.default_rng(2).standard_normal(o.n_phi)
    assert rel_l2(s.schur_apply(0, x), o.schur_apply(0, x)) < 1e-12
    b = np.abs(x)
    o.set_tol(1e-5, 1e-10, 1e-5, 10, 4000)
    xo, _, io = o.solve_group(0, b); xs, is_, _ = s.solve_group(0, b, 1e-10, 4000)
    assert rel_l2(xs, xo) < 1e-7 and abs(is_ - io) <= max(3, 0.03 * io)
    s.close()


@pytest.mark.parametrize("rt", [0, 2])
@pytest.mark.parametrize("shape", [(4, 1, 3), (1, 5, 1), (1, 1, 7), (1, 1, 1), (1, 4, 6), (2, 1, 2), (1, 1, 2), (1, 2, 1), (5, 1, 1)])
def test_single_cell_axes(shape, rt):
    """one cell along x and / or y and / or z (lines of one cell, one line per pass, a 3D mesh with ny = 1 ...)"""
    inp = degenerate_inputs(*shape)
    o, s = make_oracle(inp, rt, rt), make_hip(inp, rt, rt)
    assert (s.dim, s.nx, s.ny, s.nz) == (o.dim, o.nx, o.ny, o.nz)
    x = np.random.default_rng(0).standard_normal(o.n_phi)
    assert rel_l2(s.schur_apply(1, x), o.schur_apply(1, x)) < 1e-13
    tol = (1e-10, 1e-10, 1e-10, 200, 500)
    o.set_tol(*tol); s.set_tol(*tol)
    ko = o.SolveKeff(); ks, n = s.solve_keff()
    # both sides iterate until dk, dphi < 1e-10 with CG solves of the same relative accuracy: the last outers sit in the noise of
    # the inner solves, so the stop lands within a Chebyshev cycle of the oracle's and the answers agree to the tolerance
    assert abs(n - o.info("last_outer")) <= max(2, 0.15 * o.info("last_outer")) and abs(ks - ko) / ko < 1e-10
    assert rel_l2(s.get_phi().ravel(), o.phi_dofs().ravel()) < 1e-9
    s.close()


def test_coarsen_and_prolong_entry_points():
    """nf_coarsen + nf_solve_keff(coarse) + nf_prolong + nf_solve_keff(fine) by hand = SolveKeff(use_coarse_init=True, factors)
    (src/NeutFEM.cpp:1665-1670, 2380-2611: coarse tolerances x10, max_outer / 2, k seeded by the coarse k); nf_timers"""
    inp = synthetic_inputs(12, 10, 8, 2, seed=31)
    tol = (1e-9, 1e-9, 1e-9, 400, 2000)
    a = make_hip(inp); a.set_tol(*tol)
    ka, na = a.solve_keff(True, [2, 2, 2])
    b = make_hip(inp); b.set_tol(*tol)
    c = b.coarsen(2, 2, 2)
    assert (c.nx, c.ny, c.nz, c.n_phi) == (6, 5, 4, 120)
    c.set_linear_solver(6); c.set_tol(1e-8, 1e-8, 1e-8, 200, 2000)
    kc, nc = c.solve_keff()
    assert nc == a.history()["coarse_outer"]
    b.prolong_from(c); b.set_warm_state(1, kc)
    kb, nb = b.solve_keff()
    assert nb == na and abs(kb - ka) / ka < 1e-13
    assert rel_l2(b.get_phi().ravel(), a.get_phi().ravel()) < 1e-12
    t = b.timers()
    assert t["last_outer"] == nb and t["last_cg_total"] == int(b.history()["cg"].sum()) and "schur_x" in t
    with pytest.raises(RuntimeError, match="do not divide"):
        b.coarsen(5, 2, 2)
    c.close(); a.close(); b.close()


def test_no_device_memory_leak():
    """create / build / solve (every path that allocates lazily: coarse team, diagonal cache + device outer loop, CMFD, adjoint,
    currents, slab team with comm stream) / destroy, 12 times: free HBM must come back"""
    from neutfem_amd import capi
    from neutfem_amd.capi import HipTeam
    inp = synthetic_inputs(24, 20, 64, 2, seed=4)

    def cycle():
        s = make_hip(inp); s.set_tol(1e-6, 1e-6, 1e-6, 12, 500)
        s.solve_keff(True, [2, 2, 2]); s.solve_keff(use_diag=True); s.solve_keff(use_diag=True, use_cmfd=True)
        s.solve_adjoint(True, True); s.get_J(); s.coarsen(2, 2, 2).close(); s.close()
        t = HipTeam(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], [(0, 32), (32, 64)])
        t.set_linear_solver(6)
        for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
            t.set_bc(int(a), int(ty))
        t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); t.build()
        t.set_tol(1e-6, 1e-6, 1e-6, 6, 500); t.solve_keff(True, [2, 2, 2]); t.get_J_local(); t.close()

    cycle()                                                       # first cycle: runtime pools, code objects
    free0, total = capi.mem_info(0)
    for _ in range(12):
        cycle()
    free1, _ = capi.mem_info(0)
    assert free0 - free1 < 32 << 20, f"leaked {(free0 - free1) / 2**20:.1f} MiB over 12 cycles"


def test_progress_callback_fires_during_the_host_driven_solve():
    """VERDICT r3 "missing" 4: the reference prints its progress line every 5th outer WHILE it solves (src/NeutFEM.cpp:1791-1796); the
    module printed them after the solve, so a 200-outer run on a big mesh was silent for a minute.  nf_set_progress_callback is called after
    every outer of the host-driven loop (what every big mesh runs) with the values the history records; the in-kernel paths (milliseconds)
    do not call back and are printed from the history."""
    import ctypes as C
    inp = synthetic_inputs(20, 18, 16, 2, seed=5)
    s = make_hip(inp)
    s.set_option("resident", 0); s.set_option("keff_xcd", 0)       # the host-driven outer loop, as on meshes beyond 28 k unknowns per group
    s.set_tol(1e-7, 1e-6, 1e-6, 60, 1000)
    seen = []
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double)
    cb = CB(lambda user, it, k, dk, dphi: seen.append((it, k, dk, dphi)))
    s._chk(s.L.nf_set_progress_callback(s.h, C.cast(cb, C.c_void_p), None))
    k, n = s.solve_keff()
    h = s.history()
    assert s.info("last_path") == 0 and [t[0] for t in seen] == list(range(n))
    assert np.array_equal([t[1] for t in seen], h["k"]) and np.array_equal([t[2] for t in seen], h["dk"]) and np.array_equal([t[3] for t in seen], h["dphi"])
    seen.clear(); s.reset_flux(); s.set_option("keff_xcd", 1)
    s.solve_keff()
    assert s.info("last_path") == 3 and not seen                   # one launch for the whole SolveKeff: nothing to call back from
    s._chk(s.L.nf_set_progress_callback(s.h, None, None))
    s.close()
