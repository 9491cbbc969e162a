"""GPU parity tests: the HIP path (through the C ABI, neutfem_amd.capi) against the CPU oracle on the same
inputs.  Bars (BASELINE.json north_star): k-eff within 1 pcm, flux within 1e-8 relative L2.  The operator
level is checked much tighter (1e-12) because it is the same arithmetic in a different summation order."""
import os

import numpy as np
import pytest

from apply_exact import EPS, K_APPLY, ExactApply, rho
from helpers import TEST_TOL, load_golden, load_inputs, make_hip, make_oracle, rel_l2, synthetic_inputs

pytestmark = pytest.mark.gpu

PCM = 1e-5


def _apply_case(inp, tol=1e-12):
    """normwise against the oracle, and per component against the extended-precision apply: rho = max_i |y_i - y_exact,i| / s_i with s_i the
    magnitude of the terms that form y_i (tests/apply_exact.py; bar and its measurement in tests/test_gpu_apply_exact.py).  The normwise
    bar alone sees only the largest entries -- on IAEA-3D, with its filler of Sigma_R = 1e15, 30 % of the cells"""
    o, s = make_oracle(inp), make_hip(inp)
    rng = np.random.default_rng(3)
    for g in range(int(inp["ng"])):
        x = rng.standard_normal(o.n_phi)
        x[rng.random(o.n_phi) < 0.1] *= 1e-12            # dynamic range like CG directions near void cells
        ya, yb = s.schur_apply(g, x), o.schur_apply(g, x)
        assert np.abs(ya - yb).max() <= tol * np.abs(yb).max(), (g, np.abs(ya - yb).max() / np.abs(yb).max())
        ye, sc = ExactApply(inp, g).apply(x)
        r, ro = rho(ya, ye, sc), rho(yb, ye, sc)
        print(f"RHO parity g={g}: gpu {r:.2e} = {r / EPS:.1f} x 2^-53 (bar {K_APPLY}), oracle {ro / EPS:.1f} x 2^-53")
        assert r <= K_APPLY * EPS and r <= 100 * max(ro, EPS), (g, r / EPS, ro / EPS)
    s.close()


@pytest.mark.parametrize("name", ["iaea2d", "iaea3d", "iaea3d_1x1", "zion2d", "biblis2d", "koeberg2d"])
def test_schur_apply_benchmarks(name):
    _apply_case(load_inputs(name))


@pytest.mark.parametrize("shape", [(7, 1, 1), (64, 1, 1), (37, 5, 1), (38, 38, 1), (130, 3, 1), (3, 130, 1), (257, 4, 3),
                                   (5, 4, 300), (16, 70, 9), (33, 17, 21), (256, 8, 8), (2, 2, 2), (520, 2, 2), (1, 1, 1)])
def test_schur_apply_shapes(shape):
    nx, ny, nz = shape
    if nx == 1:
        nx = 2
    _apply_case(synthetic_inputs(nx, ny, nz, 2, seed=nx + 7 * ny + 13 * nz))


def test_schur_apply_mixed_bc():
    # Dirichlet only on some sides, MIRROR (natural) elsewhere
    inp = synthetic_inputs(20, 18, 10, 1, seed=5, dirichlet=(1, 4, 5))
    _apply_case(inp)
    inp = synthetic_inputs(24, 12, 1, 1, seed=6, dirichlet=(2, 3))
    _apply_case(inp)


def test_schur_linearity_and_symmetry_large():
    # size-independent properties at a size the oracle is not run on: S is linear and symmetric
    inp = synthetic_inputs(128, 96, 80, 1, seed=11)
    s = make_hip(inp)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(s.n_phi), rng.standard_normal(s.n_phi)
    Sx, Sy, Sxy = s.schur_apply(0, x), s.schur_apply(0, y), s.schur_apply(0, 2.0 * x - 3.0 * y)
    assert rel_l2(Sxy, 2.0 * Sx - 3.0 * Sy) < 1e-12
    assert abs(y @ Sx - x @ Sy) <= 1e-11 * abs(y @ Sx)
    assert x @ Sx > 0
    s.close()


def test_full_size_256cube_properties():
    """BASELINE config 3 at full size (IAEA-3D resampled to 256^3, 16.8 M cells, the bench workload), where the oracle is not
    run: size-independent properties.  S_g is linear, symmetric and positive definite; the 2-slab partition-method apply
    equals the undivided one; a CG solve really leaves |S x - b| <= tol |b| (checked with a separate apply); and one power
    iteration keeps the Rayleigh-quotient identity k_new = k * sum(M_f phi_new) / sum(M_f phi_old) (src/NeutFEM.cpp:1766-1774)."""
    from bench import make_solver
    from neutfem_amd import cases
    from neutfem_amd.capi import HipTeam
    case = cases.iaea3d_resampled(256)
    s = make_solver(case, 0)
    n = s.n_phi
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    for g in range(2):
        Sx, Sy, Sxy = s.schur_apply(g, x), s.schur_apply(g, y), s.schur_apply(g, 2.0 * x - 3.0 * y)
        assert rel_l2(Sxy, 2.0 * Sx - 3.0 * Sy) < 1e-12
        assert abs(y @ Sx - x @ Sy) <= 1e-10 * abs(y @ Sx)
        assert x @ Sx > 0
    b = np.abs(y)
    xs, its, res = s.solve_group(0, b, 1e-6, 3000)
    assert 0 < its < 3000 and res < 1e-6
    assert np.linalg.norm(s.schur_apply(0, xs) - b) < 1.05e-6 * np.linalg.norm(b)
    # one outer iteration from the flat flux: k stays frozen on outer 0 (:1774) and the history records |k_new - k|
    s.set_tol(0.0, 1e-4, 1e-4, 1, 1000)
    k, n_out = s.solve_keff()
    h = s.history()
    assert n_out == 1 and k == 1.0 and h["dk"][0] > 0 and np.isfinite(h["dphi"][0])
    phi = s.get_phi()
    assert np.isfinite(phi).all() and abs(np.linalg.norm(phi) - 1.0) < 1e-12          # normalised iterate (:1780-1784)
    s.close()
    # the same operator in BASELINE config 3's own layout: 8 z-slabs of 32 planes (partition method, loopback on this GPU; slabs of 32
    # planes take the single-exchange path: separator coupling 0.268^32), and cut into two slabs of 128
    for planes in ([(32 * i, 32 * i + 32) for i in range(8)], [(0, 128), (128, 256)]):
        t = HipTeam(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], planes)
        t.set_linear_solver(6)
        for a_, ty in case["bc"]:
            t.set_bc(a_, ty)
        t.upload_xs_global(case["D"], case["SigR"], case["NSF"], case["Chi"], case["SigS"]); t.build()
        yt = t.schur_apply(1, x.reshape(256, 256, 256))
        assert rel_l2(yt.ravel(), Sx) < 1e-12, len(planes)        # Sx = group 1 from the loop above
        t.close()


@pytest.mark.parametrize("name", ["iaea2d", "iaea3d_1x1", "zion2d"])
def test_cg_solve_group(name):
    inp = load_inputs(name)
    o, s = make_oracle(inp), make_hip(inp)
    o.set_tol(*TEST_TOL)
    rng = np.random.default_rng(1)
    rhs = np.abs(rng.standard_normal(o.n_phi))
    for g in range(int(inp["ng"])):
        xo, _, its_o = o.solve_group(g, rhs)
        xs, its_s, res = s.solve_group(g, rhs, TEST_TOL[1], TEST_TOL[4])
        if name.startswith("iaea3d"):           # rounding-sensitive CG path (void cells), see _keff_case
            assert abs(its_s - its_o) <= 0.2 * its_o, (its_s, its_o)
        else:
            assert its_s == its_o
        assert rel_l2(xs, xo) < (1e-10 if its_s == its_o else 20 * TEST_TOL[1])
        assert res < TEST_TOL[1]
        # the returned iterate really solves S x = b to the requested tolerance (independent check)
        assert np.linalg.norm(o.schur_apply(g, xs) - rhs) < 1.01 * TEST_TOL[1] * np.linalg.norm(rhs)
    # zero right-hand side: the |p.Sp| < 1e-30 guard (src/solvers.cpp:605) must give x = 0 after 0 iterations
    xs, its_s, _ = s.solve_group(0, np.zeros(o.n_phi), 1e-4, 10)
    assert its_s == 0 and not xs.any()
    s.close()


def _spread(key):
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "rounding_spread.json")) as f:
        return json.load(f)[key]


def _keff_case(name, run, idx):
    """HIP SolveKeff vs the committed golden vector AND vs the oracle run live on the same input.

    k-eff must agree within 1 pcm always.  The flux bar of 1e-8 applies when both sides followed the same
    iteration path (identical CG counts) or at tight tolerances.  IAEA-3D's void cells (Sigma = 1e15,
    tests/iaea3d/iaea3d.py:254) make unpreconditioned CG rounding-sensitive: merely compiling the oracle
    with FMA contraction changes its CG counts, so at the drivers' loose tolerances two
    correct implementations differ by a fraction of tol_flux there."""
    inp = load_inputs(name)
    s = make_hip(inp)
    s.set_tol(*run["tol"])
    k, n = s.solve_keff(run["coarse"], [int(v) for v in inp["coarse_factors"]], run["diag"])
    h = s.history()
    phi = s.get_phi().ravel()
    assert abs(k - run["keff"]) / run["keff"] < PCM, (k, run["keff"])
    assert h["coarse_outer"] == run["coarse_outer"]
    gold_cg = np.array(run["cg"]).reshape(-1, h["cg"].shape[1])
    same_path = n == run["n_outer"] and np.array_equal(h["cg"], gold_cg)
    if not same_path:
        # IAEA-3D only: rounding-sensitive inner CG (void cells) -> CG counts differ, and with them the outer at which a stop test
        # that sits in the noise of those solves is met (a few per cent of the outers at tight tolerances)
        assert name.startswith("iaea3d"), "outer and CG counts must match on well-conditioned benchmarks"
        assert abs(n - run["n_outer"]) <= max(1, 0.05 * run["n_outer"]), (n, run["n_outer"])
        m = min(n, run["n_outer"])
        assert abs(int(h["cg"][:m].sum()) - int(gold_cg[:m].sum())) <= 0.15 * gold_cg[:m].sum()
    # same path: 1e-8.  Different path (IAEA-3D only): the bar is MEASURED, not guessed -- three times the distance at which two correct
    # builds of the oracle itself (with / without FMA contraction, tests/test_rounding_sensitivity.py -> tests/golden/rounding_spread.json)
    # end on this very run: 6.6e-5 / 6.5e-5 on IAEA-3D 38x38x19 with / without coarse start, 1.5e-7 on the 1x1 mesh, 1.5e-8 on its tight run
    bar = 1e-8 if same_path else max(1e-8, 3.0 * _spread(f"{name}:{idx}")["flux_rel_l2"])
    m = min(n, run["n_outer"])
    np.testing.assert_allclose(h["k"][:m], run["k_hist"][:m], rtol=1e-9 if same_path else 5e-5)   # intermediate iterates: tolerance-limited
    d_gold = rel_l2(phi[::run["phi_stride"]], run["phi_samples"])
    print(f"{name}:{idx} same_path={same_path} flux rel-L2 vs golden {d_gold:.3e} (bar {bar:.1e}), k {k:.10f} vs {run['keff']:.10f}, outers {n} vs {run['n_outer']}")
    assert d_gold < bar
    o = make_oracle(inp)
    o.set_tol(*run["tol"])
    ko = o.SolveKeff(run["coarse"], [int(v) for v in inp["coarse_factors"]] if run["coarse"] else [], run["diag"])
    assert abs(k - ko) / ko < PCM
    assert rel_l2(phi, o.phi_dofs().ravel()) < bar
    s.close()
    return k


def _rt0_runs(name):
    """(index in the golden file, run): the index is the key of the run's measured rounding spread"""
    return [(i, r) for i, r in enumerate(load_golden(name)["runs"]) if r["rt"] == 0 and r["p"] == 0]


@pytest.mark.parametrize("name,idx", [(n, i) for n in ["iaea2d", "iaea3d", "iaea3d_1x1", "koeberg2d", "biblis2d", "zion2d"]
                                      for i in range(len(_rt0_runs(n)))])
def test_solve_keff_golden(name, idx):
    i, run = _rt0_runs(name)[idx]
    _keff_case(name, run, i)


def test_iaea3d_tight_tolerance_flux_parity():
    """BASELINE config 2 (IAEA-3D RT0-P0, full Schur path): the 1e-8 flux / 1 pcm bar at tolerances tight enough
    that the comparison is not limited by the stopping tests."""
    inp = load_inputs("iaea3d_1x1")
    o, s = make_oracle(inp), make_hip(inp)
    tol = (1e-12, 1e-12, 1e-12, 2000, 2000)
    o.set_tol(*tol); s.set_tol(*tol)
    ko = o.SolveKeff(); ks, n = s.solve_keff()
    assert abs(ks - ko) / ko < 1e-9
    assert rel_l2(s.get_phi().ravel(), o.phi_dofs().ravel()) < 1e-8
    s.close()


@pytest.mark.parametrize("name", ["iaea2d", "iaea3d_1x1"])
def test_diagonal_cache_and_current(name):
    inp = load_inputs(name)
    o, s = make_oracle(inp), make_hip(inp)
    for g in range(2):
        np.testing.assert_allclose(s.diagonal_cache(g), o.diag_cache(g), rtol=1e-13)
    assert not s.get_J().any()                         # Sol_J_ = 0 before any solve (src/NeutFEM.cpp:232-235)
    for diag in (True, False):
        o.reset_flux(); s.reset_flux()
        o.set_tol(*TEST_TOL); s.set_tol(*TEST_TOL)
        o.SolveKeff(False, [], diag); s.solve_keff(False, [], diag)
        Jo, Js = o.J_dofs(), s.get_J()
        # diagonal path: no inner iteration -> rounding-level; full path: 1e-8 when the CG path is identical
        same = np.array_equal(s.history()["cg"], o.history()["cg"].astype(int))
        assert rel_l2(Js, Jo) < (1e-11 if diag else (1e-8 if same else 0.1 * TEST_TOL[1]))
    s.close()


def test_warm_start_and_coarse_api():
    inp = load_inputs("iaea2d")
    o, s = make_oracle(inp), make_hip(inp)
    o.set_tol(*TEST_TOL); s.set_tol(*TEST_TOL)
    k1o = o.SolveKeff(); k1s, n1 = s.solve_keff()
    k2o = o.SolveKeff(); k2s, n2 = s.solve_keff()              # second call starts from last k / flux (has_valid_keff_)
    assert abs(k1s - k1o) < 1e-9 and abs(k2s - k2o) < 1e-9
    assert n2 == o.info("last_outer") and n2 < n1
    kco, pco = o.SolveCoarse([2, 2, 1]); kcs, pcs = s.solve_coarse([2, 2, 1])
    assert abs(kcs - kco) < 1e-9 and rel_l2(pcs, pco) < 1e-8
    # factors that do not divide the mesh -> (1.0, current flux) (src/NeutFEM.cpp:2402-2407)
    kcs, pcs = s.solve_coarse([3, 3, 1])
    assert kcs == 1.0 and rel_l2(pcs, s.get_phi().ravel()) == 0.0
    s.close()


def test_pybind_module_end_to_end():
    """the reference's Python surface: same calls as tests/iaea2d/iaea2d.py:260-361"""
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    inp = load_inputs("iaea2d")
    m = ns.NeutFEM(0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    m.set_verbosity(ns.VerbosityLevel.SILENT)
    m.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    for b in (ns.BoundaryID.LEFT_2D, ns.BoundaryID.RIGHT_2D, ns.BoundaryID.TOP_2D, ns.BoundaryID.BOTTOM_2D):
        m.set_bc(int(b), ns.BCType.DIRICHLET, 0.0)
    m.get_D()[...] = inp["D"]; m.get_SigR()[...] = inp["SigR"]; m.get_NSF()[...] = inp["NSF"]
    m.get_Chi()[...] = inp["Chi"]; m.get_SigS()[...] = inp["SigS"]
    m.BuildMatrices()
    m.set_tol(*TEST_TOL)
    k = m.SolveKeff(use_coarse_init=True, coarse_factors=[2, 2, 1])
    run = _rt0_runs("iaea2d")[0][1]
    assert abs(k - run["keff"]) / run["keff"] < PCM
    phi = m.get_flux()
    assert phi.shape == (2, 38, 38)
    assert rel_l2(phi.ravel()[::run["phi_stride"]], run["phi_samples"]) < 1e-8
    assert m.GetLastKeff() == k
    ka = m.SolveAdjoint(normalize_to_direct=True, use_direct_keff=True)      # tests/iaea2d/iaea2d.py:367-371 with --use-direct-keff
    assert ka == k and m.GetLastKeffAdjoint() == k
    fa = m.get_flux_adj()
    assert fa.shape == (2, 38, 38) and np.isfinite(fa).all() and fa.max() > 0
    vol = np.outer(np.diff(inp["y_breaks"]), np.diff(inp["x_breaks"]))
    assert abs((phi * fa * vol).sum() - 1.0) < 1e-10                         # <phi, phi+> = 1 (src/NeutFEM.cpp:2020-2066)
    # ExportVTK(export_adjoint=True) after SolveAdjoint: Flux_adj_g* fields hold the adjoint DOF-0 values (src/NeutFEM.cpp:2206-2214)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        m.ExportVTK(os.path.join(td, "adj"), export_flux=True, export_current=False, export_xs=False, export_adjoint=True)
        txt = open(os.path.join(td, "adj.vtk")).read().split("\n")
        for g in range(2):
            i = txt.index(f"SCALARS Flux_adj_g{g} double 1")
            vals = np.array([float(v) for v in txt[i + 2:i + 2 + 38 * 38]])
            assert np.abs(vals - fa[g].ravel()).max() <= 5.1e-7                         # std::fixed, 6 decimals (set by the header line, :2160)
        m.ExportFluxVTK(os.path.join(td, "adj2"), adjoint=True)
        assert "Flux_adj_g1" in open(os.path.join(td, "adj2.vtk")).read()
        m.reset_flux()                                                       # has_valid_adjoint_ = false (:347-354)
        m.ExportVTK(os.path.join(td, "adj3"), True, False, False, True)
        assert "Flux_adj_g0" not in open(os.path.join(td, "adj3.vtk")).read()


def test_vtk_export_currents(tmp_path):
    """cell-centred currents in the VTK file = face averages of the oracle's Sol_J_ (src/NeutFEM.cpp:2215-2246)"""
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    inp = synthetic_inputs(7, 6, 5, 2, seed=12)
    o = make_oracle(inp)
    m = ns.NeutFEM(0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    m.set_verbosity(ns.VerbosityLevel.SILENT); m.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    for a in inp["bc_attr"]:
        m.set_bc(int(a), ns.BCType.DIRICHLET, 0.0)
    m.get_D()[...] = inp["D"]; m.get_SigR()[...] = inp["SigR"]; m.get_NSF()[...] = inp["NSF"]; m.get_Chi()[...] = inp["Chi"]; m.get_SigS()[...] = inp["SigS"]
    m.BuildMatrices()
    tol = (1e-10, 1e-10, 1e-10, 800, 2000)
    m.set_tol(*tol); o.set_tol(*tol)
    k = m.SolveKeff(); ko = o.SolveKeff()
    m.ExportVTK(str(tmp_path / "c"), export_flux=True, export_current=True, export_xs=False)
    txt = open(str(tmp_path / "c.vtk")).read().split("\n")
    assert txt[1] == f"NeutFEM Output - k-eff={k:.6f}"
    i = txt.index("VECTORS Current_g1 double")
    got = np.array([[float(v) for v in line.split()] for line in txt[i + 1:i + 1 + 210]])
    J = o.J_dofs()[1]; nx, ny, nz = 7, 6, 5; njx = (nx + 1) * ny * nz; njy = nx * (ny + 1) * nz
    exp = np.zeros((nz, ny, nx, 3))
    for kz in range(nz):
        for j in range(ny):
            for i_ in range(nx):
                fx = (kz * ny + j) * (nx + 1) + i_; fy = njx + (kz * (ny + 1) + j) * nx + i_; fz = njx + njy + (kz * ny + j) * nx + i_
                exp[kz, j, i_] = [0.5 * (J[fx] + J[fx + 1]), 0.5 * (J[fy] + J[fy + nx]), 0.5 * (J[fz] + J[fz + nx * ny])]
    assert np.abs(got - exp.reshape(-1, 3)).max() <= 1e-6 * max(1.0, np.abs(exp).max())      # file holds 6 decimals


@pytest.mark.parametrize("name,rt", [("iaea2d", 0), ("koeberg2d", 0), ("iaea2d", 1)])
def test_solve_adjoint(name, rt):
    """SolveAdjoint (src/NeutFEM.cpp:1877-2082).  use_direct_keff=True (fixed k, no Chebyshev) converges and is compared in
    full; with a free k the reference's iteration diverges once its Chebyshev step starts at outer 5, so only the
    pre-Chebyshev iterates are compared there."""
    inp = load_inputs(name)
    o, s = make_oracle(inp, rt, rt), make_hip(inp, rt, rt)
    o.set_tol(*TEST_TOL); s.set_tol(*TEST_TOL)
    f = [int(v) for v in inp["coarse_factors"]]
    ko = o.SolveKeff(True, f); ks, _ = s.solve_keff(True, f)
    ka_o = o.SolveAdjoint(True, True); ka_s, n = s.solve_adjoint(True, True)
    assert ka_o == ko and ka_s == ks
    assert n == o.info("last_outer")
    assert rel_l2(s.get_phi_adj().ravel(), o.phi_adj_dofs().ravel()) < 1e-7
    o.set_tol(1e-5, 1e-4, 1e-4, 5, 1000); s.set_tol(1e-5, 1e-4, 1e-4, 5, 1000)      # 5 outers: before the Chebyshev step
    o.SolveAdjoint(False, False); s.solve_adjoint(False, False)
    np.testing.assert_allclose(s.history()["k"], o.history()["k"], rtol=1e-8)
    assert rel_l2(s.get_phi_adj().ravel(), o.phi_adj_dofs().ravel()) < 1e-7
    s.close()


@pytest.mark.parametrize("variant", ["default", "plain_loads_split_dot", "c3_layout_8_slabs_of_32_planes", "c3_layout_two_reductions"])
def test_iaea3d_256cube_golden(variant):
    """The HEADLINE workload at its own size (IAEA-3D resampled to 256^3, 16.8 M cells, 2 groups: what bench.py times) against the
    oracle's golden run (tests/golden/make_golden_256cube.py, about an hour of one core): 2 outer iterations from the flat flux with
    the inner CG converged to 1e-10, no coarse start -- the iteration path does not hang on rounding-sensitive CG counts, so the
    k-history is compared at 2e-9 and the flux at 1e-8, per group and overall (src/NeutFEM.cpp:1694-1802, src/solvers.cpp:577-636).
      default                 the kernels and options the bench runs: streaming loads, the whole p.q summed in the last pass
      plain_loads_split_dot   the same passes with plain loads and per-pass shares of p.q (z.w form in the y / z passes: what the
                              chunked long-line passes of 512-cell meshes need)
      c3_layout_8_slabs_of_32_planes   BASELINE config 3 AS IT IS DECOMPOSED on 8 GPUs -- 8 z-slabs of 256 x 256 x 32 (here in one process:
                              interface planes by device copy, everything else as on ranks): partition-method z lines, slab passes,
                              x || y, and the teams' default CG with ONE reduction per iteration (Cg1)
      c3_layout_two_reductions         the same team with the reference recurrence (two reductions per iteration)"""
    import json
    from bench import make_solver
    from neutfem_amd import cases
    from neutfem_amd.capi import HipTeam
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_iaea3d_256cube.json")) as f:
        r = json.load(f)["runs"]["fixed"]
    case = cases.iaea3d_resampled(256)
    team = variant.startswith("c3_layout")
    if team:
        s = HipTeam(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], [(32 * i, 32 * i + 32) for i in range(8)])
        s.set_linear_solver(6)
        for a_, ty in case["bc"]:
            s.set_bc(a_, ty)
        s.upload_xs_global(case["D"], case["SigR"], case["NSF"], case["Chi"], case["SigS"]); s.build()
        s.head.set_option("cg_single_reduce", 0 if variant.endswith("two_reductions") else 1)
    else:
        s = make_solver(case, 0)
    if variant == "plain_loads_split_dot":
        s.set_option("nt_loads", 0); s.set_option("split_dot", 2)
    s.set_tol(*r["tol"])
    k, n = s.solve_keff()
    h = s.history()
    assert n == r["n_outer"] == 2
    if team:
        assert s.head.info("cg_reductions") == (2 if variant.endswith("two_reductions") else 1) and s.head.info("n_local_slabs") == 8
    else:
        assert s.info("last_path") == 0                                          # host-driven classic path: k_schur_x / k_schur_s + k_cg_* (the bench's kernels)
    np.testing.assert_allclose(h["k"], r["k_hist"], rtol=2e-9)
    assert abs(k - r["keff"]) / r["keff"] < 2e-9
    cg_g, cg_o = h["cg"].sum(), np.sum(r["cg"])
    assert abs(cg_g - cg_o) <= 0.3 * cg_o, (cg_g, cg_o)                          # void cells: CG counts are rounding-sensitive on either side (measured 2574 vs 3163)
    phi = (s.get_phi_local() if team else s.get_phi()).ravel()                 # (ng, planes, ny, nx) either way
    smp, ref = phi[::r["phi_stride"]], np.array(r["phi_samples"])
    d = rel_l2(smp, ref)
    per = phi.size // 2; cut = (per + r["phi_stride"] - 1) // r["phi_stride"]      # samples [0, cut) belong to group 0
    dg = [rel_l2(smp[:cut], ref[:cut]), rel_l2(smp[cut:], ref[cut:])]
    print(f"256^3 {variant}: k {k:.12f} vs {r['keff']:.12f}, CG {cg_g} vs {cg_o}, flux rel-L2 {d:.2e} (groups {dg[0]:.2e} / {dg[1]:.2e})")
    assert d < 1e-8 and max(dg) < 1e-8
    for g in range(2):                                                          # whole-vector checks, not only the samples
        pg = phi[g * per:(g + 1) * per]
        assert abs(pg @ pg - r["group_sq"][g]) <= 2e-8 * r["group_sq"][g] and abs(pg.sum() - r["group_sum"][g]) <= 1e-8 * abs(r["group_sum"][g])
    s.close()


@pytest.mark.parametrize("fuse3", [1, 0])
def test_iaea3d_128cube_golden(fuse3):
    """The benchmark workload at 128^3 (2.1 M cells, the generator bench.py uses at 256^3) against the oracle's golden run
    (tests/golden/make_golden_128cube.py, ~45 min of one core): full-wavefront x lines, 16-segment y / z lines, ~1500 blocks per pass
    -- a FULL solve at a size where the chip is busy, on both CG shapes (fuse3 = 1: k_apply3, two launches per iteration;
    0: the four-launch path the 256^3 bench takes).
      fixed   5 outers, CG to 1e-10, no coarse start: the iteration path is pinned, so k-history and flux are compared tightly
      driver  the reference drivers' settings (1e-5 / 1e-4, coarse start): k and flux to the accuracy such a run has (see below)"""
    import json
    from neutfem_amd import cases
    from neutfem_amd.capi import HipSolver
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_iaea3d_128cube.json")) as f:
        gold = json.load(f)["runs"]
    c = cases.iaea3d_resampled(128)
    s = HipSolver(0, 0, c["ng"], c["x_breaks"], c["y_breaks"], c["z_breaks"]); s.set_linear_solver(6)
    for a, t in c["bc"]:
        s.set_bc(a, t)
    s.upload_xs(c["D"], c["SigR"], c["NSF"], c["Chi"], c["SigS"]); s.build()
    s.set_option("cg_fuse3", fuse3); s.set_option("cg_fuse3_max_cells", 4 << 20)   # the fused launch is the default only up to 400 k cells
    r = gold["fixed"]
    s.set_tol(*r["tol"]); k, n = s.solve_keff()
    assert n == r["n_outer"] == 5
    np.testing.assert_allclose(s.history()["k"], r["k_hist"], rtol=2e-9)
    cg_g, cg_o = s.history()["cg"].sum(), np.sum(r["cg"])
    assert abs(cg_g - cg_o) <= 0.2 * cg_o, (cg_g, cg_o)           # void cells (Sigma = 1e15): CG counts are rounding-sensitive on either side
    phi = s.get_phi().ravel()
    assert rel_l2(phi[::r["phi_stride"]], r["phi_samples"]) < 1e-8
    r = gold["driver"]
    s.reset_flux(); s.set_tol(*r["tol"]); k, n = s.solve_keff(True, r["factors"])
    # The drivers' stop test (dk < 1e-5 AND dphi < 1e-4) is met on a knife edge here: dphi hovers at 1.0-1.3e-4 for a dozen outers while
    # the Chebyshev cycle swings it (measured: one build stops at outer 23 / 24 like the oracle, another -- different FMA contraction in
    # one kernel, same operator to 1e-12 -- misses it with dphi = 1.2e-4 and runs to outer 34).  Both answers are converged to the
    # tolerance: k agrees to 1.2 pcm, and that is what is asserted; the tight comparison is the `fixed` run above.
    assert 0.6 * r["n_outer"] <= n <= 2.0 * r["n_outer"], (n, r["n_outer"])
    sp = _spread("iaea3d_128cube_driver")                            # two builds of the ORACLE on this run: flux 4.3e-4 apart, k 0.72 pcm, outers 23 / 24
    assert abs(k - r["keff"]) / r["keff"] < max(PCM, 2.0 * sp["k_pcm"] * 1e-5), (k, r["keff"], n, r["n_outer"])
    # a power iteration stopped at dphi < tol_flux is converged to about tol_flux / (1 - dominance ratio) only, and on this input the inner
    # CG counts are rounding-sensitive (void cells): two correct runs end 4e-4 apart at the drivers' 1e-4 (measured); the tight bar is the
    # `fixed` run above, where the iteration path is pinned
    d = rel_l2(s.get_phi().ravel()[::r["phi_stride"]], r["phi_samples"])
    print(f"128^3 driver settings: flux rel-L2 vs oracle {d:.2e} (tol_flux {r['tol'][1]:.0e}), k {k:.9f} vs {r['keff']:.9f}, outers {n} vs {r['n_outer']}")
    assert d < 3.0 * sp["flux_rel_l2"]                               # measured oracle-vs-oracle spread (tests/golden/make_rounding_spread_128cube.py), not a guess
    s.close()
