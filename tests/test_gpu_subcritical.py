"""GPU tests of nf_solve_subcritical / SolveSubcritical (fixed-source solve) against the EXACT solution of the same discrete system
(tests/subcrit_exact.py: one dense numpy solve), plus linearity, handle state, slab teams, the residual at size and the
not-subcritical / zero-source errors."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_inputs, make_hip, rel_l2, synthetic_inputs
from subcrit_exact import cell_measure, exact_subcritical, homogeneous_inputs, ref_from_inputs

pytestmark = pytest.mark.gpu

# test_heterogeneous_exact: tolerances of the solve, bars on the flux and on the integrals (tests/test_gpu_driver_forms.py imports them)
HET_TOL = (1e-12, 1e-11, 1e-11, 2000, 4000)
HET_FLUX_BAR, HET_SCALAR_BAR = 1e-8, 1e-9


def _solver(inp, rt=0, p=0, NSF=None, pushed=True):
    s = make_hip(dict(inp, NSF=inp["NSF"] if NSF is None else NSF), rt, p)
    if not pushed:
        s.solver_pushed = 0                                       # set_linear_solver never called: explicit-S (dense S^-1) branch
    return s


def _assert_matches(res, phi, ex, flux_tol, scalar_tol):
    assert rel_l2(phi, ex["phi"]) <= flux_tol, rel_l2(phi, ex["phi"])
    for key in ("M", "k_source", "phi_int", "phi_int_nofission", "production", "source"):
        assert abs(res[key] - ex[key]) <= scalar_tol * abs(ex[key]), (key, res[key], ex[key])


@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_homogeneous_medium_exact(dim, rt, ng):
    """uniform cross sections and source, every order and dimension: flux, M and k_source against the exact dense solve"""
    inp = homogeneous_inputs(dim, ng, n=(4, 3, 2))
    src = np.zeros((ng, inp["D"][0].size)); src[0] = 1.7
    ex = exact_subcritical(ref_from_inputs(inp, rt, rt), src)
    s = _solver(inp, rt, rt, pushed=False)
    s.set_tol(1e-14, 1e-13, 1e-13, 500, 1000)
    s.upload_source(src)
    res = s.solve_subcritical()
    _assert_matches(res, s.get_phi(), ex, 1e-11, 1e-11)
    assert res["n_outer_nofission"] <= 3 and s.info("last_path") == 0
    s.close()


def _iaea2d_subcritical():
    inp = load_inputs("iaea2d")
    s = _solver(inp)
    s.set_tol(1e-10, 1e-8, 1e-8, 1000, 2000)
    k, _ = s.solve_keff()
    s.close()
    nsf = inp["NSF"] * (0.85 / k)
    src = np.zeros(inp["D"].shape)
    ny, nx = src.shape[1:]
    iy, ix = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    src[0] = (1.0 + 0.5 * np.sin(0.3 * ix) * np.cos(0.2 * iy)) * (inp["NSF"][1] > 0)   # fuel only: reflector cells get none
    src[0][(ix // 2) % 3 == 1] = 0.0                                                    # and every third assembly column none
    return inp, nsf, src.reshape(2, -1)


def _synthetic_subcritical():
    inp = synthetic_inputs(8, 8, 4, 2, seed=4)
    s = _solver(inp, 1, 1)
    s.set_tol(1e-10, 1e-8, 1e-8, 1000, 2000)
    k, _ = s.solve_keff()
    s.close()
    src = np.zeros((2, 256)); src[0] = np.random.default_rng(7).uniform(0.5, 2.0, 256); src[0, ::5] = 0.0
    return inp, inp["NSF"] * (0.85 / k), src


@pytest.mark.parametrize("case,rt,route", [("iaea2d", 0, "direct"), ("iaea2d", 0, "cg"), ("iaea2d", 0, "diag"),
                                           ("synthetic", 1, "direct"), ("synthetic", 1, "cg")])
def test_heterogeneous_exact(case, rt, route):
    inp, nsf, src = _iaea2d_subcritical() if case == "iaea2d" else _synthetic_subcritical()
    s = _solver(inp, rt, rt, NSF=nsf, pushed=route == "cg")
    s.set_tol(*HET_TOL)
    s.upload_source(src)
    res = s.solve_subcritical(use_diag=route == "diag")
    r = ref_from_inputs(inp, rt, rt, NSF=nsf)
    ex = exact_subcritical(r, src, sinv=[s.diagonal_cache(g) for g in range(2)] if route == "diag" else None)
    _assert_matches(res, s.get_phi(), ex, HET_FLUX_BAR, HET_SCALAR_BAR)
    assert s.info("last_direct") == {"direct": 1, "cg": 0, "diag": s.info("last_direct")}[route]
    if route != "diag":                                           # the diagonal system has a k of its own
        assert abs(res["ratio"] - 0.85) <= 5e-3, res["ratio"]
    assert res["converged"] == 1 and s.progress() == res["n_outer"] + res["n_outer_nofission"]
    s.close()


def test_linearity_and_source_state():
    inp = synthetic_inputs(20, 16, 1, 2, seed=11)
    s = _solver(inp)
    s.set_tol(1e-10, 1e-8, 1e-8, 1000, 2000)
    k, _ = s.solve_keff()
    s.upload_xs(inp["D"], inp["SigR"], inp["NSF"] * (0.8 / k), inp["Chi"], inp["SigS"]); s.build()
    s.set_tol(1e-13, 1e-12, 1e-12, 2000, 4000)
    rng = np.random.default_rng(3)
    q1 = rng.uniform(0.0, 1.0, (2, 320)); q2 = np.zeros((2, 320)); q2[1, 100:140] = 3.0
    out = []
    for q in (q1, 2.0 * q1, q2, q1 + q2):
        s.upload_source(q)
        out.append((s.solve_subcritical(), s.get_phi().copy()))
    (r1, p1), (r2, p2), (_, pb), (_, pab) = out
    assert rel_l2(p2, 2.0 * p1) <= 1e-10 and abs(r2["M"] - r1["M"]) <= 1e-10 * r1["M"]
    assert rel_l2(pab, p1 + pb) <= 1e-9
    s.close()


def test_pybind_state_not_subcritical_and_zero_source():
    """IAEA-2D through the reference surface: SolveKeff on its golden k; the unmodified core is supercritical -> RuntimeError naming it,
    well before max_outer, GetLastKeff untouched, and SolveKeff still lands on the golden k; scaled to k = 0.85 the source solve runs, a
    source changed after BuildMatrices counts without a rebuild"""
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    inp = load_inputs("iaea2d")
    with open(os.path.join(GOLDEN, "golden_iaea2d.json")) as f:
        run = [r for r in json.load(f)["runs"] if r["tol"][0] == 1e-10 and not r["coarse"] and not r["diag"] and r["rt"] == 0][0]
    s = ns.NeutFEM(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    s.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        s.set_bc(int(a), ns.BCType(int(t)), 0.0)
    s.get_D()[...] = inp["D"]; s.get_SigR()[...] = inp["SigR"]; s.get_NSF()[...] = inp["NSF"]; s.get_Chi()[...] = inp["Chi"]; s.get_SigS()[...] = inp["SigS"]
    s.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    s.set_tol(*run["tol"][:3], 500, run["tol"][4])
    s.BuildMatrices()
    k1 = s.SolveKeff()
    assert abs(k1 - run["keff"]) <= 1e-8 * run["keff"]
    with pytest.raises(RuntimeError, match="subcritical"):          # zero source
        s.SolveSubcritical()
    s.get_SRC()[0] = 1.0
    with pytest.raises(RuntimeError, match="not subcritical"):
        s.SolveSubcritical()
    assert s.GetLastKeff() == k1
    assert abs(s.SolveKeff() - run["keff"]) <= 1e-8 * run["keff"]
    s.get_NSF()[...] = inp["NSF"] * (0.85 / k1)
    s.BuildMatrices()
    m1 = s.SolveSubcritical(); f1 = s.get_flux().copy()
    info = s.get_subcritical_info()
    assert info["M"] == m1 and info["converged"] == 1 and 1.0 < m1 and abs(info["ratio"] - 0.85) <= 5e-3
    s.get_SRC()[...] *= 2.0                                         # no BuildMatrices
    m2 = s.SolveSubcritical()
    assert abs(m2 - m1) <= 1e-10 * m1 and rel_l2(s.get_flux(), 2.0 * f1) <= 1e-10
    assert s.GetLastKeff() == k1


def test_not_subcritical_stops_early_and_handle_recovers():
    inp = load_inputs("iaea2d")
    s = _solver(inp)
    s.set_tol(1e-10, 1e-8, 1e-8, 500, 2000)
    s.upload_source(np.ones((2, inp["D"][0].size)))
    with pytest.raises(RuntimeError, match=r"error -6: .*not subcritical"):
        s.solve_subcritical()
    assert 5 <= s.progress() < 200
    s.upload_source(np.zeros((2, inp["D"][0].size)))
    with pytest.raises(RuntimeError, match=r"error -1: .*zero"):
        s.solve_subcritical()
    k, _ = s.solve_keff()
    t = _solver(inp); t.set_tol(1e-10, 1e-8, 1e-8, 500, 2000)
    k_ref, _ = t.solve_keff()
    assert abs(k - k_ref) <= 1e-8 * k_ref
    s.close(); t.close()


@pytest.mark.parametrize("single_reduce", [0, 1])
def test_slab_team_matches_undivided(single_reduce):
    from neutfem_amd.capi import HipTeam
    inp = synthetic_inputs(16, 16, 48, 2, seed=5)
    u = _solver(inp)
    u.set_tol(1e-10, 1e-8, 1e-8, 1000, 2000)
    k, _ = u.solve_keff()
    nsf = inp["NSF"] * (0.8 / k)
    u.upload_xs(inp["D"], inp["SigR"], nsf, inp["Chi"], inp["SigS"]); u.build()
    tol = (1e-11, 1e-10, 1e-10, 1000, 4000)
    src = np.zeros(inp["D"].shape); src[0, 10:30, 4:12, 3:9] = 1.0; src[1, 20:40] = 0.25
    u.set_tol(*tol); u.upload_source(src)
    ru = u.solve_subcritical(); pu = u.get_phi().reshape(2, 48, 16, 16)
    t = HipTeam(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], [(0, 16), (16, 32), (32, 48)])
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], nsf, inp["Chi"], inp["SigS"]); t.build()
    t.head.set_option("cg_single_reduce", single_reduce)
    t.set_tol(*tol); t.upload_source(src)
    rt = t.solve_subcritical()
    assert t.head.info("cg_reductions") == (1 if single_reduce else 2)
    assert rel_l2(t.get_phi_local(), pu) <= 1e-9 and abs(rt["M"] - ru["M"]) <= 1e-9 * ru["M"]
    assert rt["n_outer"] == ru["n_outer"] and rt["converged"] == ru["converged"] == 1
    t.close(); u.close()


def test_residual_at_size():
    """64^3, 2 groups, k scaled to 0.9: per group ||S_g phi_g - (chi_g tf + scatter_g + q_g)|| / ||q_g|| <= 1e-6, S_g applied on the device"""
    inp = synthetic_inputs(64, 64, 64, 2, seed=2)
    s = _solver(inp)
    s.set_tol(1e-8, 1e-6, 1e-6, 1000, 4000)
    k, _ = s.solve_keff()
    nsf = inp["NSF"] * (0.9 / k)
    s.upload_xs(inp["D"], inp["SigR"], nsf, inp["Chi"], inp["SigS"]); s.build()
    s.set_tol(1e-9, 1e-9, 1e-9, 2000, 4000)
    src = np.ones((2, 64 ** 3)); src[1] *= 0.1
    s.upload_source(src)
    res = s.solve_subcritical()
    assert res["converged"] == 1
    phi = s.get_phi()
    vol = np.einsum("k,j,i->kji", np.diff(inp["z_breaks"]), np.diff(inp["y_breaks"]), np.diff(inp["x_breaks"])).ravel()
    keep = lambda x: np.where(np.abs(x) > 1e-14, x, 0.0)
    tf = sum(keep(nsf[g].ravel()) * vol * phi[g] for g in range(2))
    for g in range(2):
        rhs = inp["Chi"][g].ravel() * tf + src[g] * vol
        for gp in range(2):
            if gp != g:
                rhs += keep(inp["SigS"][g, gp].ravel()) * vol * phi[gp]
        r = s.schur_apply(g, phi[g]) - rhs
        assert np.linalg.norm(r) / np.linalg.norm(src[g] * vol) <= 1e-6
    s.close()
