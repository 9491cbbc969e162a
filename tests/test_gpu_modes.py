"""GPU tests of nf_solve_modes / SolveModes (the leading lambda-modes by block power iteration) against the EXACT
eigenpairs of the same discrete system (tests/modes_exact.py: one dense numpy.linalg.eig), the two block kernels on their own against
extended-precision numpy, mode 0 against SolveKeff, the adjoint modes, handle state and the errors."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import load_inputs, make_hip, rel_l2, synthetic_inputs
from modes_exact import dense_operators, exact_modes, mode_residual
from subcrit_exact import homogeneous_inputs, ref_from_inputs

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _case(name, rt):
    inp = {"syn884": lambda: synthetic_inputs(8, 8, 4, 2, seed=4), "syn653": lambda: synthetic_inputs(6, 5, 3, 2, seed=4),
           "iaea2d": lambda: load_inputs("iaea2d")}[name]()
    return inp, ref_from_inputs(inp, rt, rt)


def _solver(inp, rt=0, pushed=True):
    s = make_hip(inp, rt, rt)
    if not pushed:
        s.solver_pushed = 0                                       # set_linear_solver never called: explicit-S (dense S^-1) branch
    return s


def _modes(s, res, adjoint=False):
    return [s.get_mode(i, adjoint).ravel() for i in range(res["n_modes"])]


# ---- 1. the block kernels alone ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blocks(n, b):
    rng = np.random.default_rng(1000 * b + n % 997)
    mk = lambda: rng.standard_normal((n, b)) * 10.0 ** rng.uniform(-6.0, 6.0, (n, b))     # entries over 12 decades
    return mk(), mk(), rng.standard_normal((b, b)), rng.standard_normal((b, b))


@pytest.fixture(scope="module")
def plain():
    s = make_hip(synthetic_inputs(4, 4, 1, 1, seed=0))
    yield s
    s.close()


@pytest.mark.parametrize("b", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_block_gram_per_entry(plain, n, b):
    """every entry of Q^T Z and Z^T Z within 1e-13 of its exact value (np.longdouble), relative to the sum of |q z| of its own terms"""
    Q, Z, _, _ = _blocks(n, b)
    H, G = plain.block_gram(Q, Z)
    Ql, Zl = Q.astype(LD), Z.astype(LD)
    for got, A in ((H, Ql), (G, Zl)):
        exact, scale = A.T @ Zl, np.abs(A).T @ np.abs(Zl)
        rho = np.abs(got.astype(LD) - exact) / scale
        print(n, b, "max rho", float(rho.max()))
        assert rho.max() <= 1e-13
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("full_m", [False, True])
@pytest.mark.parametrize("b", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_block_rotate_per_element(plain, n, b, full_m):
    """Q <- Z C element-wise within 8 b ulps of the magnitudes of its terms; the squared residual norms of Z_m - Q_m H (old Q) within
    1e-13 of the exact value relative to sum_e (|z| + sum_l |q_l H_lj|)^2 -- a sum over n like a Gram entry, held to the Gram's bound"""
    Q, Z, Cm, Hb = _blocks(n, b)
    m = b if full_m else 1
    Hm = Hb[:m, :m]
    out, res2 = plain.block_rotate(Q, Z, Cm, Hm)
    Ql, Zl = Q.astype(LD), Z.astype(LD)
    exact, scale = Zl @ Cm.astype(LD), np.abs(Zl) @ np.abs(Cm).astype(LD)
    err = np.abs(out.astype(LD) - exact) / scale
    print(n, b, m, "rotate ulps", float(err.max() / EPS))
    assert err.max() <= 8 * b * EPS
    R = Zl[:, :m] - Ql[:, :m] @ Hm.astype(LD)
    t = np.abs(Zl[:, :m]) + np.abs(Ql[:, :m]) @ np.abs(Hm).astype(LD)
    rho = np.abs(res2.astype(LD) - (R * R).sum(axis=0)) / (t * t).sum(axis=0)
    print(n, b, m, "res2 rho", float(rho.max()))
    assert rho.max() <= 1e-13


# ---- 2. homogeneous media at every order ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_homogeneous_medium_exact(dim, rt):
    inp = homogeneous_inputs(dim, 2, n=(4, 3, 2))
    r = ref_from_inputs(inp, rt, rt)
    m = 2 if dim == 1 else 3
    k_ex, _ = exact_modes(r, m)
    s = _solver(inp, rt, pushed=False)
    s.set_tol(1e-13, 1e-11, 1e-11, 500, 1000)
    res = s.solve_modes(m, n_guard=2)
    print(dim, rt, "outers", res["n_outer"], "k", res["k"], "exact", k_ex, "residual", res["residual"])
    assert res["converged"] == 1 and res["n_modes"] == m and res["n_block"] == m + 2
    for i, phi in enumerate(_modes(s, res)):
        assert abs(res["k"][i] - k_ex[i]) <= 1e-10 * k_ex[0], (i, res["k"][i], k_ex[i])
        rr = mode_residual(r, phi, res["k"][i])
        print("  mode", i, "exact residual", rr)
        assert rr <= 10 * 1e-11 and abs(np.linalg.norm(phi) - 1.0) <= 1e-13
    assert res["dominance_ratio"] == res["k"][1] / res["k"][0]
    s.close()


# ---- 3. mode 0 is SolveKeff ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iaea2d_modes():
    inp, _ = _case("iaea2d", 0)
    s = _solver(inp, 0, pushed=False)
    s.set_tol(1e-9, 1e-8, 1e-8, 2000, 1000)
    res = s.solve_modes(3, n_guard=3)
    modes = _modes(s, res)
    s.close()
    return res, modes


def _check_mode0(inp, rt, tol, res, phi0):
    t = _solver(inp, rt, pushed=False)
    t.set_tol(*tol)
    k, _ = t.solve_keff()
    flux = t.get_phi().ravel(); flux = flux / np.linalg.norm(flux)
    t.close()
    d = min(rel_l2(phi0, flux), rel_l2(-phi0, flux))
    print("k", res["k"][0], k, "flux distance", d)
    assert abs(res["k"][0] - k) <= 10 * tol[0] and d <= 100 * tol[1]


def test_mode0_is_solve_keff_homogeneous_3d_rt1():
    inp = homogeneous_inputs(3, 2, n=(4, 3, 2))
    tol = (1e-13, 1e-11, 1e-11, 500, 1000)
    s = _solver(inp, 1, pushed=False); s.set_tol(*tol)
    res = s.solve_modes(3, n_guard=2)
    _check_mode0(inp, 1, tol, res, s.get_mode(0).ravel())
    s.close()


def test_mode0_is_solve_keff_iaea2d(iaea2d_modes):
    res, modes = iaea2d_modes
    _check_mode0(_case("iaea2d", 0)[0], 0, (1e-9, 1e-8, 1e-8, 2000, 1000), res, modes[0])


# ---- 4. heterogeneous cores on the CG route ------------------------------------------------------------------------------------------
HET_TOL = (1e-11, 1e-10, 1e-10, 400, 2000)
HET_K_BAR, HET_RES_BAR = 1e-8, 100 * HET_TOL[1]                    # eigenvalues relative to k_0, exact residual of a mode (tests/test_gpu_driver_forms.py imports them)


@pytest.mark.parametrize("name,rt,route", [("syn884", 0, "cg"), ("syn653", 1, "cg"), ("syn884", 0, "diag")])
def test_heterogeneous_exact(name, rt, route):
    inp, r = _case(name, rt)
    s = _solver(inp, rt)
    s.set_tol(*HET_TOL)
    res = s.solve_modes(3, n_guard=2, use_diag=route == "diag")
    sinv = [s.diagonal_cache(g) for g in range(2)] if route == "diag" else None
    k_ex, _ = exact_modes(r, 3, sinv=sinv)
    print(name, rt, route, "outers", res["n_outer"], "cg", res["cg_total"], "k", res["k"], "exact", k_ex, "residual", res["residual"])
    assert res["converged"] == 1
    if route == "cg":                                             # the CG route really ran: more than one iteration per group solve
        assert res["cg_total"] > 2 * (res["n_outer"] * 5 + 3) * 2
    for i, phi in enumerate(_modes(s, res)):
        assert abs(res["k"][i] - k_ex[i]) <= HET_K_BAR * k_ex[0], (i, res["k"][i], k_ex[i])
        rr = mode_residual(r, phi, res["k"][i], sinv=sinv)
        print("  mode", i, "exact residual", rr)
        assert rr <= HET_RES_BAR
    s.close()


# ---- 5. the degenerate pair of IAEA-2D -----------------------------------------------------------------------------------------------
def test_iaea2d_degenerate_pair(iaea2d_modes):
    res, modes = iaea2d_modes
    inp, r = _case("iaea2d", 0)
    k_ex, _ = exact_modes(r, 4)
    print("outers", res["n_outer"], "k", res["k"], "exact", k_ex, "residual", res["residual"])
    assert np.abs(k_ex[:3] - [1.02898628, 1.01548626, 1.01548626]).max() <= 1e-8      # the yardstick reproduces the quoted spectrum
    assert res["converged"] == 1
    for i in range(3):
        assert abs(res["k"][i] - k_ex[i]) <= 1e-8
        rr = mode_residual(r, modes[i], res["k"][i])
        print("  mode", i, "exact residual", rr)
        assert rr <= 1e-7
    assert abs(res["k"][1] - res["k"][2]) <= 1e-8
    assert res["dominance_ratio"] == res["k"][1] / res["k"][0]


# ---- 6. adjoint ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_modes():
    inp, r = _case("syn884", 0)
    s = _solver(inp, 0)
    s.set_tol(*HET_TOL)
    rd = s.solve_modes(3, n_guard=2)
    ra = s.solve_modes(3, n_guard=2, adjoint=True)
    phi, adj = _modes(s, rd), _modes(s, ra, adjoint=True)
    assert ra["converged"] == 1
    assert all(np.array_equal(a, b) for a, b in zip(phi, _modes(s, rd)))      # the direct modes stay beside the adjoint ones
    _, F = dense_operators(r)
    print("direct", rd["k"], "adjoint", ra["k"], "outers", rd["n_outer"], ra["n_outer"])
    for i in range(3):
        assert abs(ra["k"][i] - rd["k"][i]) <= HET_K_BAR * rd["k"][0]
        rr = mode_residual(r, adj[i], ra["k"][i], adjoint=True)
        print("  adjoint mode", i, "exact residual", rr)
        assert rr <= HET_RES_BAR
    B = np.array([[a @ (F @ p) for p in phi] for a in adj])
    for i in range(3):
        for j in range(3):
            if i != j:
                assert abs(B[i, j]) <= 1e-6 * np.sqrt(abs(B[i, i]) * abs(B[j, j])), (i, j, B)
    s.close()


# ---- 7. state and errors -------------------------------------------------------------------------------------------------------------
def _warm(s):
    v, k = C.c_int(), C.c_double()
    s._chk(s.L.nf_get_warm_state(s.h, C.byref(v), C.byref(k)))
    return v.value, k.value


def test_handle_state_is_untouched():
    inp = synthetic_inputs(12, 10, 1, 2, seed=3)
    s = _solver(inp); s.set_tol(1e-10, 1e-8, 1e-8, 500, 1000)
    k0, n0 = s.solve_keff()
    s.solve_adjoint()
    before = (s.get_phi().copy(), s.get_phi_adj().copy(), s.history(), _warm(s), s.progress(), s.info("last_outer"))
    res = s.solve_modes(2)
    assert res["converged"] == 1 and abs(res["k"][0] - k0) <= 1e-8
    after = (s.get_phi(), s.get_phi_adj(), s.history(), _warm(s), s.progress(), s.info("last_outer"))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for key in ("k", "dk", "dphi", "cg"):
        assert np.array_equal(before[2][key], after[2][key])
    assert before[3:] == after[3:]
    s.reset_flux(); s.set_warm_state(0, 1.0)
    k1, n1 = s.solve_keff()
    assert k1 == k0 and n1 == n0                                  # a following solve_keff reproduces what it gave before
    s.close()


def test_argument_and_state_errors():
    inp = synthetic_inputs(12, 10, 1, 2, seed=3)
    s = _solver(inp); s.set_tol(1e-10, 1e-8, 1e-8, 500, 1000)
    with pytest.raises(RuntimeError, match="error -5"):
        s.get_mode(0)
    for kw in (dict(n_modes=0), dict(n_modes=7, n_guard=2), dict(n_modes=2, use_cmfd=True), dict(n_modes=2, use_coarse=True, factors=(2, 2))):
        with pytest.raises(RuntimeError, match="error -1"):
            s.solve_modes(**kw)
    s.solve_modes(2)
    with pytest.raises(RuntimeError, match="error -5"):
        s.get_mode(0, adjoint=True)                               # no adjoint solve yet
    with pytest.raises(RuntimeError, match="error -1"):
        s.get_mode(2)
    assert np.isfinite(s.get_mode(1)).all()
    s.build()
    with pytest.raises(RuntimeError, match="error -5"):
        s.get_mode(0)                                             # nf_build drops the modes
    s.close()


def test_upscatter_and_slab_teams_are_refused():
    from neutfem_amd.capi import HipTeam
    inp = synthetic_inputs(12, 10, 1, 2, seed=3)
    up = dict(inp, SigS=inp["SigS"].copy()); up["SigS"][0, 1] = 0.002
    s = _solver(up)
    with pytest.raises(RuntimeError, match="error -4: .*upscatter"):
        s.solve_modes(2)
    s.close()
    i3 = synthetic_inputs(4, 4, 8, 2, seed=1)
    t = HipTeam(0, 0, 2, i3["x_breaks"], i3["y_breaks"], i3["z_breaks"], [(0, 4), (4, 8)])
    with pytest.raises(RuntimeError, match="error -4: .*undivided"):
        t.head.solve_modes(2)
    t.close()


def test_max_outer_and_single_vector_block():
    inp = synthetic_inputs(12, 10, 1, 2, seed=3)
    s = _solver(inp); s.set_tol(1e-12, 1e-11, 1e-11, 3, 1000)
    res = s.solve_modes(2)
    assert res["converged"] == 0 and res["n_outer"] == 3 and np.isfinite(res["k"]).all() and np.isfinite(res["residual"]).all()
    s.set_tol(1e-10, 1e-8, 1e-8, 2000, 1000)
    res = s.solve_modes(1, n_guard=0)                             # b = 1 through both kernels: the plain power iteration
    k, _ = s.solve_keff()
    print("b = 1: outers", res["n_outer"], "k", res["k"], k)
    assert res["converged"] == 1 and res["n_block"] == 1 and res["dominance_ratio"] == 0.0 and abs(res["k"][0] - k) <= 1e-8
    s.close()


# ---- 8. pybind surface ---------------------------------------------------------------------------------------------------------------
def test_pybind_surface_matches_ctypes():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    inp = synthetic_inputs(12, 10, 1, 2, seed=3)
    tol = (1e-10, 1e-8, 1e-8, 500, 1000)
    p = ns.NeutFEM(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    p.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        p.set_bc(int(a), ns.BCType(int(t)), 0.0)
    p.get_D()[...] = inp["D"]; p.get_SigR()[...] = inp["SigR"]; p.get_NSF()[...] = inp["NSF"]; p.get_Chi()[...] = inp["Chi"]; p.get_SigS()[...] = inp["SigS"]
    p.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    p.set_tol(*tol)
    with pytest.raises(RuntimeError):
        p.get_modes_info()
    p.BuildMatrices()
    ks = p.SolveModes(2)
    s = _solver(inp); s.set_tol(*tol)
    res = s.solve_modes(2)
    info = p.get_modes_info()
    assert ks == res["k"] == info["k"] and info["residual"] == res["residual"] and info["n_outer"] == res["n_outer"]
    assert info["converged"] == 1 and info["n_block"] == 4 and info["adjoint"] is False and info["dominance_ratio"] == res["dominance_ratio"]
    m1 = p.get_mode(1)
    assert m1.shape == p.get_flux().shape and np.array_equal(m1.ravel(), s.get_mode(1).ravel())
    assert p.GetLastKeff() == 1.0                                 # SolveModes leaves the warm state alone
    s.close()
