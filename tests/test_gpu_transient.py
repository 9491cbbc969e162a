"""GPU tests of nf_transient_begin / nf_transient_step (space-time kinetics with delayed-neutron precursors) against the
EXACT implicit-Euler stepper of the same discrete system (tests/transient_exact.py: one dense solve per step), plus the rebalance, the
null transient, handle state, errors and the pybind surface."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import load_inputs, make_hip, rel_l2, synthetic_inputs
from subcrit_exact import homogeneous_inputs, ref_from_inputs
from transient_exact import SIX_BETA, SIX_LAMBDA, TWO_GROUP_V, ExactTransient, fundamental_mode, homogeneous_recurrence, mass_weights

pytestmark = pytest.mark.gpu

KEFF_TOL = (1e-10, 1e-8, 1e-8, 1000, 2000)                       # the k-eff solves behind the heterogeneous cases (_synthetic_subcritical's)
EXACT_TOL = (1e-12, 1e-11, 1e-11, 2000, 4000)
EXACT_FLUX_BAR, EXACT_SCALAR_BAR = 1e-8, 1e-9                      # flux and precursors, scalars and power of a step at EXACT_TOL (tests/test_gpu_driver_forms.py imports them)
SCALARS = ("time", "power", "production", "phi_int", "precursors")


def _solver(inp, rt=0, p=0, pushed=True):
    s = make_hip(inp, rt, p)
    if not pushed:
        s.solver_pushed = 0                                       # set_linear_solver never called: explicit-S (dense S^-1) branch
    return s


def _rebuild(s, inp):
    s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); s.build()


def _assert_step(s, res, st, flux_tol, scalar_tol):
    """flux, every precursor family and the scalars of the handle after a step against the yardstick's step `st`"""
    assert rel_l2(s.get_phi(), st["phi"]) <= flux_tol, rel_l2(s.get_phi(), st["phi"])
    for i in range(st["c"].shape[0]):
        assert rel_l2(s.get_precursors(i), st["c"][i]) <= flux_tol, (i, rel_l2(s.get_precursors(i), st["c"][i]))
    for key in SCALARS:
        assert abs(res[key] - st[key]) <= scalar_tol * abs(st[key]), (key, res[key], st[key])


def _scaled_sigr(inp, g, factor):
    sig = np.array(inp["SigR"], dtype=np.float64)
    flat = sig[g].reshape(-1); flat[:16] *= factor               # the first 16 cells of group g
    return sig


def _scenario(s, ex, inp, g):
    """the perturbation sequence of the heterogeneous cases on handle and yardstick alike: SigR of group g x 0.97 in the first 16 cells,
    3 steps of 1e-2, then x 1.05 on the same cells, 2 steps of 1e-3; every step compared.  Returns (results, outers of the calls)"""
    out, outers = [], []
    cur = dict(inp)
    for factor, dt, n in ((0.97, 1e-2, 3), (1.05, 1e-3, 2)):
        cur = dict(cur, SigR=_scaled_sigr(cur, g, factor))
        _rebuild(s, cur); ex.set_xs(SigR=cur["SigR"])
        for st in ex.step(dt, n):                                 # one step per call: every step's flux is compared
            res, power = s.transient_step(dt, 1)
            _assert_step(s, res, st, EXACT_FLUX_BAR, EXACT_SCALAR_BAR)
            assert abs(power[0] - st["power"]) <= EXACT_SCALAR_BAR * st["power"] and s.progress() == res["n_outer"]
            out.append(res); outers.append(res["n_outer"])
    return out, outers


# ---- 1. homogeneous medium: every order and dimension on the dense route ---------------------------------------------------------------
@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_homogeneous_closed_form(dim, rt, ng):
    eps, dt, beta, lam = 0.004, 0.02, 0.0065, 0.08
    v = (3e5,) if ng == 1 else (1e7, 3e5)
    inp = homogeneous_inputs(dim, ng, n=(4, 3, 2))
    r = ref_from_inputs(inp, rt, rt)
    k0, phi0 = fundamental_mode(r)
    ex = ExactTransient(inp, rt, rt, v, [beta], [lam], k0, phi0)
    s = _solver(inp, rt, rt, pushed=False)
    s.set_tol(1e-14, 1e-13, 1e-13, 500, 1000)
    s.set_phi(phi0); s.transient_begin(v, [beta], [lam], k0)
    up = dict(inp, NSF=inp["NSF"] * (1.0 + eps))
    _rebuild(s, up); ex.set_xs(NSF=up["NSF"])
    rec = homogeneous_recurrence(float(inp["NSF"].ravel()[0]) / k0, eps, v[0], dt, beta, lam, 4)
    W = mass_weights(r)
    for st, (amp, gam) in zip(ex.step(dt, 4), rec):
        res, power = s.transient_step(dt, 1)
        _assert_step(s, res, st, 1e-11, 1e-11)
        assert abs(power[0] - st["power"]) <= 1e-11 * st["power"]
        if ng == 1:                                               # the scalar recurrence
            assert rel_l2(s.get_phi(), amp * phi0) <= 1e-11 and rel_l2(s.get_precursors(0), gam * W * phi0[0]) <= 1e-11
            assert abs(power[0] - amp * (1.0 + eps)) <= 1e-11 * amp
    assert s.info("last_direct") == 1 and s.info("transient_steps") == 4 and s.info("transient_rebuilds") == 1
    s.close()


# ---- 2. heterogeneous, exact ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _critical_state(case):
    """(inputs, rt, k, phi) of a converged k-eff solve: the start of the heterogeneous cases, solved once"""
    inp, rt = (load_inputs("iaea2d"), 0) if case == "iaea2d" else (synthetic_inputs(8, 8, 4, 2, seed=4), 1)
    s = _solver(inp, rt, rt)
    s.set_tol(*KEFF_TOL)
    k, _ = s.solve_keff()
    phi = s.get_phi().copy()
    s.close()
    return inp, rt, k, phi


@functools.lru_cache(maxsize=None)
def _reference_scenario(case):
    """the yardstick's five steps of _scenario, computed once per case and left unchanged"""
    inp, rt, k, phi = _critical_state(case)
    ex = ExactTransient(inp, rt, rt, TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, phi, chi_delayed=(1.0, 0.0))
    steps, cur = [], dict(inp)
    for factor, dt, n in ((0.97, 1e-2, 3), (1.05, 1e-3, 2)):
        cur = dict(cur, SigR=_scaled_sigr(cur, 1, factor))
        ex.set_xs(SigR=cur["SigR"])
        steps += ex.step(dt, n)
    return steps


class _Replay:
    """an ExactTransient stand-in that replays recorded steps (the shared reference of the two routes)"""

    def __init__(self, steps): self.steps, self.at = steps, 0
    def set_xs(self, **xs): pass

    def step(self, dt, n):
        out = self.steps[self.at:self.at + n]; self.at += n
        return out


@pytest.mark.parametrize("case,route", [("iaea2d", "direct"), ("iaea2d", "cg"), ("synthetic", "direct"), ("synthetic", "cg")])
def test_heterogeneous_exact(case, route):
    inp, rt, k, phi = _critical_state(case)
    s = _solver(inp, rt, rt, pushed=route == "cg")
    s.set_tol(*EXACT_TOL)
    s.set_phi(phi); s.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, chi_delayed=(1.0, 0.0))
    xcd0 = s.info("xcd_solves")
    results, _ = _scenario(s, _Replay(_reference_scenario(case)), inp, 1)
    assert all(r["n_unconverged"] == 0 for r in results) and results[-1]["n_steps"] == 5
    assert s.info("transient_rebuilds") == 2 and s.info("transient_steps") == 5
    assert s.info("last_direct") == (1 if route == "direct" else 0)
    if case == "synthetic" and route == "cg":                     # 2048 unknowns per group: the one-XCD CG engages
        assert s.info("xcd_solves") > xcd0
    s.close()


# ---- 3. the rebalance is engaged -----------------------------------------------------------------------------------------------------------
def test_rebalance_bounds_the_outers():
    """first step of the synthetic case (8 x 8 x 4, RT1-P1) at tol_flux 1e-10: at most 100 outers with the rebalance (plain source iteration
    contracts like 1 - beta: 800 outers or more).  tol_keff is set to tol_flux: P is a linear functional of the flux, so a tighter tol_keff
    would ask for more than the flux tolerance this test is about.  The scalar rebalance removes the fundamental mode; what is left decays
    at the core's dominance ratio (0.86 here), so the count is that of 1e-10 at 0.855 per outer: 89 measured (118 down to tol_keff 1e-12)"""
    inp, rt, k, phi = _critical_state("synthetic")
    s = _solver(inp, rt, rt)
    s.set_tol(1e-10, 1e-10, 1e-10, 2000, 4000)
    s.set_phi(phi); s.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, chi_delayed=(1.0, 0.0))
    _rebuild(s, dict(inp, SigR=_scaled_sigr(inp, 1, 0.97)))
    res, _ = s.transient_step(1e-2, 1)
    print("outers of the step with the rebalance:", res["n_outer_max"], "f =", res["rebalance"])
    assert res["n_outer_max"] <= 100 and res["n_unconverged"] == 0
    s.close()


def test_plain_iteration_lands_on_the_same_step():
    """option transient_rebalance = 0 on the (4, 3, 2) RT1 mesh: slow, but the same fixed point.  The plain iteration contracts like
    (1 - a)(1 + eps) = 0.9945 per outer and stops once its own change is below tol_flux, that is 1 / (1 - 0.9945) = 180 x tol_flux above the
    exact step: about 2e-8 at tol 1e-10 (the 1e-7 bar), after some 2800 of the 5000 outers allowed"""
    eps = 0.001
    inp = homogeneous_inputs(3, 2, n=(4, 3, 2))
    inp["SigR"][1][0, 0, :2] *= 1.3                               # not homogeneous any more: the flux shape moves too
    r = ref_from_inputs(inp, 1, 1)
    k0, phi0 = fundamental_mode(r)
    v, beta, lam = (1e7, 3e5), [0.0065], [0.08]
    ex = ExactTransient(inp, 1, 1, v, beta, lam, k0, phi0)
    up = dict(inp, NSF=inp["NSF"] * (1.0 + eps)); ex.set_xs(NSF=up["NSF"])
    st = ex.step(0.02, 1)[0]
    s = _solver(inp, 1, 1, pushed=False)
    s.set_tol(1e-10, 1e-10, 1e-10, 5000, 4000)
    s.set_option("transient_rebalance", 0)
    s.set_phi(phi0); s.transient_begin(v, beta, lam, k0)
    _rebuild(s, up)
    res, _ = s.transient_step(0.02, 1)
    print("outers of the step without the rebalance:", res["n_outer"])
    assert res["rebalance"] == 1.0 and res["n_unconverged"] == 0 and res["n_outer"] > 1000
    _assert_step(s, res, st, 1e-7, 1e-7)
    s.close()


# ---- 4. null transient -------------------------------------------------------------------------------------------------------------------------
def test_null_transient_is_stationary():
    inp = load_inputs("iaea2d")
    tol_flux = 1e-10
    s = _solver(inp)
    s.set_tol(1e-12, tol_flux, tol_flux, 2000, 4000)
    k, _ = s.solve_keff()
    phi0 = s.get_phi().copy()
    bar = 100.0 * tol_flux
    s.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k)
    vol = np.einsum("j,i->ji", np.diff(inp["y_breaks"]), np.diff(inp["x_breaks"])).ravel()
    tf = sum(np.where(np.abs(inp["NSF"][g].ravel()) > 1e-14, inp["NSF"][g].ravel(), 0.0) * vol * phi0[g] for g in range(2))
    for i in range(6):                                            # equilibrium precursors at begin
        assert rel_l2(s.get_precursors(i), SIX_BETA[i] * tf / (SIX_LAMBDA[i] * k)) <= 1e-13
    s.set_tol(1e-13, 1e-12, 1e-12, 2000, 4000)
    res, power = s.transient_step(0.1, 5)
    assert np.abs(power - 1.0).max() <= bar, power
    phi = s.get_phi()
    assert rel_l2(phi / np.linalg.norm(phi), phi0 / np.linalg.norm(phi0)) <= bar
    for i in range(6):
        assert rel_l2(s.get_precursors(i), SIX_BETA[i] * tf / (SIX_LAMBDA[i] * k)) <= bar
    assert abs(res["time"] - 0.5) <= 1e-15 and res["n_steps"] == 5 and res["n_unconverged"] == 0
    s.close()


# ---- 5. three groups with upscatter, the family loop bounds, more than one block ------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,nfam", [(16, 12, 1), (20, 16, 0), (20, 16, 1), (20, 16, 8)])
def test_three_groups_upscatter_and_family_bounds(nx, ny, nfam):
    inp = synthetic_inputs(nx, ny, 1, 3, seed=6)
    inp["SigS"][0, 2] = 0.002 * (inp["NSF"][0] > 0)               # a second upscatter block, 3 -> 1
    beta = (SIX_BETA + (1e-4, 3e-4))[:nfam] if nfam != 1 else (0.0065,)
    lam = (SIX_LAMBDA + (5.0, 0.05))[:nfam] if nfam != 1 else (0.08,)
    v, chid = (1e7, 1e6, 2.2e5), (1.0, 0.0, 0.0)
    s = _solver(inp)
    s.set_tol(*KEFF_TOL)
    k, _ = s.solve_keff()
    phi = s.get_phi().copy()
    ex = ExactTransient(inp, 0, 0, v, beta, lam, k, phi, chi_delayed=chid)
    s.set_tol(*EXACT_TOL)
    s.transient_begin(v, beta, lam, k, chi_delayed=chid)
    results, _ = _scenario(s, ex, inp, 2)
    assert all(r["n_unconverged"] == 0 for r in results) and s.info("transient_rebuilds") == 2
    if nfam == 0:
        assert results[-1]["precursors"] == 0.0
        with pytest.raises(RuntimeError, match="error -1: "):
            s.get_precursors(0)
    s.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------------
def _warm_state(s):
    v, k = C.c_int(), C.c_double()
    s._chk(s.L.nf_get_warm_state(s.h, C.byref(v), C.byref(k)))
    return v.value, k.value


def test_state_survives_other_solves_and_restarts():
    inp = synthetic_inputs(20, 16, 1, 2, seed=11)
    probe = _solver(inp); probe.set_tol(*KEFF_TOL)
    k_raw, _ = probe.solve_keff(); probe.close()
    inp = dict(inp, NSF=inp["NSF"] * (0.9 / k_raw))               # k = 0.9: the handle's own system is subcritical, SolveSubcritical runs on it
    up = dict(inp, SigR=_scaled_sigr(inp, 1, 0.97))
    src = np.ones((2, 320))

    def run(interrupt):
        s = _solver(inp); s.set_tol(*KEFF_TOL)
        k, _ = s.solve_keff()
        phi = s.get_phi().copy()
        s.set_tol(*EXACT_TOL)
        s.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, chi_delayed=(1.0, 0.0))
        _rebuild(s, up)
        r1, p1 = s.transient_step(1e-2, 2)
        mid = (s.history(), _warm_state(s))
        if interrupt:
            s.set_tol(*KEFF_TOL); s.solve_keff(); s.upload_source(src); s.solve_subcritical(); s.set_tol(*EXACT_TOL)
            assert rel_l2(s.get_phi(), phi) > 1e-3                # the handle's current flux is the other solve's now
        r2, p2 = s.transient_step(1e-2, 2)
        return s, k, phi, (r1, r2), np.concatenate([p1, p2]), mid

    a, k, phi, ra, pa, mid_a = run(False)
    # stepping leaves the warm k-eff state and the history alone
    h, w = a.history(), _warm_state(a)
    assert w == mid_a[1] == (1, k) and h["n_outer"] == mid_a[0]["n_outer"] and np.array_equal(h["k"], mid_a[0]["k"])
    b, _, _, rb, pb, _ = run(True)
    assert np.array_equal(pa, pb) and ra[1] == rb[1]              # bit-identical to the uninterrupted run
    assert np.array_equal(a.get_phi(), b.get_phi()) and np.array_equal(a.get_precursors(3), b.get_precursors(3))
    c, _, _, rc, pc, _ = run(False)                               # determinism
    assert np.array_equal(pa, pc) and ra == rc
    c.close(); b.close()
    # get_phi() after the steps is the yardstick's flux
    ex = ExactTransient(inp, 0, 0, TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, phi, chi_delayed=(1.0, 0.0))
    ex.set_xs(SigR=up["SigR"])
    st = ex.step(1e-2, 4)
    _assert_step(a, ra[1], st[-1], EXACT_FLUX_BAR, EXACT_SCALAR_BAR)
    assert ra[1]["n_steps"] == 4 and abs(ra[1]["time"] - 0.04) <= 1e-15
    # a second begin restarts at t = 0 from the current flux
    a.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, chi_delayed=(1.0, 0.0))
    assert a.info("transient_steps") == 0 and a.info("transient_rebuilds") == 0
    r, _ = a.transient_step(1e-2, 1)
    assert r["n_steps"] == 1 and abs(r["time"] - 1e-2) <= 1e-15
    a.transient_end()
    with pytest.raises(RuntimeError, match="error -5: .*nf_transient_begin"):
        a.transient_step(1e-2, 1)
    with pytest.raises(RuntimeError, match="error -5: "):
        a.get_precursors(0)
    a.transient_end()                                             # NF_OK without one
    a.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    from neutfem_amd.capi import HipSolver
    inp = homogeneous_inputs(2, 2, n=(4, 3, 2))
    s = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    v, b, l = (1e7, 3e5), [0.0065], [0.08]
    with pytest.raises(RuntimeError, match="error -5: "):         # not built
        s.transient_begin(v, b, l, 1.0)
    s.close()
    s = _solver(inp, pushed=False)
    with pytest.raises(RuntimeError, match="error -5: "):         # no begin
        s.transient_step(1e-2, 1)
    bad = [dict(velocity=(1e7, 0.0)), dict(velocity=(1e7, -1.0)), dict(velocity=(np.inf, 3e5)), dict(lam=[0.0]), dict(lam=[-0.1]), dict(beta=[-1e-3]),
           dict(beta=[0.6, 0.4], lam=[0.08, 0.1]), dict(beta=[np.nan]), dict(lam=[np.inf]), dict(keff=0.0), dict(keff=-1.0), dict(keff=np.nan),
           dict(chi_delayed=(np.nan, 0.0)), dict(beta=[1e-4] * 9, lam=[0.1] * 9)]
    for kw in bad:
        args = dict(velocity=v, beta=b, lam=l, keff=1.0); args.update(kw)
        with pytest.raises(RuntimeError, match="error -1: "):
            s.transient_begin(**args)
    s.set_phi(np.zeros((2, s.n_phi)))                             # P(0) = 0
    with pytest.raises(RuntimeError, match="error -1: .*P\\(0\\)"):
        s.transient_begin(v, b, l, 1.0)
    s.reset_flux()
    s.transient_begin(v, [], [], 1.0)                             # prompt neutrons only is valid
    for dt, n in ((0.0, 1), (-1.0, 1), (np.nan, 1), (np.inf, 1), (1e-2, 0)):
        with pytest.raises(RuntimeError, match="error -1: "):
            s.transient_step(dt, n)
    for kw in (dict(use_coarse=True, factors=(2, 1)), dict(use_cmfd=True), dict(use_diag=True)):
        o = s.opts(**kw)
        assert s.L.nf_transient_step(s.h, C.byref(o), 1e-2, 1, None, None) == -1
    s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    with pytest.raises(RuntimeError, match="error -5: .*nf_build"):   # uploaded, not built again
        s.transient_step(1e-2, 1)
    s.close()


def test_slab_team_is_unsupported():
    from neutfem_amd.capi import HipTeam
    inp = synthetic_inputs(8, 8, 12, 2, seed=5)
    t = HipTeam(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], [(0, 6), (6, 12)])
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); t.build()
    with pytest.raises(RuntimeError, match="error -4: "):
        t.head.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, 1.0)
    with pytest.raises(RuntimeError, match="error -4: "):
        t.head.transient_step(1e-2, 1)
    t.close()


def test_non_finite_step_keeps_the_last_completed_state():
    """dt = 1e-320 makes 1 / (v dt) overflow: the dense step of the yardstick is non-finite, the GPU step returns NF_ERR_NUMERIC and time,
    flux and precursors stay those of the last completed step; the following valid step matches the yardstick"""
    inp = homogeneous_inputs(2, 2, n=(4, 3, 2))
    inp["SigR"][1][0, :2] *= 1.3
    r = ref_from_inputs(inp, 1, 1)
    k0, phi0 = fundamental_mode(r)
    v, beta, lam = (1e7, 3e5), [0.0065], [0.08]
    ex = ExactTransient(inp, 1, 1, v, beta, lam, k0, phi0)
    up = dict(inp, NSF=inp["NSF"] * 1.004); ex.set_xs(NSF=up["NSF"])
    first = ex.step(0.02, 1)[0]
    with np.errstate(all="ignore"), pytest.raises(FloatingPointError):
        ex.step(1e-320, 1)                                        # the chosen input really is non-finite in the dense step
    ex._op = None
    s = _solver(inp, 1, 1, pushed=False)
    s.set_tol(1e-13, 1e-12, 1e-12, 500, 1000)
    s.set_phi(phi0); s.transient_begin(v, beta, lam, k0)
    _rebuild(s, up)
    res, _ = s.transient_step(0.02, 1)
    _assert_step(s, res, first, 1e-9, 1e-9)
    phi1, c1 = s.get_phi().copy(), s.get_precursors(0).copy()
    from neutfem_amd.capi import TransientResult
    o, bad = s.opts(), TransientResult()
    assert s.L.nf_transient_step(s.h, C.byref(o), 1e-320, 1, None, C.byref(bad)) == -6
    assert bad.time == res["time"] and bad.n_steps == 1 and bad.production == res["production"] and bad.precursors == res["precursors"]
    assert np.array_equal(s.get_phi(), phi1) and np.array_equal(s.get_precursors(0), c1) and s.info("transient_steps") == 1
    res2, _ = s.transient_step(0.02, 1)                           # the handle stays usable
    _assert_step(s, res2, ex.step(0.02, 1)[0], 1e-9, 1e-9)
    s.close()


# ---- 8. pybind -----------------------------------------------------------------------------------------------------------------------------------
def test_pybind_matches_the_c_abi():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    inp = load_inputs("iaea2d")
    tol = (1e-10, 1e-9, 1e-9, 1000, 2000)
    p = ns.NeutFEM(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    p.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        p.set_bc(int(a), ns.BCType(int(t)), 0.0)
    p.get_D()[...] = inp["D"]; p.get_SigR()[...] = inp["SigR"]; p.get_NSF()[...] = inp["NSF"]; p.get_Chi()[...] = inp["Chi"]; p.get_SigS()[...] = inp["SigS"]
    p.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    p.set_tol(*tol)
    p.BuildMatrices()
    k = p.SolveKeff()
    phi0 = np.array(p.get_flux()).reshape(2, -1)
    with pytest.raises(RuntimeError, match="begin_transient"):
        p.get_transient_info()
    p.begin_transient(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, chi_delayed=(1.0, 0.0))      # keff = GetLastKeff()
    p.get_SigR()[1].reshape(-1)[:16] *= 0.97
    p.BuildMatrices()
    power = p.step_transient(1e-2, 3)
    info = p.get_transient_info()
    assert power.shape == (3,) and info["n_steps"] == 3 and info["power"] == power[-1] and abs(info["time"] - 0.03) <= 1e-15
    assert p.get_precursors(2).shape == p.get_flux().shape[1:]
    assert p.GetLastKeff() == k
    s = _solver(inp); s.set_tol(*tol)
    s.set_phi(phi0); s.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, chi_delayed=(1.0, 0.0))
    _rebuild(s, dict(inp, SigR=_scaled_sigr(inp, 1, 0.97)))
    res, ref = s.transient_step(1e-2, 3)
    assert np.abs(power - ref).max() <= 1e-12 * np.abs(ref).max()
    assert rel_l2(np.array(p.get_flux()).ravel(), s.get_phi().ravel()) <= 1e-12      # get_flux() holds the flux at time t
    assert rel_l2(np.array(p.get_precursors(2)).ravel(), s.get_precursors(2)) <= 1e-12
    s.close()
