"""GPU tests of nf_kinetics_params / nf_transient_kinetics (adjoint-weighted kinetics parameters and dynamic reactivity)
against the numpy twin of tests/kinetics_exact.py: the forms on injected fields, the grid-stride wrap, the static reactivity end to end,
the discrete point-kinetics balance of every step of a transient, the state of the handle, the errors and the pybind surface."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from helpers import load_inputs, make_hip, synthetic_inputs
from kinetics_exact import RAW, balance_residual, dense_operators, derived, kinetics_forms
from subcrit_exact import homogeneous_inputs, ref_from_inputs
from test_gpu_transient import (EXACT_FLUX_BAR, EXACT_SCALAR_BAR, EXACT_TOL, KEFF_TOL, _critical_state, _rebuild, _reference_scenario,
                                _scaled_sigr, _solver)
from transient_exact import SIX_BETA, SIX_LAMBDA, TWO_GROUP_V, ExactTransient
from zoom_exact import _mass, fission_matrix, ref_unbuilt

pytestmark = pytest.mark.gpu

KEFF = 0.9
THREE_GROUP_V = (1e7, 1e6, 2.2e5)
FORM_BAR = 1e-13          # a raw form against the twin, times the sum of the absolute values of its terms: sums of <= 1e6 products in two orders
APPLY_BAR = 1e-12         # the bar of the apply tests on y = S_g phi_g, carried through the dot: APPLY_BAR max|y| ||w||_1
TIGHT = (1e-12, 1e-11, 1e-11, 2000, 4000)
ORDERS = [(dim, rt, rt) for dim in (1, 2, 3) for rt in (0, 1, 2)] + [(2, 1, 0), (2, 2, 1)]   # the grid of test_gpu_sensitivity.py


def _trim(dim, n=(9, 7, 5)):
    return n[0], n[1] if dim >= 2 else 1, n[2] if dim == 3 else 1


def _ulps(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(max(abs(a), abs(b)))


def _bars(tw, w):
    """absolute bar of every raw form of the twin result `tw` (c_amp: a list)"""
    sc = tw["scale"]
    bars = {k: FORM_BAR * sc[k] for k in RAW}
    bars["removal_leakage"] += APPLY_BAR * float(np.abs(tw["y"]).max()) * float(np.abs(w).sum())
    bars["c_amp"] = [FORM_BAR * s for s in sc["c_amp"]]
    return bars


def _assert_raw(res, tw, w, label):
    bars = _bars(tw, w)
    for k in RAW:
        print(f"kin {label}: {k} gpu={res[k]:.15e} twin={tw[k]:.15e} |d|={abs(res[k] - tw[k]):.2e} bar={bars[k]:.2e}")
        assert abs(res[k] - tw[k]) <= bars[k], (label, k, res[k], tw[k], bars[k])
    for i, (a, b) in enumerate(zip(res["c_amp"], tw["c_amp"])):
        assert abs(a - b) <= bars["c_amp"][i], (label, "c_amp", i, a, b)
    return bars


def _assert_derived(res, beta, k0):
    """the derived fields are the header's expressions on the RETURNED raw forms, to 4 ulp"""
    d = derived(res, beta, k0)
    for k in ("fw", "rho", "beta_eff", "gen_time", "rho_dollars"):
        assert _ulps(res[k], d[k]) <= 4, (k, res[k], d[k])
    assert len(res["beta_eff_i"]) == len(d["beta_eff_i"]) == res["n_families"]
    for a, b in zip(res["beta_eff_i"], d["beta_eff_i"]):
        assert _ulps(a, b) <= 4, (a, b)


# ---- 1. the kernel against the twin, injected fields -------------------------------------------------------------------------------------
_REF = {}


def _injected(dim, rt, p):
    """(inputs, built RefScipy, phi, phi+, twins for chi_d given / NULL) of one case, computed once"""
    key = (dim, rt, p)
    if key not in _REF:
        nx, ny, nz = _trim(dim)
        inp = synthetic_inputs(nx, ny, nz, 3, seed=20 + dim)
        r = ref_from_inputs(inp, rt, p)
        rng = np.random.default_rng(500 + 10 * rt + p)
        phi, adj = rng.standard_normal((3, r.nPhi)), rng.standard_normal((3, r.nPhi))      # sign-mixed
        y = np.stack([r.schur_apply(g, phi[g]) for g in range(3)])
        tw = {cd: kinetics_forms(r, adj, phi, THREE_GROUP_V, SIX_BETA, KEFF, chi_delayed=cd, y=y) for cd in ((1.0, 0.0, 0.0), None)}
        _REF[key] = (inp, r, phi, adj, tw)
    return _REF[key]


def _check_injected(c, r, phi, adj, tw, label):
    c.set_phi(phi); c.set_phi_adj(adj)
    nrm = c.sensitivity(KEFF, which=())["result"]["norm"]
    for cd, t in tw.items():
        res = c.kinetics_params(THREE_GROUP_V, SIX_BETA, SIX_LAMBDA, KEFF, chi_delayed=cd)
        _assert_raw(res, t, adj, f"{label} chi_d={'given' if cd else 'NULL'}")
        _assert_derived(res, SIX_BETA, KEFF)
        assert res["keff"] == KEFF and res["time"] == 0.0 and res["n_families"] == 6 and res["from_transient"] == 0
        assert res["c_amp"] == [0.0] * 6
        assert abs(res["production"] - nrm) <= 1e-13 * abs(nrm), (res["production"], nrm)      # nf_sensitivity's Nrm
        if cd is None:
            assert res["delayed_production"] == res["production"]
            assert all(_ulps(a, b) <= 4 for a, b in zip(res["beta_eff_i"], SIX_BETA))


@pytest.mark.parametrize("dim,rt,p", ORDERS)
def test_forms_match_twin(dim, rt, p):
    """non-uniform 9 x 7 x 5 cells (trimmed per dimension), 3 groups (a down-scatter chain and one up-scatter block), random sign-mixed phi
    and phi+, k0 = 0.9, six families, chi_d given and NULL"""
    inp, r, phi, adj, tw = _injected(dim, rt, p)
    c = make_hip(inp, rt, p)
    _check_injected(c, r, phi, adj, tw, f"dim={dim} RT{rt}-P{p}")
    c.close()


@pytest.mark.parametrize("rt", [0, 1, 2])
def test_grid_stride_wraps_at_one_block(rt):
    """the 3D cases again with option kin_grid = 1: one block of 256 threads walks 315 x (rt + 1)^3 indices, the carried cell index wraps"""
    inp, r, phi, adj, tw = _injected(3, rt, rt)
    c = make_hip(inp, rt, rt)
    c.set_option("kin_grid", 1)
    _check_injected(c, r, phi, adj, tw, f"kin_grid=1 RT{rt}-P{rt}")
    c.close()


# ---- 2. wrap at the default grid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rt", [((300, 1500), 0), ((40, 30), 1)])
def test_larger_grids(n, rt):
    """2D at 300 x 1500 = 450 000 cells, more than the 1024 blocks x 256 threads the launch is capped at (the grid stride wraps), and RT1-P1
    at 40 x 30 (several blocks, moments beyond the first).  The yardstick is too slow there: vectorised numpy with y = S_g phi_g taken from
    schur_apply of the same handle (its own tests cover it)"""
    inp = synthetic_inputs(n[0], n[1], 1, 2, seed=31)
    c = make_hip(inp, rt, rt)
    r = ref_unbuilt(inp, rt, rt)
    r.Mf = fission_matrix(r)
    r.Ms = {(1, 0): np.repeat(np.asarray(inp["SigS"][1, 0], dtype=np.float64).ravel(), r.nloc) * _mass(r)}
    rng = np.random.default_rng(9)
    phi, adj = rng.standard_normal((2, c.n_phi)), rng.standard_normal((2, c.n_phi))
    c.set_phi(phi); c.set_phi_adj(adj)
    y = np.stack([c.schur_apply(g, phi[g]) for g in range(2)])
    tw = kinetics_forms(r, adj, phi, TWO_GROUP_V, SIX_BETA, KEFF, chi_delayed=(1.0, 0.0), y=y)
    res = c.kinetics_params(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, KEFF, chi_delayed=(1.0, 0.0))
    _assert_raw(res, tw, adj, f"{n} RT{rt}")
    _assert_derived(res, SIX_BETA, KEFF)
    c.close()


# ---- 3. static, end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["synthetic", "iaea2d"])
def test_static_reactivity_end_to_end(case):
    """solve_keff, solve_adjoint, SigR of group 2 x 0.97 in the first 16 fuel cells, rebuild, solve_keff again, kinetics_params with k0: (a) rho against the
    twin on the SAME read-back vectors at the bars of the injected fields; (b) the physics, |rho - (1 - k0 / k')| <= 1 % of |rho| -- a sanity
    bound: identity 1 is exact for an exact eigenpair, what is measured here is how converged the solves are (DESIGN.md 19 has the figure)"""
    inp, rt = (load_inputs("iaea2d"), 0) if case == "iaea2d" else (synthetic_inputs(8, 8, 4, 2, seed=4), 1)
    c = make_hip(inp, rt, rt); c.set_tol(*TIGHT)
    k0, _ = c.solve_keff()
    c.solve_adjoint(True, True)
    sig = np.array(inp["SigR"], dtype=np.float64)
    fuel = np.flatnonzero(np.asarray(inp["NSF"][1]).ravel() > 0.0)[:16]      # cells that carry flux: the corner cells of IAEA-2D are reflector
    sig[1].reshape(-1)[fuel] *= 0.97
    up = dict(inp, SigR=sig)
    _rebuild(c, up)
    kp, _ = c.solve_keff()
    res = c.kinetics_params(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k0, chi_delayed=(1.0, 0.0))
    phi, adj = c.get_phi(), c.get_phi_adj()
    c.close()
    tw = kinetics_forms(ref_from_inputs(up, rt, rt), adj, phi, TWO_GROUP_V, SIX_BETA, k0, chi_delayed=(1.0, 0.0))
    bars = _assert_raw(res, tw, adj, f"static {case}")
    _assert_derived(res, SIX_BETA, k0)
    bar_rho = (bars["production"] / k0 + bars["removal_leakage"] + bars["scatter"]) / abs(tw["fw"]) + abs(tw["rho"]) * bars["production"] / abs(tw["production"])
    exact = 1.0 - k0 / kp
    print(f"kin static {case}: rho={res['rho']:.10e} twin={tw['rho']:.10e} (bar {bar_rho:.1e}) 1-k0/k'={exact:.10e} distance={abs(res['rho'] - exact) / abs(res['rho']):.2e} "
          f"beta_eff={res['beta_eff']:.6e} Lambda={res['gen_time']:.6e} rho$={res['rho_dollars']:.5f}")
    assert abs(res["rho"] - tw["rho"]) <= bar_rho
    assert abs(res["rho"]) > 1e-6 and abs(res["rho"] - exact) <= 0.01 * abs(res["rho"])     # a real perturbation, and the sanity bound
    # delayed neutrons born fast are worth at least the average neutron here (IAEA-2D: chi = (1, 0) = chi_d, so beta_eff = beta)
    assert res["beta_eff"] >= sum(SIX_BETA) * (1.0 - 4e-16) and res["gen_time"] > 0.0


# ---- 4. transient ---------------------------------------------------------------------------------------------------------------------------
def left_eigenvector(r, k):
    """the dense left eigenvector of the built RefScipy next to the eigenvalue k by inverse iteration on (K0 - F / k)^T (three solves:
    k is an eigenvalue to the tolerance of the solve that gave it), (ng, n_phi), unit norm, positive sum"""
    import scipy.linalg as sla
    K0, F = dense_operators(r)
    lu = sla.lu_factor((K0 - F / (k * (1.0 + 1e-9))).T)
    w = np.ones(K0.shape[0])
    for _ in range(3):
        w = sla.lu_solve(lu, w); w /= np.linalg.norm(w)
    return (w * np.sign(w.sum())).reshape(r.ng, r.nPhi)


@functools.lru_cache(maxsize=None)
def _weight(case):
    inp, rt, k, _ = _critical_state(case)
    return left_eigenvector(ref_from_inputs(inp, rt, rt), k)


@functools.lru_cache(maxsize=None)
def _scenario_refs(case):
    """the built RefScipy of the two perturbed cores of the scenario, once per case"""
    inp, rt, _, _ = _critical_state(case)
    out, cur = [], dict(inp)
    for factor in (0.97, 1.05):
        cur = dict(cur, SigR=_scaled_sigr(cur, 1, factor))
        out.append((cur, ref_from_inputs(cur, rt, rt)))
    return out


def _compare_step(res, tw, prev_amp, dt, lam, k0, worst, label):
    """transient_kinetics() of one completed step against the twin on the yardstick's state, and identity 2 on the GPU's own numbers"""
    size = abs(res["production"]) / k0 + abs(res["removal_leakage"]) + abs(res["scatter"])
    rel = lambda a, b: abs(a - b) / abs(b)
    for k in RAW + ("fw", "gen_time"):
        worst["scalar"] = max(worst["scalar"], rel(res[k], tw[k]))
        assert rel(res[k], tw[k]) <= EXACT_SCALAR_BAR, (label, k, res[k], tw[k])
    for k in ("beta_eff_i", "c_amp"):
        for a, b in zip(res[k], tw[k]):
            worst["scalar"] = max(worst["scalar"], rel(a, b))
            assert rel(a, b) <= EXACT_SCALAR_BAR, (label, k, a, b)
    d_rho = abs(res["rho"] - tw["rho"]) / (size / res["fw"])
    worst["rho"] = max(worst["rho"], d_rho)
    assert d_rho <= EXACT_SCALAR_BAR, (label, res["rho"], tw["rho"])
    lhs, rhs, _ = balance_residual(prev_amp, res, dt, lam)
    worst["balance"] = max(worst["balance"], abs(lhs - rhs) / size)
    print(f"kin transient {label} t={res['time']:.3f}: rho={res['rho']:.8e} twin={tw['rho']:.8e} rho$={res['rho_dollars']:.5f} beta_eff={res['beta_eff']:.6e} "
          f"Lambda={res['gen_time']:.6e} balance |lhs-rhs|/size={abs(lhs - rhs) / size:.2e}")
    assert abs(lhs - rhs) <= EXACT_FLUX_BAR * size, (label, lhs, rhs, size)


@pytest.mark.parametrize("case,route", [("synthetic", "direct"), ("synthetic", "cg"), ("iaea2d", "direct")])
def test_transient_balance(case, route):
    """the scenario of test_gpu_transient.py (SigR of group 2 x 0.97 in 16 cells, 3 steps of 1e-2, then x 1.05, 2 steps of 1e-3) at EXACT_TOL
    with w = the dense left eigenvector of the unperturbed core: after every step the parameters against the twin on ExactTransient's
    state, and the discrete point-kinetics balance on the GPU's own numbers"""
    inp, rt, k, phi = _critical_state(case)
    w, steps, refs = _weight(case), _reference_scenario(case), _scenario_refs(case)
    s = _solver(inp, rt, rt, pushed=route == "cg")
    s.set_tol(*EXACT_TOL)
    s.set_phi(phi); s.set_phi_adj(w)
    s.transient_begin(TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k, chi_delayed=(1.0, 0.0))
    r0 = s.transient_kinetics()                                   # T^0 of the balance; the critical state: rho = 0 to the solve's tolerance
    assert r0["from_transient"] == 1 and r0["time"] == 0.0 and r0["keff"] == k and abs(r0["rho"]) <= 1e-7
    prev, at = r0["amplitude"], 0
    worst = dict(scalar=0.0, rho=0.0, balance=0.0)
    for (cur, r), (dt, n) in zip(refs, ((1e-2, 3), (1e-3, 2))):
        _rebuild(s, cur)
        for st in steps[at:at + n]:
            out, _ = s.transient_step(dt, 1)
            res = s.transient_kinetics()
            assert res["time"] == out["time"] and res["n_families"] == 6
            tw = kinetics_forms(r, w, st["phi"], TWO_GROUP_V, SIX_BETA, k, chi_delayed=(1.0, 0.0), c=st["c"])
            _assert_derived(res, SIX_BETA, k)
            _compare_step(res, tw, prev, dt, SIX_LAMBDA, k, worst, f"{case}/{route}")
            prev = res["amplitude"]
        at += n
    print(f"kin transient {case}/{route}: worst scalar {worst['scalar']:.2e}, rho {worst['rho']:.2e} of its terms, balance {worst['balance']:.2e} of its terms")
    s.close()


@pytest.mark.parametrize("nfam", [0, 8])
def test_transient_family_bounds(nfam):
    """no family and NF_PRECURSORS_MAX families on the three-group case with two upscatter blocks (20 x 16, RT0-P0)"""
    inp = synthetic_inputs(20, 16, 1, 3, seed=6)
    inp["SigS"][0, 2] = 0.002 * (inp["NSF"][0] > 0)
    beta, lam = (SIX_BETA + (1e-4, 3e-4))[:nfam], (SIX_LAMBDA + (5.0, 0.05))[:nfam]
    chid = (1.0, 0.0, 0.0)
    s = _solver(inp)
    s.set_tol(*KEFF_TOL)
    k, _ = s.solve_keff()
    phi = s.get_phi().copy()
    w = left_eigenvector(ref_from_inputs(inp, 0, 0), k)
    ex = ExactTransient(inp, 0, 0, THREE_GROUP_V, beta, lam, k, phi, chi_delayed=chid)
    s.set_tol(*EXACT_TOL)
    s.set_phi_adj(w)
    s.transient_begin(THREE_GROUP_V, beta, lam, k, chi_delayed=chid)
    prev = s.transient_kinetics()["amplitude"]
    up = dict(inp, SigR=_scaled_sigr(inp, 2, 0.97))
    _rebuild(s, up); ex.set_xs(SigR=up["SigR"])
    r = ref_from_inputs(up, 0, 0)
    worst = dict(scalar=0.0, rho=0.0, balance=0.0)
    for st in ex.step(1e-2, 2):
        s.transient_step(1e-2, 1)
        res = s.transient_kinetics()
        assert res["n_families"] == nfam and len(res["c_amp"]) == len(res["beta_eff_i"]) == nfam
        tw = kinetics_forms(r, w, st["phi"], THREE_GROUP_V, beta, k, chi_delayed=chid, c=st["c"])
        _assert_derived(res, beta, k)
        _compare_step(res, tw, prev, 1e-2, lam, k, worst, f"I={nfam}")
        prev = res["amplitude"]
    if nfam == 0:
        assert res["beta_eff"] == 0.0 and res["rho_dollars"] == 0.0
    s.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------------------
def _warm(s):
    v, k = C.c_int(), C.c_double()
    s._chk(s.L.nf_get_warm_state(s.h, C.byref(v), C.byref(k)))
    return v.value, k.value


def _snapshot(s):
    h = s.history()
    return (s.get_phi().copy(), s.get_phi_adj().copy(), s.get_J().copy(), _warm(s), h["n_outer"], np.array(h["k"]).copy(), np.array(h["cg"]).copy(),
            s.progress(), s.info("transient_rebuilds"), s.info("transient_steps"), s.info("last_outer"), s.info("last_cg_total"))


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_calls_change_no_state():
    inp = synthetic_inputs(9, 7, 1, 3, seed=41)
    up = dict(inp, SigR=_scaled_sigr(inp, 2, 0.97))
    args = (THREE_GROUP_V, SIX_BETA, SIX_LAMBDA)

    def run(with_calls):
        s = make_hip(inp, 1, 1)
        s.set_tol(1e-9, 1e-8, 1e-8, 500, 2000)
        k, _ = s.solve_keff()                                     # nf_get_J, the history and the warm state have something to report
        s.solve_adjoint(True, True)
        s.transient_begin(*args, k, chi_delayed=(1.0, 0.0, 0.0))
        _rebuild(s, up)
        p = [s.transient_step(1e-2, 1)[1][0]]
        if with_calls:
            before = _snapshot(s)
            a, b = s.transient_kinetics(), s.transient_kinetics()
            assert a == b                                         # bit-identical
            c, d = s.kinetics_params(*args, k), s.kinetics_params(*args, k)      # works with a transient running
            assert c == d and c["from_transient"] == 0 and a["from_transient"] == 1
            s.set_option("kin_grid", 3); s.kinetics_params(*args, k, chi_delayed=(1.0, 0.0, 0.0)); s.set_option("kin_grid", 1024)
            assert _same(before, _snapshot(s))
        p.append(s.transient_step(1e-2, 1)[1][0])
        return s, p

    a, pa = run(True)
    b, pb = run(False)
    assert pa == pb                                               # the transient stepped with the calls in between is the one stepped without
    assert np.array_equal(a.get_phi(), b.get_phi()) and all(np.array_equal(a.get_precursors(i), b.get_precursors(i)) for i in range(6))
    assert a.info("transient_rebuilds") == b.info("transient_rebuilds") == 1
    a.close(); b.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from neutfem_amd.capi import HipSolver, HipTeam, KineticsArgs, PkResult
    inp = homogeneous_inputs(2, 2, n=(4, 3, 2))
    v, b, l = (1e7, 3e5), [0.0065], [0.08]
    u = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    u.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    with pytest.raises(RuntimeError, match=r"error -5: nf_kinetics_params.*nf_build"):
        u.kinetics_params(v, b, l, KEFF)
    with pytest.raises(RuntimeError, match=r"error -5: nf_transient_kinetics.*nf_build"):
        u.transient_kinetics()
    u.close()
    s = _solver(inp, pushed=False)
    with pytest.raises(RuntimeError, match=r"error -5: nf_kinetics_params: no adjoint flux"):
        s.kinetics_params(v, b, l, KEFF)
    with pytest.raises(RuntimeError, match=r"error -5: nf_transient_kinetics: no adjoint flux"):
        s.transient_kinetics()
    s.set_phi_adj(np.ones((2, s.n_phi)))
    with pytest.raises(RuntimeError, match=r"error -5: nf_transient_kinetics.*nf_transient_begin"):
        s.transient_kinetics()
    bad = [dict(velocity=(1e7, 0.0)), dict(velocity=(1e7, -1.0)), dict(velocity=(np.inf, 3e5)), dict(lam=[0.0]), dict(lam=[-0.1]), dict(beta=[-1e-3]),
           dict(beta=[0.6, 0.4], lam=[0.08, 0.1]), dict(beta=[np.nan]), dict(lam=[np.inf]), dict(keff=0.0), dict(keff=-1.0), dict(keff=np.nan),
           dict(keff=np.inf), dict(chi_delayed=(np.nan, 0.0)), dict(beta=[1e-4] * 9, lam=[0.1] * 9)]
    for kw in bad:                                                # the rules of nf_transient_begin, in its words under this function's name
        args = dict(velocity=v, beta=b, lam=l, keff=1.0); args.update(kw)
        with pytest.raises(RuntimeError, match=r"error -1: nf_kinetics_params: ") as e1:
            s.kinetics_params(**args)
        with pytest.raises(RuntimeError, match=r"error -1: nf_transient_begin: ") as e2:
            s.transient_begin(**args)
        assert str(e1.value).split("nf_kinetics_params: ")[1] == str(e2.value).split("nf_transient_begin: ")[1]
    k, keep = s._kinetics_args(v, b, l, None)
    assert s.L.nf_kinetics_params(s.h, C.byref(k), KEFF, None) == -1 and b"nf_kinetics_params" in s.L.nf_last_error()
    assert s.L.nf_kinetics_params(s.h, None, KEFF, C.byref(PkResult())) == -1
    assert s.L.nf_transient_kinetics(s.h, None) == -1 and b"nf_transient_kinetics" in s.L.nf_last_error()
    # production = 0 with the other forms alive: chi = (1, 0) and a weight that lives in group 2 only; res still holds the raw forms
    s.set_phi_adj(np.stack([np.zeros(s.n_phi), np.ones(s.n_phi)]))
    res = PkResult()
    assert s.L.nf_kinetics_params(s.h, C.byref(k), KEFF, C.byref(res)) == -6 and b"nf_kinetics_params" in s.L.nf_last_error()
    assert res.production == 0.0 and res.removal_leakage != 0.0 and res.scatter > 0.0 and res.amplitude > 0.0 and res.rho == 0.0 and res.fw == 0.0
    s.set_phi(np.full((2, s.n_phi), 1e308)); s.set_phi_adj(np.full((2, s.n_phi), 1e308))
    with pytest.raises(RuntimeError, match=r"error -6: nf_kinetics_params"):
        s.kinetics_params(v, b, l, KEFF)                          # non-finite forms
    s.set_phi(np.ones((2, s.n_phi))); s.set_phi_adj(np.ones((2, s.n_phi)))
    ok = s.kinetics_params(v, b, l, KEFF)                         # the handle stays usable
    assert np.isfinite(ok["rho"]) and ok["beta_eff"] == b[0]
    s.transient_begin(v, b, l, KEFF)
    assert s.transient_kinetics()["from_transient"] == 1
    s.transient_end()
    with pytest.raises(RuntimeError, match=r"error -5: nf_transient_kinetics"):
        s.transient_kinetics()
    # a handle with cut-out cells
    mask = np.zeros(s.ne, dtype=np.uint8); mask[0] = 1
    s.set_void(mask, 0.4692); s.build()
    with pytest.raises(RuntimeError, match=r"error -4: nf_kinetics_params.*nf_set_void"):
        s.kinetics_params(v, b, l, KEFF)
    with pytest.raises(RuntimeError, match=r"error -4: nf_transient_kinetics.*nf_set_void"):
        s.transient_kinetics()
    s.set_void(None); s.build()
    assert s.kinetics_params(v, b, l, KEFF) == ok
    s.close()
    # a two-slab team
    s3 = synthetic_inputs(4, 4, 6, 2, seed=83)
    team = HipTeam(0, 0, 2, s3["x_breaks"], s3["y_breaks"], s3["z_breaks"], [(0, 3), (3, 6)])
    team.upload_xs_global(s3["D"], s3["SigR"], s3["NSF"], s3["Chi"], s3["SigS"]); team.build()
    for sl in team.slabs:
        sl.set_phi_adj(np.ones((2, sl.n_phi)))
        with pytest.raises(RuntimeError, match=r"error -4: nf_kinetics_params"):
            sl.kinetics_params(v, b, l, KEFF)
        with pytest.raises(RuntimeError, match=r"error -4: nf_transient_kinetics"):
            sl.transient_kinetics()
    team.close()


# ---- 7. pybind ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_pybind_matches_the_c_abi(dim):
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    nx, ny, nz = _trim(dim, (8, 6, 4))
    inp = synthetic_inputs(nx, ny, nz, 2, seed=90 + dim, void_frac=0.0)
    tol = (1e-10, 1e-9, 1e-9, 1000, 2000)
    p = ns.NeutFEM(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    p.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        p.set_bc(int(a), ns.BCType(int(t)), 0.0)
    p.get_D()[...] = inp["D"]; p.get_SigR()[...] = inp["SigR"]; p.get_NSF()[...] = inp["NSF"]; p.get_Chi()[...] = inp["Chi"]; p.get_SigS()[...] = inp["SigS"]
    p.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    p.set_tol(*tol)
    args = (TWO_GROUP_V, SIX_BETA, SIX_LAMBDA)
    with pytest.raises(RuntimeError, match="BuildMatrices"):
        p.kinetics_parameters(*args)
    with pytest.raises(RuntimeError, match="BuildMatrices"):
        p.get_transient_kinetics()
    p.BuildMatrices()
    with pytest.raises(RuntimeError, match="SolveKeff"):
        p.kinetics_parameters(*args)
    k = p.SolveKeff()
    with pytest.raises(RuntimeError, match="SolveAdjoint"):
        p.kinetics_parameters(*args)
    with pytest.raises(RuntimeError, match="begin_transient"):
        p.get_transient_kinetics()
    p.SolveAdjoint(True, True)
    flux, adj = np.array(p.get_flux()).copy(), np.array(p.get_flux_adj()).copy()
    with pytest.raises(RuntimeError, match="nf_kinetics_params: velocity of group 1"):     # the C ABI's text
        p.kinetics_parameters((1e7, -1.0), SIX_BETA, SIX_LAMBDA)
    static = p.kinetics_parameters(*args, chi_delayed=(1.0, 0.0))
    assert static["keff"] == k == p.GetLastKeff() and len(static["beta_eff_i"]) == len(static["c_amp"]) == static["n_families"] == 6
    assert np.array_equal(p.get_flux(), flux) and np.array_equal(p.get_flux_adj(), adj)
    h = make_hip(inp); h.set_tol(*tol)                            # RT0-P0: the mirrors are the whole fields, the inputs are the same bits
    h.set_phi(flux.reshape(2, -1)); h.set_phi_adj(adj.reshape(2, -1))
    assert h.kinetics_params(*args, k, chi_delayed=(1.0, 0.0)) == static
    assert h.kinetics_params(*args, k) == p.kinetics_parameters(*args)
    # the transient: the same perturbation and steps on both sides
    p.begin_transient(*args, chi_delayed=(1.0, 0.0))
    p.get_SigR()[1].reshape(-1)[:16] *= 0.97
    p.BuildMatrices()
    p.step_transient(1e-2, 2)
    dyn = p.get_transient_kinetics()
    h.transient_begin(*args, k, chi_delayed=(1.0, 0.0))
    _rebuild(h, dict(inp, SigR=_scaled_sigr(inp, 1, 0.97)))
    h.transient_step(1e-2, 2)
    ref = h.transient_kinetics()
    assert dyn["from_transient"] == 1 and dyn["n_families"] == 6 and dyn["time"] == ref["time"] and dyn["keff"] == k
    for key in RAW + ("rho", "rho_dollars", "beta_eff", "gen_time", "fw"):
        assert abs(dyn[key] - ref[key]) <= 1e-12 * max(abs(ref[key]), abs(ref["fw"]) if key == "rho" else 0.0), (key, dyn[key], ref[key])
    for key in ("beta_eff_i", "c_amp"):
        assert len(dyn[key]) == 6 and all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(dyn[key], ref[key])), key
    h.close()
