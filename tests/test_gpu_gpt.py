"""GPU tests of the generalized adjoint and the response-ratio maps (nf_solve_gpt, nf_gpt_sensitivity, HipSolver.solve_gpt, SolveGPT;
DESIGN.md 18) against the numpy yardstick of tests/gpt_exact.py: the maps of injected fields, the response / source / deflation kernels
alone, the solve against its twin at fixed work on every group solver and every form of the CG iteration, the convergence to the dense
Gamma+, the first-order prediction end to end, the state of the handle, the errors and the pybind surface.

Measured on an MI355X (the figures enter no assertion except EXACT_MEASURED, whose tenfold stays below the floor of its bar):
  maps of injected fields             every map and <Gamma, F phi> <= 1e-13, dD below its derived bar, also with one block per group
  fixed work, exact group solves      |G12 - twin| 5.4e-16 .. 2.2e-14 relative L2 (dense S^-1 <= 5.0e-15, stand-in <= 2.2e-14); bar 1e-12
  fixed work, CG forms (M0 / M1)      1.7e-11 .. 1.8e-11 / 1.4e-11 on xcd, fuse3, lean, fused, classic; bar 1e-8
  convergence to 1e-10, dense branch  3.8e-10 / 3.5e-10 / 2.1e-10 in 105 / 103 / 66 outers (the twin's counts), contraction 0.817 / 0.812 / 0.720
  end to end                          predicted dR/R 1.033713e-3 / 1.016705e-3: 4.7e-10 / 6.3e-9 from the twin, 1.62 % / 1.42 % from the true change
  deflation residual after a solve    3e-18 .. 1e-17"""
import ctypes as C
import functools

import numpy as np
import pytest

from gpt_exact import dense_gamma, direct_maps, fission_of, gpt_maps, gpt_source, iterate_gamma, predicted_dR, response
from helpers import CG_FORMS, degenerate_inputs, make_hip, rel_l2, synthetic_inputs
from project_exact import random_coefficients
from sens_exact import dominant_pair, flat_inputs, perturbed_block
from subcrit_exact import ref_from_inputs
from test_gpt_exact import block_weights, weights
from test_gpu_driver_forms import LAST_DIRECT, ROUTES, _new, _planned, _ref as _form_ref, _reported
from test_gpu_sensitivity import KEFF, MAPS, MASS_BAR, ORDERS, _current_distance, _field, _trim, _warm, _with_mirrors

pytestmark = pytest.mark.gpu

GPT_MAPS = MAPS + ("Wa", "Wb")
SUM_BAR = 1e-13                                                   # a sum against the sum of the absolute values of its terms
EXACT_FLOOR = 1e-12                                               # floor of the fixed-work bar where the group solves are exact
CG_BAR = 1e-8                                                     # fixed work on a CG form against the twin (the flux bar of test_gpu_subcritical / test_gpu_driver_forms)
N_FIXED = 12


def _gamma_field(ng, ne, nloc, seed):
    return random_coefficients(ng, ne, nloc, seed=seed).reshape(ng, ne * nloc)


# ---- 1. the maps of injected fields ---------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(key, inp, rt, p):
    """(built RefScipy, phi, phi+, Gamma, w_a, w_b, yardstick maps at k = 0.9) of one case, computed once"""
    if key not in _REF:
        r = ref_from_inputs(inp, rt, p)
        ng = int(inp["ng"])
        phi, adj, gam = _field(ng, r.ne, r.nloc, 7 + rt), _field(ng, r.ne, r.nloc, 107 + p), _gamma_field(ng, r.ne, r.nloc, 207 + rt + p)
        wa, wb = weights(ng, r.ne, seed=3 + rt)
        ref = gpt_maps(r, KEFF, phi, gam); ref.update(direct_maps(r, phi, wa, wb))
        ref["scale"] = float(np.linalg.norm(gam) * np.linalg.norm(fission_of(r, phi)))
        _REF[key] = (r, phi, adj, gam, wa, wb, ref)
    return _REF[key]


def _inject(c, phi, adj, gam, wa, wb):
    c.set_phi(phi); c.set_phi_adj(adj)
    c.gpt_source(wa, wb, want_source=False)                       # the weights of the direct maps
    c.set_gamma(gam)


def _compare(c, case, label, bar_d):
    r, phi, adj, gam, wa, wb, ref = case
    _inject(c, phi, adj, gam, wa, wb)
    out = c.gpt_sensitivity(KEFF)
    errs = {w: rel_l2(out[w], ref[w]) for w in GPT_MAPS}
    e_nrm = abs(out["result"]["norm"] - ref["gamma_F_phi"]) / ref["scale"]
    print(f"gpt maps {label}: " + " ".join(f"{w}={errs[w]:.2e}" for w in GPT_MAPS) + f" <G,F phi>={e_nrm:.2e} | dD bar {bar_d:.2e}")
    assert out["result"]["keff"] == KEFF and out["result"]["n_cells"] == r.ne
    assert e_nrm <= MASS_BAR, e_nrm
    for w in ("SigR", "SigS", "NSF", "Chi", "Wa", "Wb"):
        assert errs[w] <= MASS_BAR, (w, errs[w])
    assert errs["D"] <= bar_d, (errs["D"], bar_d)
    for g in range(r.ng):
        assert not out["SigS"][g, g].any()
    return out


@pytest.mark.parametrize("dim,rt,p", ORDERS)
def test_maps_of_injected_fields(dim, rt, p):
    """the cases of test_gpu_sensitivity.py::test_maps_match_yardstick with a random Gamma (any sign) in place of phi+ and c = -1; the bar of
    dD is that file's: 10 x the distance between nf_get_J and the yardstick's current (floor 1e-13), measured first"""
    nx, ny, nz = _trim(dim)
    inp = synthetic_inputs(nx, ny, nz, 3, seed=20 + dim)
    case = _reference(("dir", dim, rt, p), inp, rt, p)
    c = make_hip(inp, rt, p)
    bar_d = max(10.0 * _current_distance(c, case[0]), 1e-13)
    _compare(c, case, f"dim={dim} RT{rt}-P{p}", bar_d)
    c.close()


@pytest.mark.parametrize("rt", [0, 1, 2])
def test_grid_stride_wraps_in_every_kernel(rt):
    """9 x 7 x 5 with the launches held to one block per group (option sens_grid): 315 cells on 256 threads, so k_gpt_response,
    k_gpt_source, k_gpt_defl_dot and the section-14 kernels all take a second trip of their grid stride.  dD at the floor of its bar"""
    inp = synthetic_inputs(9, 7, 5, 3, seed=23)
    case = _reference(("dir", 3, rt, rt), inp, rt, rt)
    c = make_hip(inp, rt, rt)
    c.set_option("sens_grid", 1)
    _compare(c, case, f"sens_grid=1 RT{rt}-P{rt}", 1e-13)
    c.close()


def test_skipped_outputs_are_bit_identical():
    inp = synthetic_inputs(9, 7, 1, 3, seed=20 + 2)
    case = _reference(("dir", 2, 1, 1), inp, 1, 1)
    c = make_hip(inp, 1, 1)
    _inject(c, *case[1:6])
    full = c.gpt_sensitivity(KEFF)
    again = c.gpt_sensitivity(KEFF)
    for w in GPT_MAPS:
        assert np.array_equal(full[w], again[w]), w
    assert full["result"] == again["result"]
    for left_out in GPT_MAPS:
        part = c.gpt_sensitivity(KEFF, which=tuple(w for w in GPT_MAPS if w != left_out))
        assert left_out not in part and part["result"] == full["result"]
        for w in GPT_MAPS:
            if w != left_out:
                assert np.array_equal(part[w], full[w]), (left_out, w)
    only = c.gpt_sensitivity(KEFF, which=())
    assert set(only) == {"result"} and only["result"] == full["result"]
    with pytest.raises(ValueError):
        c.gpt_sensitivity(KEFF, which=("D", "Sigma"))
    c.close()


# ---- 2. response, source and deflation kernels alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("dim,rt", [(1, 2), (2, 0), (2, 1), (3, 0), (3, 2)])
def test_response_and_source(dim, rt, grid):
    nx, ny, nz = _trim(dim)
    inp = synthetic_inputs(nx, ny, nz, 3, seed=20 + dim)
    r, phi, adj, _, wa, wb, _ = _reference(("dir", dim, rt, rt), inp, rt, rt)
    wa = wa * np.where(np.random.default_rng(1).random(wa.shape) < 0.3, -1.0, 1.0)      # any finite values: some negative
    c = make_hip(inp, rt, rt)
    if grid: c.set_option("sens_grid", grid)
    c.set_phi(phi); c.set_phi_adj(adj)
    src, (sa, sb) = c.gpt_source(wa, wb)
    R, a, b = response(r, phi, wa, wb)
    vol_phi = np.abs(phi.reshape(3, r.ne, r.nloc)[:, :, 0]) * np.einsum("k,j,i->kji", r.hz, r.hy, r.hx).ravel()[None, :]
    abs_a, abs_b = float((np.abs(wa) * vol_phi).sum()), float((np.abs(wb) * vol_phi).sum())
    S = gpt_source(r, phi, wa, wb)
    e_src, e_orth = rel_l2(src, S), abs((src * phi).sum()) / np.abs(src * phi).sum()
    print(f"gpt response dim={dim} RT{rt} grid={grid}: <wa,phi> {abs(sa - a) / abs_a:.2e} <wb,phi> {abs(sb - b) / abs_b:.2e} S+ {e_src:.2e} <S+,phi> {e_orth:.2e}")
    assert abs(sa - a) <= SUM_BAR * abs_a and abs(sb - b) <= SUM_BAR * abs_b
    assert abs(sa / sb - R) <= SUM_BAR * (abs_a / abs(b) + abs(a) * abs_b / b ** 2)
    assert e_src <= MASS_BAR and e_orth <= SUM_BAR
    assert not src.reshape(3, r.ne, r.nloc)[:, :, 1:].any()       # the higher moments carry no source
    c.close()


@pytest.mark.parametrize("grid", [0, 1])
def test_deflation_residual_after_a_solve(grid):
    """injected random phi / phi+ (positive cell means), 5 outers on the dense branch: whatever the iterate is, the deflation leaves
    |<Gamma, F phi>| / (||Gamma|| ||F phi||) at rounding, and the result's figure is the one numpy finds in the returned Gamma"""
    inp = synthetic_inputs(9, 7, 5, 3, seed=23)
    r, phi, adj, _, wa, wb, _ = _reference(("dir", 3, 1, 1), inp, 1, 1)
    c = make_hip(inp, 1, 1); c.set_linear_solver(1)
    if grid: c.set_option("sens_grid", grid)
    c.set_tol(0.0, 0.0, 0.0, 5, 1000)
    c.set_phi(phi); c.set_phi_adj(adj)
    res = c.solve_gpt(wa, wb, KEFF)
    G = c.get_gamma(); Fp = fission_of(r, phi)
    mine = abs((G * Fp).sum()) / (np.linalg.norm(G) * np.linalg.norm(Fp))
    print(f"gpt deflation grid={grid}: reported {res['deflation']:.2e}, numpy on the returned Gamma {mine:.2e}; norm {res['norm']:.6e}")
    assert res["n_outer"] == 5 and res["converged"] == 0
    assert res["deflation"] <= 1e-12 and mine <= 1e-12
    assert abs(res["norm"] - (adj * Fp).sum()) <= MASS_BAR * np.abs(adj * Fp).sum()
    c.close()


# ---- 3. the solve against the twin at fixed work ----------------------------------------------------------------------------------------------
EXACT_CASES = {  # name -> (inputs, rt): at most ~1000 unknowns, the dense eigenproblem of the twin stays at seconds
    "1d-rt0": (lambda: synthetic_inputs(9, 1, 1, 3, seed=21), 0), "1d-rt1": (lambda: synthetic_inputs(9, 1, 1, 3, seed=21), 1),
    "1d-rt2": (lambda: synthetic_inputs(9, 1, 1, 3, seed=21), 2),
    "2d-rt0": (lambda: synthetic_inputs(9, 7, 1, 3, seed=22), 0), "2d-rt1": (lambda: synthetic_inputs(9, 7, 1, 3, seed=22), 1),
    "2d-rt2": (lambda: synthetic_inputs(6, 5, 1, 3, seed=22), 2),
    "3d-rt0": (lambda: synthetic_inputs(9, 7, 5, 3, seed=23), 0), "3d-rt1": (lambda: synthetic_inputs(4, 3, 3, 3, seed=23), 1),
    "3d-rt2": (lambda: synthetic_inputs(3, 2, 2, 3, seed=23), 2),
    "2d-mirror-rt1": (lambda: _with_mirrors(synthetic_inputs(9, 7, 1, 3, seed=22), (1, 4)), 1),
    "3d-mirror-rt0": (lambda: _with_mirrors(synthetic_inputs(9, 7, 5, 3, seed=23), (1, 4, 5)), 0),
    "deg513-rt0": (lambda: degenerate_inputs(5, 1, 3), 0), "deg513-rt1": (lambda: degenerate_inputs(5, 1, 3), 1),
}


@functools.lru_cache(maxsize=None)
def _twin(name):
    """the dense k, phi, phi+ of a case, its weights and the twin's iterate after N_FIXED outers with the change of every outer"""
    make, rt = EXACT_CASES[name]
    inp = make()
    r = ref_from_inputs(inp, rt, rt)
    k, phi, adj = dominant_pair(r)
    wa, wb = weights(r.ng, r.ne, seed=9)
    G, ch = iterate_gamma(r, k, phi, adj, wa, wb, n_outer=N_FIXED + 1)
    G12, _ = iterate_gamma(r, k, phi, adj, wa, wb, n_outer=N_FIXED)
    for a in (phi, adj, wa, wb, G12): a.setflags(write=False)
    return dict(inp=inp, rt=rt, r=r, k=k, phi=phi, adj=adj, wa=wa, wb=wb, G=G12, changes=ch)


EXACT_MEASURED = 2.2e-14                                          # worst relative L2 of the test below over every case and both routes, MI355X (3d-rt2, stand-in)
EXACT_BAR = max(10 * EXACT_MEASURED, EXACT_FLOOR)


@pytest.mark.parametrize("route", ["dense", "standin"])
@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_fixed_work_exact_group_solves(name, route):
    """dense k, phi, phi+ injected; tol_flux between the twin's changes of outers 11 and 12, so exactly 12 outers run on both sides.
    Dense S^-1 and the CG-to-1e-14 stand-in solve the groups exactly: the bar is 10 x the worst relative L2 measured over these cases
    on an MI355X, floor 1e-12"""
    t = _twin(name)
    c = make_hip(t["inp"], t["rt"], t["rt"]); c.set_linear_solver(1)
    if route == "standin": c.set_option("direct_max_dofs", 0)
    tol = float(np.sqrt(t["changes"][N_FIXED - 1] * t["changes"][N_FIXED - 2]))
    c.set_tol(0.0, tol, 0.0, 50, 1000)
    c.set_phi(t["phi"]); c.set_phi_adj(t["adj"])
    res = c.solve_gpt(t["wa"], t["wb"], t["k"])
    err = rel_l2(c.get_gamma(), t["G"])
    print(f"gpt fixed work {name} {route}: outers {res['n_outer']} dgamma {res['dgamma']:.3e} (twin {t['changes'][N_FIXED - 1]:.3e}) |G12 - twin| = {err:.2e} cg {res['cg_total']}")
    assert res["n_outer"] == N_FIXED and res["converged"] == 1
    assert c.info("last_direct") == LAST_DIRECT[route]
    assert abs(res["dgamma"] - t["changes"][N_FIXED - 1]) <= 1e-6 * t["changes"][N_FIXED - 1]
    assert abs(res["R"] - response(t["r"], t["phi"], t["wa"], t["wb"])[0]) <= 1e-12 * abs(res["R"])
    assert err <= EXACT_BAR, (err, EXACT_BAR)
    c.close()


@functools.lru_cache(maxsize=None)
def _twin_form(mesh):
    r = _form_ref(mesh)
    k, phi, adj = dominant_pair(r)
    wa, wb = weights(2, r.ne, seed=9)
    G, ch = iterate_gamma(r, k, phi, adj, wa, wb, n_outer=N_FIXED)
    for a in (phi, adj, wa, wb, G): a.setflags(write=False)
    return dict(k=k, phi=phi, adj=adj, wa=wa, wb=wb, G=G, changes=ch)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("mesh", ["M0", "M1"])
def test_fixed_work_on_every_form(mesh, route):
    """the meshes and routes of tests/test_gpu_driver_forms.py: every form cg_plan can return on an undivided mesh (xcd, fuse3, lean,
    fused, classic), the dense S^-1 and the stand-in.  On a CG form tol_flux is also the tolerance of the group solves, so the work is
    fixed by max_outer = 12 with tol_flux = 1e-11 (the contraction leaves the outer test far from firing); bar 1e-8"""
    t = _twin_form(mesh)
    label = f"gpt {mesh} {route}"
    kind = ROUTES[route][0]
    form = route if kind == "cg" else None if route == "dense" else "fuse3"
    s = _new(mesh, route)
    s.set_tol(0.0, 1e-11, 0.0, N_FIXED, 5000)
    s.set_phi(t["phi"]); s.set_phi_adj(t["adj"])
    _planned(s, form, label)
    res = s.solve_gpt(t["wa"], t["wb"], t["k"])
    _reported(s, route, form, label)
    err = rel_l2(s.get_gamma(), t["G"])
    print(f"{label}: outers {res['n_outer']} cg {res['cg_total']} form {CG_FORMS[s.info('cg_form')] if form else '-'} |G12 - twin| = {err:.2e}")
    assert res["n_outer"] == N_FIXED and res["converged"] == 0
    assert err <= (CG_BAR if kind == "cg" else EXACT_BAR), err
    s.close()


# ---- 4. convergence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-rt0", "2d-rt1", "3d-rt0"])
def test_converges_to_dense_gamma(name):
    """to tol_flux = 1e-10 on the dense branch: the error against the dense Gamma+ is at most 10 tol / (1 - rho) with rho the contraction the
    result reports, and the outer count is within 2 of the twin's"""
    t = _twin(name)
    tol = 1e-10
    exact = dense_gamma(t["r"], t["k"], t["phi"], t["adj"], t["wa"], t["wb"])
    _, ch = iterate_gamma(t["r"], t["k"], t["phi"], t["adj"], t["wa"], t["wb"], tol=tol)
    c = make_hip(t["inp"], t["rt"], t["rt"]); c.set_linear_solver(1)
    c.set_tol(0.0, tol, 0.0, 2000, 1000)
    c.set_phi(t["phi"]); c.set_phi_adj(t["adj"])
    res = c.solve_gpt(t["wa"], t["wb"], t["k"])
    err = rel_l2(c.get_gamma(), exact)
    print(f"gpt convergence {name}: outers {res['n_outer']} (twin {len(ch)}) contraction {res['ratio']:.3f} |G - dense| = {err:.2e} deflation {res['deflation']:.1e}")
    assert res["converged"] == 1 and c.info("last_direct") == 1
    assert 0 < res["ratio"] < 1
    assert err <= 10 * tol / (1 - res["ratio"]), (err, res["ratio"])
    assert abs(res["n_outer"] - len(ch)) <= 2
    assert res["deflation"] <= 1e-12
    c.close()


# ---- 5. end to end on the device --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [0, 1])
def test_first_order_prediction_end_to_end(rt):
    """solve_keff, solve_adjoint, solve_gpt, gpt_sensitivity on the 9 x 7 case; R = the share of the perturbed block.  The predicted dR / R
    of +1 % SigR_1, -1 % D_0, +1 % nuSigf_1 on rows 2-4 x columns 3-6 against R of a second solve_keff on the perturbed input: within 3 %;
    and within 1e-5 relative of the twin's prediction"""
    base = flat_inputs(synthetic_inputs(9, 7, 1, 2, seed=8))
    pert = perturbed_block(base)
    wa, wb = block_weights("perturbed")
    tol = (1e-10, 1e-9, 1e-10, 2000, 1000)
    c = make_hip(base, rt, rt); c.set_tol(*tol)
    k, n = c.solve_keff()
    _, na = c.solve_adjoint(True, True)
    res = c.solve_gpt(wa, wb)                                     # k from the warm state
    assert n < 2000 and na < 2000 and res["converged"] == 1, (n, na, res)
    pred = predicted_dR(c.gpt_sensitivity(k, which=MAPS), base, pert)
    d = make_hip(pert, rt, rt); d.set_tol(*tol)
    d.solve_keff()
    r = ref_from_inputs(base, rt, rt)
    a2, b2 = response(r, d.get_phi(), wa, wb)[1:]                  # the mesh of r is the perturbed handle's too
    true = (a2 / b2) / res["R"] - 1.0
    kk, phi, adj = dominant_pair(r)
    G, _ = iterate_gamma(r, kk, phi, adj, wa, wb, tol=1e-10)
    twin = predicted_dR(gpt_maps(r, kk, phi, G), base, pert)
    print(f"gpt end to end RT{rt}-P{rt}: k={k:.10f} R={res['R']:.8f} outers {n}/{na}/{res['n_outer']} predicted dR/R={pred:.6e} twin {twin:.6e} "
          f"({abs(pred / twin - 1):.1e}) true {true:.6e} ({abs(pred / true - 1):.2%})")
    assert abs(true) > 1e-5 and abs(pred - true) <= 0.03 * abs(true), (pred, true)
    assert abs(pred - twin) <= 1e-5 * abs(twin), (pred, twin)
    c.close(); d.close()


# ---- 6. state, errors, pybind -----------------------------------------------------------------------------------------------------------------
def test_state_is_untouched_and_calls_repeat():
    inp = synthetic_inputs(9, 7, 1, 3, seed=41)
    c = make_hip(inp, 1, 1)
    c.set_tol(1e-8, 1e-7, 1e-7, 500, 2000)
    k, _ = c.solve_keff()
    c.solve_adjoint(True, True)
    wa, wb = weights(3, c.ne, seed=2)
    hist = lambda: tuple(np.array(x) for x in _history(c))
    sens0 = c.sensitivity(k)
    before = (c.get_phi().copy(), c.get_phi_adj().copy(), _warm(c), c.get_J().copy(), c.info("last_outer"), c.info("last_cg_total"), hist())
    r1 = c.solve_gpt(wa, wb, k); g1 = c.get_gamma().copy(); m1 = c.gpt_sensitivity(k)
    r2 = c.solve_gpt(wa, wb, k); g2 = c.get_gamma().copy(); m2 = c.gpt_sensitivity(k)
    assert r1 == r2 and np.array_equal(g1, g2)
    for w in GPT_MAPS:
        assert np.array_equal(m1[w], m2[w]), w
    assert m1["result"] == m2["result"]
    c.set_gamma(g1)
    assert np.array_equal(c.get_gamma(), g1)
    after = (c.get_phi(), c.get_phi_adj(), _warm(c), c.get_J(), c.info("last_outer"), c.info("last_cg_total"), hist())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert np.array_equal(before[3], after[3]) and before[4:6] == after[4:6]
    for a, b in zip(before[6], after[6]):
        assert np.array_equal(a, b)
    sens1 = c.sensitivity(k)
    for w in MAPS:
        assert np.array_equal(sens0[w], sens1[w]), w
    assert sens0["result"] == sens1["result"]
    c.close()


def _history(c):
    n = c.info("last_outer")
    k, dk, dphi = np.zeros(n), np.zeros(n), np.zeros(n); cg = np.zeros(n * c.ng, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    c._chk(c.L.nf_get_history(c.h, k.ctypes.data_as(dp), dk.ctypes.data_as(dp), dphi.ctypes.data_as(dp), cg.ctypes.data_as(ip), n))
    return k, dk, dphi, cg


NO_GAMMA = r"error -5: .*no generalized adjoint"


def test_gamma_is_dropped_with_the_operator():
    inp = synthetic_inputs(6, 5, 1, 2, seed=81)
    c = make_hip(inp)
    c.set_tol(1e-6, 1e-6, 1e-6, 200, 1000)
    c.set_phi_adj(np.ones((2, c.n_phi)))
    wa, wb = weights(2, c.ne, seed=2)
    xs = (inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    drops = {"upload_xs": lambda: (c.upload_xs(*xs), c.build()), "build": c.build, "set_bc": lambda: c.set_bc(1, 0),
             "set_void": lambda: (c.set_void(np.zeros(c.ne, int), 0.5), c.build())}
    for name, drop in drops.items():
        c.solve_gpt(wa, wb, 0.9)
        assert np.isfinite(c.get_gamma()).all()
        drop()
        with pytest.raises(RuntimeError, match=NO_GAMMA):
            c.get_gamma()
        with pytest.raises(RuntimeError, match=NO_GAMMA):
            c.gpt_sensitivity(0.9)
    c.close()


def test_errors():
    from neutfem_amd.capi import HipSolver, HipTeam
    inp = synthetic_inputs(6, 5, 1, 2, seed=81, nonuniform=False)
    ne = 30
    wa, wb = weights(2, ne, seed=2)
    u = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    u.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    with pytest.raises(RuntimeError, match=r"error -5: .*nf_build"):
        u.solve_gpt(wa, wb, 0.9)
    with pytest.raises(RuntimeError, match=r"error -5: .*nf_build"):
        u.gpt_sensitivity(0.9)
    u.close()
    c = make_hip(inp)
    c.set_tol(1e-6, 1e-6, 1e-6, 200, 1000)
    with pytest.raises(RuntimeError, match=r"error -5: .*no adjoint flux \(nf_solve_adjoint or nf_set_phi_adj first\)"):
        c.solve_gpt(wa, wb, 0.9)
    with pytest.raises(RuntimeError, match=NO_GAMMA):
        c.gpt_sensitivity(0.9)
    with pytest.raises(RuntimeError, match=NO_GAMMA):
        c.get_gamma()
    c.set_phi_adj(np.ones((2, c.n_phi)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"error -1: .*keff"):
            c.solve_gpt(wa, wb, bad)
    for i, bad in enumerate((float("nan"), float("inf"))):
        w = (wa if i else wb).copy(); w[1, 3] = bad
        with pytest.raises(RuntimeError, match=r"error -1: .*non-finite weight in group 1, cell 3"):
            c.solve_gpt(w if i else wa, wb if i else w, 0.9)
    for lam in (1.0, 2.0, -0.5):
        with pytest.raises(RuntimeError, match=r"error -1: .*identically zero"):
            c.solve_gpt(lam * wb, wb, 0.9)
    for kw in (dict(use_diag=True), dict(use_cmfd=True), dict(use_coarse=True, factors=(2, 1))):
        with pytest.raises(RuntimeError, match=r"error -1: .*use_coarse_init, use_cmfd and use_diagonal_solver"):
            c.solve_gpt(wa, wb, 0.9, **kw)
    # uniform mesh, flux 1: +1 and -1 on two cells cancel exactly
    cancel = np.zeros((2, ne)); cancel[0, 4] = 1.0; cancel[1, 7] = -1.0
    with pytest.raises(RuntimeError, match=r"error -6: .*numerator <w_a, phi>"):
        c.solve_gpt(cancel, wb, 0.9)
    with pytest.raises(RuntimeError, match=r"error -6: .*denominator <w_b, phi>"):
        c.solve_gpt(wa, cancel, 0.9)
    with pytest.raises(RuntimeError, match=r"error -6: .*numerator <w_a, phi>"):
        c.solve_gpt(np.zeros((2, ne)), wb, 0.9)
    c.set_phi_adj(np.zeros((2, c.n_phi)))
    with pytest.raises(RuntimeError, match=r"error -6: .*phi\+\^T F phi"):
        c.solve_gpt(wa, wb, 0.9)                                  # <phi+, F phi> = 0
    c.set_phi_adj(np.ones((2, c.n_phi)))
    c.set_phi(np.full((2, c.n_phi), 1e200)); c.set_phi_adj(np.full((2, c.n_phi), 1e200))
    with pytest.raises(RuntimeError, match=r"error -6: "):
        c.solve_gpt(wa, wb, 0.9)                                  # <phi+, F phi> = inf
    c.set_phi(np.ones((2, c.n_phi))); c.set_phi_adj(np.ones((2, c.n_phi)))
    with pytest.raises(RuntimeError, match=r"error -6: .*non-finite iterate"):
        c.solve_gpt(wa, wb, 1e-200)                               # 1 / k = 1e200 on the fission term: ||Gamma||^2 overflows in the second outer
    with pytest.raises(RuntimeError, match=NO_GAMMA):
        c.get_gamma()                                             # a failed solve leaves no Gamma
    res = c.solve_gpt(wa, wb, 0.9)                                # the handle stays usable
    assert np.isfinite(res["R"]) and np.isfinite(c.get_gamma()).all() and np.isfinite(c.gpt_sensitivity(0.9)["D"]).all()
    c.set_gamma(c.get_gamma())
    c.close()
    # a handle without weights: the cross-section maps work on an injected Gamma, the maps of the weights do not
    c = make_hip(inp)
    c.set_phi_adj(np.ones((2, c.n_phi))); c.set_gamma(np.ones((2, c.n_phi)))
    assert set(c.gpt_sensitivity(0.9, which=MAPS)) == set(MAPS) | {"result"}
    with pytest.raises(RuntimeError, match=r"error -5: .*weights"):
        c.gpt_sensitivity(0.9, which=("Wa",))
    # a masked handle: refused through nf_set_void's text, before anything else
    mask = np.zeros(ne, int); mask[0] = 1
    c.set_void(mask, 0.4692); c.build()
    for call in (lambda: c.solve_gpt(wa, wb, 0.9), lambda: c.gpt_sensitivity(0.9), lambda: c.gpt_source(wa, wb)):
        with pytest.raises(RuntimeError, match=r"error -4: .*nf_set_void"):
            call()
    c.close()
    s3 = synthetic_inputs(4, 4, 6, 2, seed=83)
    team = HipTeam(0, 0, 2, s3["x_breaks"], s3["y_breaks"], s3["z_breaks"], [(0, 3), (3, 6)])
    team.upload_xs_global(s3["D"], s3["SigR"], s3["NSF"], s3["Chi"], s3["SigS"]); team.build()
    for s in team.slabs:
        s.set_phi_adj(np.ones((2, s.n_phi))); s.set_gamma(np.ones((2, s.n_phi)))
        w = np.ones((2, s.ne)); w2 = w.copy(); w2[0, 0] = 2.0
        with pytest.raises(RuntimeError, match=r"error -4: "):
            s.solve_gpt(w2, w, 0.9)
        with pytest.raises(RuntimeError, match=r"error -4: "):
            s.gpt_sensitivity(0.9)
    team.close()


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_pybind_matches_ctypes(dim):
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    nx, ny, nz = _trim(dim, (8, 6, 4))
    inp = synthetic_inputs(nx, ny, nz, 2, seed=90 + dim, void_frac=0.0)
    tol = (1e-10, 1e-9, 1e-9, 1000, 2000)
    s = ns.NeutFEM(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    s.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        s.set_bc(int(a), ns.BCType(int(t)), 0.0)
    s.get_D()[...] = inp["D"]; s.get_SigR()[...] = inp["SigR"]; s.get_NSF()[...] = inp["NSF"]; s.get_Chi()[...] = inp["Chi"]; s.get_SigS()[...] = inp["SigS"]
    s.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    s.set_tol(*tol)
    wa, wb = weights(2, nx * ny * nz, seed=4)
    num, den = wa.reshape(s.get_D().shape), wb.reshape(s.get_D().shape)
    with pytest.raises(RuntimeError, match="BuildMatrices"):
        s.SolveGPT(num, den)
    s.BuildMatrices()
    with pytest.raises(RuntimeError, match="SolveKeff"):
        s.SolveGPT(num, den)
    k = s.SolveKeff()
    with pytest.raises(RuntimeError, match="SolveAdjoint"):
        s.SolveGPT(num, den)
    for call in (s.get_gamma, s.gpt_sensitivity_maps, s.get_gpt_info):
        with pytest.raises(RuntimeError, match="SolveGPT"):
            call()
    s.SolveAdjoint(True, True)
    with pytest.raises(RuntimeError, match="shaped like"):
        s.SolveGPT(num.ravel()[:-1], den)
    flux, adj = s.get_flux().copy(), s.get_flux_adj().copy()
    R = s.SolveGPT(num, den)
    gam = s.get_gamma()
    maps = s.gpt_sensitivity_maps()
    info = s.get_gpt_info()
    assert gam.shape == s.get_flux_adj().shape and set(maps) == set(GPT_MAPS)
    for w in ("D", "SigR", "NSF", "Chi", "Wa", "Wb"):
        assert maps[w].shape == s.get_D().shape, w
    assert maps["SigS"].shape == s.get_SigS().shape
    assert info["R"] == R and info["keff"] == k == s.GetLastKeff() and info["converged"] == 1
    assert np.array_equal(s.get_flux(), flux) and np.array_equal(s.get_flux_adj(), adj)
    h = make_hip(inp); h.set_linear_solver(int(ns.LinearSolverType.BICGSTAB)); h.set_tol(*tol)   # RT0-P0: the mirrors are the whole fields
    h.set_phi(flux.reshape(2, -1)); h.set_phi_adj(adj.reshape(2, -1))
    res = h.solve_gpt(wa, wb, k)
    out = h.gpt_sensitivity(k)
    assert res["R"] == R and np.array_equal(h.get_gamma().ravel(), gam.ravel())
    for key in ("wa_phi", "wb_phi", "dgamma", "ratio", "deflation", "norm", "n_outer", "cg_total", "converged"):
        assert res[key] == info[key], key
    for w in GPT_MAPS:
        assert np.array_equal(maps[w].ravel(), out[w].ravel()), w
    assert out["result"]["norm"] == info["gamma_F_phi"]
    h.close()
