"""Every solve driver on every form of the CG iteration, against the driver's exact twin.

SolveKeff is checked on every form (tests/test_gpu_paths.py, test_gpu_variants.py, test_gpu_cg_forms.py).  The other drivers enter the same
cg_solve through the one group_sweep, each with its own settings and its own vectors: solve_subcritical and transient_step
with the CG start riding in k_group_rhs, the transient on a twin handle; solve_modes into a column of its block, the adjoint modes on
transposed blocks; zoom_resolved on the fine handle nf_refine makes; solve_adjoint with a plain start.  CASES is one explicit table of (driver, mesh, route,
expected form).  Every entry asserts the form before the call (apply_plan(True)["form"]; the transient: on the caller's handle, whose
options its step operator takes; the zoom: on the returned fine handle, which takes the coarse handle's), the form, the one-XCD counters
and last_direct after it (nf_info), and the numbers against the twin at the bar the driver's own test file applies at the same tolerances:

  solve_subcritical   subcrit_exact.exact_subcritical, nuSigf scaled to k = 0.85        flux 1e-8, integrals 1e-9   (test_gpu_subcritical)
  solve_modes         modes_exact.exact_modes, 3 modes + 2 guards, direct and adjoint   k 1e-8 k_0, exact residual 1e-8 (test_gpu_modes);
                      shape up to sign: residual bar / relative gap to the nearest other eigenvalue (first-order perturbation of a simple
                      eigenvalue: a residual of size r moves the vector by r / gap)
  transient_step      transient_exact.ExactTransient, 3 steps, one delayed family      flux, precursors 1e-8, scalars, power 1e-9 (test_gpu_transient)
                      one option changes between step 2 and step 3 and the form follows
  zoom_resolved       zoom_exact (the dense K0 of the fine mesh), options on the coarse handle only
                                                                                        dense: flux 1e-11; CG, stand-in (a CG solve): 1e-8;
                                                                                        integrals 10 x, source 1e-12 (test_gpu_zoom)
  solve_adjoint       the oracle's SolveAdjoint(True, True) after a fixed-work SolveKeff  equal k, equal outers, flux 1e-7 (test_gpu_void)

Meshes (helpers.synthetic_inputs, 2 groups, seed 4): M0 (12, 10, 6) RT0-P0 -- 720 unknowns per group, three blocks of the vector kernels, y
lines of one full 8-cell segment and a ragged one, z lines shorter than a segment; M1 (6, 5, 3) RT1-P1 -- 720 unknowns, bubble moments;
MT (8, 6, 12) RT0-P0 as two and three linked slabs, against the dense twin (the oracle for the adjoint) of the undivided mesh.

Every route is also compared with the classic route of the same driver and mesh (printed, not asserted: the forms differ in summation order).

Measured on an MI355X, the largest error over every route and mesh of a driver (bar); the figures enter no assertion:
  solve_subcritical   flux 6.4e-12 (1e-8), integrals 5.0e-12 (1e-9); linked slabs: flux 6.0e-12, integrals 5.6e-12
  solve_modes         k 6.5e-12 (1e-8), exact residual 8.4e-11 (1e-8), shape 3.5e-10 (3.6e-8 .. 1.0e-7); adjoint: 8.2e-12, 8.6e-11, 3.5e-10
  transient_step      flux 1.8e-11 (1e-8), precursors 3.4e-14 (1e-8), scalars and power 1.7e-11 (1e-9)
  zoom_resolved       dense: flux 2.3e-13 (1e-11), integrals 2.1e-13 (1e-10); CG and stand-in: flux 2.9e-12 (1e-8), integrals 3.2e-14 (1e-7);
                      source 3.4e-16 (1e-12)
  solve_adjoint       k 2.6e-14 (1e-9), adjoint flux 9.9e-13 (1e-7); linked slabs: 1.0e-13, 3.1e-13
  distance to the classic route, largest per driver: 4.2e-12, 5.6e-11 (adjoint modes 6.4e-11), 8.9e-12, 2.2e-12, 4.8e-12
No route misses a bar that another route of the same driver holds."""
import functools

import numpy as np
import pytest

from helpers import CG_FORMS, make_hip, rel_l2, synthetic_inputs
from modes_exact import exact_modes, iteration_matrix
from subcrit_exact import exact_subcritical, ref_from_inputs
from test_gpu_cg_forms import _prepare, _team
from test_gpu_modes import HET_K_BAR, HET_RES_BAR, HET_TOL as MODES_TOL
from test_gpu_subcritical import HET_FLUX_BAR, HET_SCALAR_BAR, HET_TOL as SUBCRIT_TOL
from test_gpu_transient import EXACT_FLUX_BAR, EXACT_SCALAR_BAR, EXACT_TOL, SCALARS, _rebuild, _scaled_sigr
from test_gpu_variants import FIXED, _set
from test_gpu_void import ADJOINT_BAR, FIXED_HI
from test_gpu_zoom import CG_BAR, CG_TOL, DENSE_BAR, DENSE_TOL, INTEGRAL_FACTOR, KEFF, SOURCE_BAR, _field
from transient_exact import TWO_GROUP_V, ExactTransient
from zoom_exact import _k0_dense, integrals, refine_inputs, zoom_source_reference

pytestmark = pytest.mark.gpu

MESHES = {"M0": ((12, 10, 6), 0), "M1": ((6, 5, 3), 1), "MT": ((8, 6, 12), 0)}
SEED = 4
ZOOM = {"M0": (2, 2, 1), "M1": (2, 1, 1)}                         # fine meshes of 2880 and 1440 unknowns per group
DIRECT_TYPE = 1                                                  # a direct linear-solver type: the explicit-S branch (inner_plan)
BETA, LAMBDA, DT = (0.0065,), (0.08,), 1e-2                      # one delayed family

# route -> (kind, options); the options that force a form on a small mesh are those of tests/test_gpu_paths.py and tests/test_gpu_cg_forms.py
NO_XCD = dict(cg_xcd=0)
ROUTES = {
    "xcd": ("cg", dict(cg_xcd=1, cg_xcd_min_cells=0, cg_xcd_max_cells=1 << 30, cg_fuse3=1)),
    "fuse3": ("cg", dict(NO_XCD, cg_fuse3=1)),
    "lean": ("cg", dict(NO_XCD, cg_fuse3=0)),
    "fused": ("cg", dict(NO_XCD, cg_fuse3=0, cg_lean=0)),
    "classic": ("cg", dict(NO_XCD, cg_fuse3=0, cg_fuse=0)),
    "dense": ("dense", {}),
    "standin": ("standin", dict(direct_max_dofs=0)),
}
LAST_DIRECT = {"cg": 0, "dense": 1, "standin": 2}
DRIVERS = ("subcritical", "modes", "modes_adjoint", "transient", "zoom", "adjoint")


def _default_form(driver, mesh):
    """what default options pick where the stand-in runs: the fine mesh of the M0 zoom (2880 unknowns) lies in the one-XCD window
    (2000 .. 28000 unknowns per group), every other mesh of the table below it"""
    return "xcd" if (driver, mesh) == ("zoom", "M0") else "fuse3"


# (driver, mesh, route, expected form): every driver on both meshes on every route; None = the dense S^-1 runs no CG
CASES = [(d, m, r, r if ROUTES[r][0] == "cg" else None if r == "dense" else _default_form(d, m)) for d in DRIVERS for m in ("M0", "M1") for r in ROUTES]

TEAM_FORMS = [("team_sr", dict(cg_single_reduce=1), 1), ("team_lean", dict(cg_single_reduce=0), 2), ("fused", dict(cg_lean=0), 2), ("classic", dict(cg_fuse=0), 2)]
SLABS = {"two": [(0, 6), (6, 12)], "three": [(0, 4), (4, 8), (8, 12)]}
# the drivers that take a linked team (solve_modes, transient_step and zoom_resolved refuse one: their own test files assert that)
TEAM_CASES = [(d, sl, f, o, red) for d in ("subcritical", "adjoint") for sl in SLABS for f, o, red in TEAM_FORMS]

# What the code cannot run, with the predicate that says so by construction.  test_not_applicable_is_refused asserts each entry; whatever
# is not here runs.  No undivided route on M0 or M1 is here: every form has its instantiation at RT0-P0 and at RT1-P1 with 4-cell segments.
NOT_APPLICABLE = {
    ("subcritical", "MT", "xcd"): "cg_plan: a linked team (!single) takes the team forms; xcd, fuse3 and lean are forms of the undivided mesh",
    ("subcritical", "MT", "fuse3"): "cg_plan: as above",
    ("subcritical", "MT", "lean"): "cg_plan: as above",
    ("subcritical", "MT", "dense"): "inner_plan: the dense S^-1 needs an undivided mesh (single); CG to 1e-14 stands in (last_direct 2)",
}


# ---- the twins: once per mesh, shared by the routes, never modified ------------------------------------------------------------------
def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _inputs(mesh):
    shape, _ = MESHES[mesh]
    return synthetic_inputs(*shape, 2, seed=SEED)


@functools.lru_cache(maxsize=None)
def _ref(mesh):
    return ref_from_inputs(_inputs(mesh), MESHES[mesh][1], MESHES[mesh][1])


@functools.lru_cache(maxsize=None)
def _twin_modes(mesh, adjoint):
    """four leading eigenpairs (three asked for, the fourth for the gap of the third), the dense A for the residuals, the shape bars"""
    r = _ref(mesh)
    k, phi = exact_modes(r, 4, adjoint)
    A = iteration_matrix(r, adjoint)
    gap = [min(abs(k[i] - k[j]) for j in range(4) if j != i) / abs(k[i]) for i in range(3)]
    _freeze(k, phi, A)
    return dict(k=k, phi=phi, A=A, shape_bar=[HET_RES_BAR / g for g in gap])


def _critical(mesh):
    """(k, phi) of the fundamental mode, phi (ng, n_phi) with a positive sum"""
    t = _twin_modes(mesh, False)
    phi = t["phi"][:, 0] * np.sign(t["phi"][:, 0].sum())
    return float(t["k"][0]), phi.reshape(2, -1)


def _k_power(r):
    """the dominant eigenvalue of the dense iteration matrix by the power method (MT: 2304 unknowns, no full eigen-decomposition)"""
    A = iteration_matrix(r)
    x = np.ones(A.shape[0]); k = 0.0
    for _ in range(5000):
        y = A @ x
        k_new = np.linalg.norm(y) / np.linalg.norm(x)
        x = y / np.linalg.norm(y)
        if abs(k_new - k) <= 1e-13 * k_new:
            break
        k = k_new
    return float(k_new)


@functools.lru_cache(maxsize=None)
def _twin_subcritical(mesh):
    inp, rt = _inputs(mesh), MESHES[mesh][1]
    k = _critical(mesh)[0] if mesh != "MT" else _k_power(_ref(mesh))
    nsf = inp["NSF"] * (0.85 / k)
    ne = inp["D"][0].size
    src = np.zeros((2, ne)); src[0] = np.random.default_rng(7).uniform(0.5, 2.0, ne); src[0, ::5] = 0.0
    ex = exact_subcritical(ref_from_inputs(inp, rt, rt, NSF=nsf), src)
    _freeze(nsf, src, ex["phi"])
    return dict(inp=dict(inp, NSF=nsf), src=src, ex=ex)


@functools.lru_cache(maxsize=None)
def _twin_transient(mesh):
    inp, rt = _inputs(mesh), MESHES[mesh][1]
    k, phi = _critical(mesh)
    ex = ExactTransient(inp, rt, rt, TWO_GROUP_V, BETA, LAMBDA, k, phi)
    up = dict(inp, SigR=_scaled_sigr(inp, 1, 0.97))
    ex.set_xs(SigR=up["SigR"])
    steps = ex.step(DT, 3)
    for st in steps:
        _freeze(st["phi"], st["c"])
    return dict(k=k, phi=phi, up=up, steps=steps)


@functools.lru_cache(maxsize=None)
def _twin_zoom(mesh):
    """the frozen source by quadrature and one dense solve of the fine mesh's K0 (zoom_exact.exact_zoom's steps; its own solve turns to
    Gauss-Seidel sweeps above 4000 unknowns, and the dense route's bar is 1e-11)"""
    inp, rt = _inputs(mesh), MESHES[mesh][1]
    rc = _ref(mesh)
    rf = ref_from_inputs(refine_inputs(inp, ZOOM[mesh]), rt, rt)
    coef = _field(2, rc.ne, rc.nloc, 9)
    q = zoom_source_reference(rc, rf, coef, KEFF, ZOOM[mesh], False)
    phi = np.linalg.solve(_k0_dense(rf, False), q.ravel()).reshape(2, -1)
    _freeze(coef, q, phi)
    return dict(coef=coef, q=q, phi=phi, **integrals(rf, q, phi))


def _oracle(inp, rt, solver_type):
    from oracle.oracle import OracleNeutFEM
    o = OracleNeutFEM(rt, rt, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    o.set_linear_solver(solver_type)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        o.set_bc(int(a), int(t), 0.0)
    o.get_D()[...] = inp["D"]; o.get_SigR()[...] = inp["SigR"]; o.get_NSF()[...] = inp["NSF"]; o.get_Chi()[...] = inp["Chi"]; o.get_SigS()[...] = inp["SigS"]
    o.BuildMatrices()
    return o


def _adjoint_tol(mesh):
    return FIXED if MESHES[mesh][1] == 0 else FIXED_HI


@functools.lru_cache(maxsize=None)
def _twin_adjoint(mesh, direct):
    """the oracle's SolveAdjoint(True, True) after its fixed-work SolveKeff, with the CG (type 6) or with a direct type"""
    o = _oracle(_inputs(mesh), MESHES[mesh][1], DIRECT_TYPE if direct else 6)
    o.set_tol(*_adjoint_tol(mesh))
    ko = o.SolveKeff(); ka = o.SolveAdjoint(True, True)
    adj = o.phi_adj_dofs().copy()
    _freeze(adj)
    return dict(ko=ko, ka=ka, n=o.info("last_outer"), adj=adj)


# ---- one case --------------------------------------------------------------------------------------------------------------------------
ERRORS = {}                                                       # (driver, quantity) -> largest error / bar seen in this process (printed per case)


def _bar(label, what, err, bar):
    """print, remember, assert"""
    key = (label.split()[0], what)
    ERRORS[key] = max(ERRORS.get(key, 0.0), float(err))
    print(f"{label}: {what} {err:.3e} (bar {bar:.1e})")
    assert err <= bar, (label, what, err, bar)


def _new(mesh, route, inp=None):
    rt = MESHES[mesh][1]
    s = make_hip(inp or _inputs(mesh), rt, rt)
    kind, opts = ROUTES[route]
    if kind != "cg":
        s.set_linear_solver(DIRECT_TYPE)
    _set(s, opts)
    return s


def _planned(s, form, label):
    plan = s.apply_plan(True)["form"]
    assert form is None or plan == form, (label, plan, form)


def _reported(s, route, form, label, xcd_before=0):
    """after the call: the form that ran, the one-XCD counters, the group solver's route"""
    kind = ROUTES[route][0]
    assert s.info("last_direct") == LAST_DIRECT[kind], (label, s.info("last_direct"))
    if form is None:
        return
    assert CG_FORMS[s.info("cg_form")] == form, (label, CG_FORMS[s.info("cg_form")], form)
    assert s.info("last_xcd") == int(form == "xcd") and s.info("xcd_refused") == 0, (label, s.info("last_xcd"), s.info("xcd_refused"))
    assert (s.info("xcd_solves") > xcd_before) == (form == "xcd"), (label, s.info("xcd_solves"), xcd_before)
    if kind == "standin":
        assert s.info("direct_standin_unconverged") == 0, label


def _run_subcritical(mesh, route, form, label, team=None):
    tw = _twin_subcritical(mesh)
    if team is None:
        s = _new(mesh, route, tw["inp"])
        s.set_tol(*SUBCRIT_TOL); s.upload_source(tw["src"])
        _planned(s, form, label)
        res = s.solve_subcritical()
        _reported(s, route, form, label)
        phi = s.get_phi()
        s.close()
    else:
        res = team.solve_subcritical()
        phi = team.get_phi_local().reshape(2, -1)
    ex = tw["ex"]
    assert res["converged"] == 1, label
    _bar(label, "flux", rel_l2(phi, ex["phi"]), HET_FLUX_BAR)
    for key in ("M", "k_source", "phi_int", "phi_int_nofission", "production", "source"):
        _bar(label, key, abs(res[key] - ex[key]) / abs(ex[key]), HET_SCALAR_BAR)
    return phi


def _run_modes(mesh, route, form, label, adjoint):
    tw = _twin_modes(mesh, adjoint)
    s = _new(mesh, route)
    s.set_tol(*MODES_TOL)
    _planned(s, form, label)
    res = s.solve_modes(3, n_guard=2, adjoint=adjoint)
    _reported(s, route, form, label)
    modes = [s.get_mode(i, adjoint).ravel() for i in range(3)]
    s.close()
    assert res["converged"] == 1 and res["n_modes"] == 3 and res["n_block"] == 5, (label, res)
    for i, phi in enumerate(modes):
        k = res["k"][i]
        _bar(label, f"k[{i}]", abs(k - tw["k"][i]) / tw["k"][0], HET_K_BAR)
        _bar(label, f"residual[{i}]", np.linalg.norm(tw["A"] @ phi - k * phi) / np.linalg.norm(k * phi), HET_RES_BAR)   # modes_exact.mode_residual with the twin's A
        _bar(label, f"shape[{i}]", min(rel_l2(phi, tw["phi"][:, i]), rel_l2(-phi, tw["phi"][:, i])), tw["shape_bar"][i])
    return np.concatenate([m * np.sign(m @ tw["phi"][:, i]) for i, m in enumerate(modes)])


# the option that changes between step 2 and step 3 of the transient, and what the third step must then run: (options, route, form)
def _switch(mesh, route):
    if route == "classic":
        return dict(cg_fuse=1), "lean", "lean"
    if route == "dense":
        return dict(direct_max_dofs=0), "standin", _default_form("transient", mesh)
    if route == "standin":
        return dict(cg_fuse3=0), "standin", "lean"
    return dict(cg_fuse=0), "classic", "classic"


def _run_transient(mesh, route, form, label):
    tw = _twin_transient(mesh)
    s = _new(mesh, route)
    s.set_tol(*EXACT_TOL)
    s.set_phi(tw["phi"]); s.transient_begin(TWO_GROUP_V, BETA, LAMBDA, tw["k"])
    _rebuild(s, tw["up"])
    for i, st in enumerate(tw["steps"]):
        if i == 2:
            opts, route, form = _switch(mesh, route)
            _set(s, opts)
        _planned(s, form, label)                                  # the caller's handle plans like the step operator it hands its options to
        xcd0 = s.info("xcd_solves")
        res, power = s.transient_step(DT, 1)
        _reported(s, route, form, f"{label} step {i + 1}", xcd0)
        assert res["n_unconverged"] == 0 and res["n_steps"] == i + 1, (label, res)
        _bar(label, "flux", rel_l2(s.get_phi(), st["phi"]), EXACT_FLUX_BAR)
        _bar(label, "precursors", rel_l2(s.get_precursors(0), st["c"][0]), EXACT_FLUX_BAR)
        for key in SCALARS:
            _bar(label, key, abs(res[key] - st[key]) / abs(st[key]), EXACT_SCALAR_BAR)
        _bar(label, "power[]", abs(power[0] - st["power"]) / st["power"], EXACT_SCALAR_BAR)
        if i == 1:
            phi2 = s.get_phi().copy()
    assert s.info("transient_rebuilds") == 1                      # the options reach the kept step operator: no rebuild for them
    s.close()
    return phi2                                                   # the flux after step 2: still on the route of the case


def _run_zoom(mesh, route, form, label):
    tw = _twin_zoom(mesh)
    kind = ROUTES[route][0]
    tol, bar = (DENSE_TOL, DENSE_BAR) if kind == "dense" else (CG_TOL, CG_BAR)   # the stand-in is a CG solve: the CG route's bar
    c = _new(mesh, route)                                         # the options go to the coarse handle only
    c.set_tol(*tol)
    c.set_phi(tw["coef"])
    f, res = c.zoom_resolved(ZOOM[mesh], KEFF)
    _planned(f, form, label)                                      # the fine handle reports its own plan and its own solve
    _reported(f, route, form, label)
    assert c.info("xcd_solves") == 0, label
    phi = f.get_phi()
    f.close(); c.close()
    assert res["converged"] == 1 and res["n_cells"] == tw["n_cells"], (label, res)
    _bar(label, "flux", rel_l2(phi, tw["phi"]), bar)
    _bar(label, "source", abs(res["source"] - tw["source"]) / np.abs(tw["q"]).sum(), SOURCE_BAR)
    for key in ("phi_int", "production"):
        _bar(label, key, abs(res[key] - tw[key]) / abs(tw[key]), INTEGRAL_FACTOR * bar)
    return phi


def _run_adjoint(mesh, route, form, label, team=None):
    tw = _twin_adjoint(mesh, team is None and ROUTES[route][0] != "cg")
    tol = _adjoint_tol(mesh)
    if team is None:
        s = _new(mesh, route)
        s.set_tol(*tol)
        _planned(s, form, label)
        ks, _ = s.solve_keff()
        xcd0 = s.info("xcd_solves")
        ka, n = s.solve_adjoint(True, True)
        _reported(s, route, form, label, xcd0)
        adj = s.get_phi_adj()
        s.close()
    else:
        ks, _ = team.solve_keff()
        ka, n = team.solve_adjoint(True, True)
        adj = team.get_phi_adj_local().reshape(2, -1)
    assert tw["ka"] == tw["ko"] and ka == ks, (label, ka, ks)
    assert n == tw["n"] == tol[3], (label, n, tw["n"])
    _bar(label, "k", abs(ks - tw["ko"]) / tw["ko"], 1e-9)       # the k both sides fix: the fixed-work bar of tests/test_gpu_variants.py
    _bar(label, "adjoint-flux", rel_l2(adj, tw["adj"]), ADJOINT_BAR)
    return adj


RUN = {"subcritical": _run_subcritical, "modes": lambda *a: _run_modes(*a, adjoint=False), "modes_adjoint": lambda *a: _run_modes(*a, adjoint=True),
       "transient": _run_transient, "zoom": _run_zoom, "adjoint": _run_adjoint}


@functools.lru_cache(maxsize=None)
def _classic(driver, mesh):
    """the fixed-work reference point: the classic route of the driver on the mesh, run once"""
    out = RUN[driver](mesh, "classic", "classic", f"{driver} {mesh} classic (reference point)")
    _freeze(out)
    return out


@pytest.mark.parametrize("driver,mesh,route,form", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_driver_on_form(driver, mesh, route, form):
    assert (driver, mesh, route) not in NOT_APPLICABLE
    label = f"{driver} {mesh} {route} [{form or 'dense S^-1'}]"
    out = RUN[driver](mesh, route, form, label)
    print(f"{label}: distance to the classic route {rel_l2(out, _classic(driver, mesh)):.3e} (printed only)")


# ---- linked teams ----------------------------------------------------------------------------------------------------------------------
def _make_team(driver, slabs, opts, direct=False):
    inp = _twin_subcritical("MT")["inp"] if driver == "subcritical" else _inputs("MT")
    t = _team(inp, SLABS[slabs], 0, opts)
    if direct:
        t.set_linear_solver(DIRECT_TYPE)
    t.set_tol(*(SUBCRIT_TOL if driver == "subcritical" else FIXED))
    if driver == "subcritical":
        t.upload_source(_twin_subcritical("MT")["src"].reshape(2, 12, 6, 8))
    _prepare(t)
    return t


@pytest.mark.parametrize("driver,slabs,form,opts,reductions", TEAM_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in TEAM_CASES])
def test_team_driver_on_form(driver, slabs, form, opts, reductions):
    label = f"{driver} MT-{slabs} [{form}]"
    t = _make_team(driver, slabs, opts)
    for x in t.slabs:
        assert x.apply_plan(True)["form"] == form, (label, x.apply_plan(True)["form"])
    (_run_subcritical if driver == "subcritical" else _run_adjoint)("MT", None, form, label, team=t)
    h = t.head
    assert CG_FORMS[h.info("cg_form")] == form and h.info("cg_reductions") == reductions and h.info("vec_reduce") == 0, (label, h.info("cg_form"), h.info("cg_reductions"))
    assert h.info("last_direct") == 0 and h.info("xcd_solves") == 0 and h.info("last_xcd") == 0, label
    t.close()


def test_not_applicable_is_refused():
    """every entry of NOT_APPLICABLE: the plan never names the form there, or the solve takes the other group solver"""
    seen = set()
    for (driver, mesh, route), why in NOT_APPLICABLE.items():
        assert driver == "subcritical" and mesh == "MT", (driver, mesh)      # no undivided route is exempt
        kind, opts = ROUTES[route]
        for slabs in SLABS:
            t = _make_team(driver, slabs, opts, direct=kind != "cg")
            plans = {x.apply_plan(True)["form"] for x in t.slabs}
            if kind == "cg":
                assert plans == {"team_sr"}, (route, plans, why)      # the options that force the form on an undivided mesh leave the team on its own
            else:
                t.set_tol(*(SUBCRIT_TOL[:3] + (2,) + SUBCRIT_TOL[4:]))      # two outers: which group solver ran shows after the first
                t.solve_subcritical()
                assert t.head.info("last_direct") == 2 and CG_FORMS[t.head.info("cg_form")] in plans, (route, t.head.info("last_direct"), why)
            print(f"{driver} {mesh}-{slabs} {route}: planned {sorted(plans)}, last_direct {t.head.info('last_direct')} -- {why}")
            t.close()
        seen.add(route)
    assert seen == {"xcd", "fuse3", "lean", "dense"}


# ---- default options: the twins run what they ran before they took options ------------------------------------------------------------
EXPLICIT_DEFAULTS = dict(cg_xcd=1, cg_fuse3=1, cg_lean=1, cg_fuse=1, cg_batch=0, host_pub=1, cg_single_reduce=-1, direct_max_dofs=6000, xcd=-1, s_long=-1, line_dict=-1,
                         c_early=-1, nt_loads=1, split_dot=1, s_tx=0, s_seg=0)


def test_default_options_change_nothing():
    """a handle nobody set an option on against one with the defaults spelled out: transient steps with bit-equal flux and equal CG
    counts, zoom re-solves with bit-equal fine flux"""
    tw, tz = _twin_transient("M0"), _twin_zoom("M0")
    out = []
    for opts in ({}, EXPLICIT_DEFAULTS):
        s = make_hip(_inputs("M0"))
        _set(s, opts)
        s.set_tol(*EXACT_TOL)
        s.set_phi(tw["phi"]); s.transient_begin(TWO_GROUP_V, BETA, LAMBDA, tw["k"])
        _rebuild(s, tw["up"])
        res, power = s.transient_step(DT, 2)
        tr = (s.get_phi().copy(), res["cg_total"], res["n_outer"], CG_FORMS[s.info("cg_form")])
        s.set_tol(*CG_TOL); s.set_phi(tz["coef"])
        f, zres = s.zoom_resolved(ZOOM["M0"], KEFF)
        out.append(tr + (f.get_phi().copy(), zres["cg_total"], CG_FORMS[f.info("cg_form")]))
        f.close(); s.close()
    a, b = out
    print(f"default options: transient form {a[3]}, cg_total {a[1]}; zoom form {a[6]}, cg_total {a[5]}")
    assert np.array_equal(a[0], b[0]) and a[1:4] == b[1:4]
    assert np.array_equal(a[4], b[4]) and a[5:] == b[5:]
    assert a[3] == "fuse3" and a[6] == "xcd"                       # what the sizes pick: 720 unknowns below the one-XCD window, 2880 inside it
