"""GPU tests of the zoom (nf_refine, nf_zoom_source, nf_get_source, nf_set_phi_adj, nf_zoom_resolved, zoom_resolved)
against the numpy yardstick of tests/zoom_exact.py: the load vector against the quadrature restriction, the refined twin against a solver
built from the refined inputs, the re-solve against the exact solve of the same system, the refine-1 identity, the physics on IAEA-2D,
the state of the coarse handle, the errors and the pybind surface."""
import ctypes as C

import numpy as np
import pytest

from helpers import load_inputs, make_hip, rel_l2, synthetic_inputs
from project_exact import random_coefficients
from subcrit_exact import ref_from_inputs
from zoom_exact import exact_zoom, ref_unbuilt, refine_inputs, solve_k0, zoom_source_reference

pytestmark = pytest.mark.gpu

KEFF = 0.9
# test_resolve_matches_exact: (tolerances, flux bar) of the dense-S^-1 route and of the CG route; the integrals at INTEGRAL_FACTOR x the flux bar,
# the source total at SOURCE_BAR of sum |q| (tests/test_gpu_driver_forms.py imports them)
DENSE_TOL, DENSE_BAR = (1e-14, 1e-13, 1e-13, 500, 1000), 1e-11
CG_TOL, CG_BAR = (1e-12, 1e-11, 1e-11, 2000, 4000), 1e-8
INTEGRAL_FACTOR, SOURCE_BAR = 10, 1e-12


def _trim(dim, n=(9, 7, 5)):
    return n[0], n[1] if dim >= 2 else 1, n[2] if dim == 3 else 1


def _r(dim, refine):
    return tuple(f if a < dim else 1 for a, f in enumerate(refine))


def _field(ng, ne, nloc, seed):
    """random coefficients with positive cell means (DOF 0 in 0.5 .. 1.5): the integrals the stop rule divides by stay away from zero"""
    c = random_coefficients(ng, ne, nloc, seed=seed).reshape(ng, ne, nloc)
    c[:, :, 0] = np.random.default_rng(seed + 1000).uniform(0.5, 1.5, (ng, ne))
    return c.reshape(ng, ne * nloc)


def _best_scaled_error(v, truth):
    v, truth = np.asarray(v).ravel(), np.asarray(truth).ravel()
    return rel_l2((v @ truth) / (v @ v) * v, truth)


# ---- 1. the source kernel against the quadrature restriction ---------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_source_matches_quadrature(dim, rt):
    """non-uniform 9 x 7 x 5 cells (trimmed per dimension), refine (3, 2, 2): NX = 27 odd, the scalar tail; (2, 1, 3): NX = 18 even, the
    16-byte stores, one factor 1, asymmetric by 3.  Random phi / phi+ and k = 0.9, direct and adjoint: relative L2 <= 1e-13"""
    nx, ny, nz = _trim(dim)
    inp = synthetic_inputs(nx, ny, nz, 2, seed=20 + dim)
    c = make_hip(inp, rt, rt)
    rc = ref_unbuilt(inp, rt, rt)
    phi = random_coefficients(2, c.ne, c.n_loc, seed=dim * 10 + rt)
    adj = random_coefficients(2, c.ne, c.n_loc, seed=dim * 10 + rt + 100)
    c.set_phi(phi); c.set_phi_adj(adj)
    assert np.array_equal(c.get_phi_adj(), adj)
    for refine in ((3, 2, 2), (2, 1, 3)):
        r = _r(dim, refine)
        f = c.refine(*r)
        assert (f.nx, f.ny, f.nz) == (nx * r[0], ny * r[1], nz * r[2]) and f.n_loc == c.n_loc
        rf = ref_unbuilt(refine_inputs(inp, r), rt, rt)
        for adjoint, field in ((False, phi), (True, adj)):
            c.zoom_source(f, KEFF, adjoint=adjoint)
            q = f.get_source()
            ref = zoom_source_reference(rc, rf, field, KEFF, r, adjoint)
            err = rel_l2(q, ref)
            print(f"zoom source dim={dim} rt={rt} refine={r} adjoint={adjoint}: rel_l2={err:.3e}")
            assert err <= 1e-13, (r, adjoint, err)
        f.close()
    c.close()


@pytest.mark.parametrize("n,rt", [((40, 30), 1), ((300, 1500), 1)])
def test_source_larger_grids(n, rt):
    """2D refined (3, 2) at 40 x 30 cells (several blocks), and refined (3, 1) at 300 x 1500: 1500 rows x 450 pairs = 675 000 work items,
    more than the 8 x 256 CUs x 256 threads the launch is capped at, so the grid stride wraps (rows and pairs both advance)"""
    refine = (3, 2, 1) if n[0] == 40 else (3, 1, 1)
    inp = synthetic_inputs(n[0], n[1], 1, 2, seed=31)
    c = make_hip(inp, rt, rt)
    phi = random_coefficients(2, c.ne, c.n_loc, seed=3)
    c.set_phi(phi)
    f = c.refine(*refine)
    c.zoom_source(f, KEFF)
    ref = zoom_source_reference(ref_unbuilt(inp, rt, rt), ref_unbuilt(refine_inputs(inp, refine), rt, rt), phi, KEFF, refine)
    assert rel_l2(f.get_source(), ref) <= 1e-13
    f.close(); c.close()


# ---- 2. refine (1, 1, 1): the source is the fission term ------------------------------------------------------------------------------
def test_refine_one_source_is_the_fission_term():
    """RT1-P1 in 2D against chi / k sum Mf phi of a built RefScipy, entry by entry to 1e-14 relative (a positive field: no cancellation
    in the sum over the groups, so a few ulps of the products is all that separates the two)"""
    inp = synthetic_inputs(9, 7, 1, 2, seed=8)
    c = make_hip(inp, 1, 1)
    r = ref_from_inputs(inp, 1, 1)
    phi = np.random.default_rng(4).uniform(0.5, 1.5, (2, c.n_phi))
    c.set_phi(phi)
    f = c.refine(1, 1)
    c.zoom_source(f, KEFF)
    q = f.get_source()
    tf = (r.Mf * phi).sum(axis=0)
    ref = np.repeat(r.Chi, r.nloc, axis=1) * tf[None, :] / KEFF
    assert np.all(np.abs(q - ref) <= 1e-14 * np.abs(ref)), np.max(np.abs(q - ref) / np.maximum(np.abs(ref), 1e-300))
    f.close(); c.close()


# ---- 3. nf_refine ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,rt,refine", [(1, 2, (3, 1, 1)), (2, 1, (2, 3, 1)), (3, 0, (2, 1, 3)), (3, 1, (1, 2, 2))])
def test_refine_matches_a_solver_built_from_refined_inputs(dim, rt, refine):
    nx, ny, nz = _trim(dim, (6, 5, 4))
    inp = synthetic_inputs(nx, ny, nz, 2, seed=40 + dim, dirichlet=(1, 3, 6))       # some faces Dirichlet, the others natural
    c = make_hip(inp, rt, rt)
    f = c.refine(*refine)
    d = make_hip(refine_inputs(inp, refine), rt, rt)
    for key in ("dim", "nx", "ny", "nz", "ne", "ng", "n_phi", "n_J", "n_loc", "rt_order", "p_order"):
        assert f.info(key) == d.info(key), key
    x = np.random.default_rng(1).standard_normal(d.n_phi)
    for g in range(2):
        assert rel_l2(f.schur_apply(g, x), d.schur_apply(g, x)) <= 1e-13
    # boundary types carry over: with every face natural the operator differs
    n = make_hip(dict(refine_inputs(inp, refine), bc_attr=np.array([], int), bc_type=np.array([], int)), rt, rt)
    assert rel_l2(n.schur_apply(0, x), d.schur_apply(0, x)) > 1e-6
    f.close(); d.close(); n.close(); c.close()


# ---- 4. the re-solve against the exact solve -----------------------------------------------------------------------------------------
CASES = [  # dim, cells, refine, rt, ng
    (1, (5, 1, 1), (3, 1, 1), 1, 2),
    (2, (4, 3, 1), (2, 3, 1), 1, 2),
    (3, (3, 2, 2), (2, 2, 2), 0, 2),
    (3, (3, 2, 2), (2, 2, 2), 1, 2),
    (3, (2, 2, 2), (2, 1, 2), 2, 2),
    (2, (4, 3, 1), (2, 3, 1), 1, 3),     # three groups: the up-scatter block
]


@pytest.mark.parametrize("route", ["dense", "cg"])
@pytest.mark.parametrize("dim,n,refine,rt,ng", CASES)
def test_resolve_matches_exact(dim, n, refine, rt, ng, route):
    """random phi, k = 0.9; the dense-S^-1 route at 1e-11 and the CG route at 1e-8 (the bars of test_gpu_subcritical)"""
    inp = synthetic_inputs(n[0], n[1], n[2], ng, seed=50 + dim + rt, void_frac=0.0)
    c = make_hip(inp, rt, rt)
    if route == "dense":
        c.solver_pushed = 0
        c.set_tol(*DENSE_TOL); bar = DENSE_BAR
    else:
        c.set_tol(*CG_TOL); bar = CG_BAR
    phi = _field(ng, c.ne, c.n_loc, 9)
    c.set_phi(phi)
    ex = exact_zoom(inp, rt, rt, phi, KEFF, refine)
    f, res = c.zoom_resolved(refine, KEFF)
    err = rel_l2(f.get_phi(), ex["phi"])
    print(f"zoom resolve dim={dim} rt={rt} ng={ng} {route}: rel_l2={err:.3e} outers={res['n_outer']} cg={res['cg_total']}")
    assert err <= bar, err
    direct = route == "dense" or f.n_phi < 200                     # below 200 unknowns per group every solver type is the explicit-S branch
    assert f.info("last_direct") == (1 if direct else 0) and res["converged"] == 1 and res["n_cells"] == ex["n_cells"]
    assert abs(res["source"] - ex["source"]) <= SOURCE_BAR * np.abs(ex["q"]).sum()
    for key in ("phi_int", "production"):
        assert abs(res[key] - ex[key]) <= INTEGRAL_FACTOR * bar * abs(ex[key]), (key, res[key], ex[key])
    assert f.get_J().shape == (ng, f.n_J) and f.project_flux((1, 1, 1)).size == ng * f.ne     # the fine handle is a full handle
    f.close(); c.close()


def test_resolve_adjoint_matches_exact():
    inp = synthetic_inputs(4, 3, 1, 3, seed=61, void_frac=0.0)
    c = make_hip(inp, 1, 1)
    c.solver_pushed = 0
    c.set_tol(1e-14, 1e-13, 1e-13, 500, 1000)
    adj = _field(3, c.ne, c.n_loc, 10)
    phi0 = c.get_phi().copy()
    c.set_phi_adj(adj)
    ex = exact_zoom(inp, 1, 1, adj, KEFF, (2, 3, 1), adjoint=True)
    f, res = c.zoom_resolved((2, 3), KEFF, adjoint=True)
    assert rel_l2(f.get_source(), ex["q"]) <= 1e-13
    assert rel_l2(f.get_phi(), ex["phi"]) <= 1e-11, rel_l2(f.get_phi(), ex["phi"])
    assert abs(res["phi_int"] - ex["phi_int"]) <= 1e-10 * abs(ex["phi_int"])
    # the transposed blocks matter here: the direct operator on the same source gives another flux
    assert rel_l2(solve_k0(ex["rf"], ex["q"], adjoint=False), ex["phi"]) > 1e-6
    assert np.array_equal(c.get_phi(), phi0)
    f.close(); c.close()


# ---- 5. the one-XCD CG range ------------------------------------------------------------------------------------------------------------
def test_resolve_one_xcd_cg():
    """26 x 20 refined (2, 2): 2080 unknowns per group, CG pushed -> every group solve is one launch on one XCD"""
    inp = synthetic_inputs(26, 20, 1, 2, seed=70)
    c = make_hip(inp)
    c.set_tol(1e-12, 1e-11, 1e-11, 2000, 4000)
    phi = _field(2, c.ne, 1, 11)
    c.set_phi(phi)
    ex = exact_zoom(inp, 0, 0, phi, KEFF, (2, 2, 1))
    f, res = c.zoom_resolved((2, 2), KEFF)
    err = rel_l2(f.get_phi(), ex["phi"])
    print(f"zoom one-XCD: rel_l2={err:.3e} outers={res['n_outer']} cg={res['cg_total']} xcd_solves={f.info('xcd_solves')}")
    assert err <= 1e-8, err
    assert f.info("xcd_solves") > 0 and f.info("xcd_refused") == 0 and c.info("xcd_solves") == 0
    f.close(); c.close()


# ---- 6. identity on IAEA-2D -------------------------------------------------------------------------------------------------------------
def test_identity_on_iaea2d():
    """a converged (phi, k) zoomed by (1, 1, 1) comes back: the bar is twice what the yardstick's exact solve of the same source leaves
    (the coarse solve's own stop error, not the zoom's), plus 1e-8 for the zoom's iteration"""
    inp = load_inputs("iaea2d")
    c = make_hip(inp)
    c.set_tol(1e-12, 1e-11, 1e-11, 2000, 4000)
    k, _ = c.solve_keff()
    phi = c.get_phi().copy()
    ex = exact_zoom(inp, 0, 0, phi, k, (1, 1, 1))
    f, res = c.zoom_resolved((1, 1), k)
    zoom_err, exact_err = rel_l2(f.get_phi(), phi), rel_l2(ex["phi"], phi)
    print(f"zoom identity IAEA-2D: zoom={zoom_err:.3e} exact={exact_err:.3e} outers={res['n_outer']}")
    assert zoom_err <= 2 * exact_err + 1e-8, (zoom_err, exact_err)
    f.close(); c.close()


# ---- 7. physics, RT0-P0 -----------------------------------------------------------------------------------------------------------------
def test_zoom_beats_projection_on_iaea2d():
    """IAEA-2D subsampled to 19 x 19 (the 38 x 38 input is its (2, 2) injection), zoomed (2, 2), against the eigen-solve on 38 x 38:
    cell means at their best scaling.  The reference alone gives 3.13e-2 (zoom) and 9.05e-2 (projection)"""
    fine_inp = load_inputs("iaea2d")
    inp = dict(fine_inp, x_breaks=fine_inp["x_breaks"][::2], y_breaks=fine_inp["y_breaks"][::2])
    for key in ("D", "SigR", "NSF", "Chi", "SigS"):
        inp[key] = np.ascontiguousarray(fine_inp[key][..., ::2, ::2])
    inj = refine_inputs(inp, (2, 2))
    for key in ("D", "SigR", "NSF", "Chi", "SigS"):
        assert np.array_equal(inj[key], fine_inp[key]), key
    assert np.allclose(inj["x_breaks"], fine_inp["x_breaks"], rtol=0, atol=1e-12) and np.allclose(inj["y_breaks"], fine_inp["y_breaks"], rtol=0, atol=1e-12)
    tol = (1e-10, 1e-9, 1e-9, 2000, 4000)
    c = make_hip(inp); c.set_tol(*tol)
    k, _ = c.solve_keff()
    t = make_hip(fine_inp); t.set_tol(*tol)
    t.solve_keff()
    truth = t.get_phi()
    f, res = c.zoom_resolved((2, 2), k)
    e_zoom = _best_scaled_error(f.get_phi(), truth)
    e_proj = _best_scaled_error(c.project_flux((2, 2)), truth)
    print(f"zoom physics IAEA-2D 19x19 -> 38x38: zoom={e_zoom:.4e} projection={e_proj:.4e} outers={res['n_outer']} cg={res['cg_total']}")
    assert e_zoom <= 0.5 * e_proj and e_zoom <= 4e-2, (e_zoom, e_proj)
    f.close(); t.close(); c.close()


# ---- 8. state and errors ----------------------------------------------------------------------------------------------------------------
def _warm(s):
    v, k = C.c_int(), C.c_double()
    s._chk(s.L.nf_get_warm_state(s.h, C.byref(v), C.byref(k)))
    return v.value, k.value


def test_coarse_handle_is_untouched_and_zoom_is_linear():
    inp = synthetic_inputs(8, 6, 1, 2, seed=80, void_frac=0.0)
    c = make_hip(inp, 1, 1)
    c.set_tol(1e-8, 1e-7, 1e-7, 500, 2000)
    k, n = c.solve_keff()
    before = (c.get_phi().copy(), _warm(c), c.history(), c.progress(), c.info("last_outer"), c.info("last_cg_total"), c.info("last_path"))
    c.solver_pushed = 0
    c.set_tol(1e-14, 1e-13, 1e-13, 500, 1000)
    f, _ = c.zoom_resolved((2, 3), k)
    f.close()
    after = (c.get_phi(), _warm(c), c.history(), c.progress(), c.info("last_outer"), c.info("last_cg_total"), c.info("last_path"))
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and before[3:] == after[3:]
    for key in ("k", "dk", "dphi", "cg"):
        assert np.array_equal(before[2][key], after[2][key]), key
    a, b = _field(2, c.ne, c.n_loc, 1), _field(2, c.ne, c.n_loc, 2)
    out = []
    for field in (a, b, a + 2.0 * b):
        c.set_phi(field)
        f, _ = c.zoom_resolved((2, 3), KEFF)
        out.append(f.get_phi().copy()); f.close()
    assert rel_l2(out[2], out[0] + 2.0 * out[1]) <= 1e-10
    c.close()


def test_errors():
    from neutfem_amd.capi import HipSolver
    inp = synthetic_inputs(6, 5, 1, 2, seed=81)
    c = make_hip(inp)
    c.set_phi(np.zeros((2, c.n_phi)))
    with pytest.raises(RuntimeError, match=r"error -1: .*zero"):
        c.zoom_resolved((2, 2), KEFF)
    c.set_phi(np.ones((2, c.n_phi)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"error -1: .*keff"):
            c.zoom_resolved((2, 2), bad)
    with pytest.raises(RuntimeError, match=r"error -1: "):
        c.zoom_resolved((2, 2), KEFF, use_cmfd=True)
    with pytest.raises(RuntimeError, match=r"error -1: "):
        c.zoom_resolved((2, 2), KEFF, use_diag=True)
    with pytest.raises(RuntimeError, match=r"error -1: .*refine factor"):
        c.zoom_resolved((2, 2, 2), KEFF)                          # no z axis
    with pytest.raises(RuntimeError, match=r"error -5: "):
        c.get_source()
    other = make_hip(synthetic_inputs(13, 10, 1, 2, seed=82))     # 13 is no multiple of 6
    with pytest.raises(RuntimeError, match=r"error -1: .*not a refinement"):
        c.zoom_source(other, KEFF)
    p1 = make_hip(refine_inputs(inp, (2, 2)), 1, 1)                # the right mesh, another order
    with pytest.raises(RuntimeError, match=r"error -1: .*not a refinement"):
        c.zoom_source(p1, KEFF)
    c.set_phi(np.full((2, c.n_phi), 1e308))
    f = c.refine(2, 2)
    with pytest.raises(RuntimeError, match=r"error -6: .*not finite"):
        c.zoom_source(f, 1e-3)
    c.set_phi(np.ones((2, c.n_phi)))
    c.zoom_source(f, KEFF)                                        # the handles stay usable
    assert np.isfinite(f.get_source()).all()
    f.close(); p1.close(); other.close(); c.close()
    s3 = synthetic_inputs(4, 4, 6, 2, seed=83)
    slab = HipSolver(0, 0, 2, s3["x_breaks"], s3["y_breaks"], s3["z_breaks"], 0, False, True)
    slab.upload_xs(s3["D"], s3["SigR"], s3["NSF"], s3["Chi"], s3["SigS"]); slab.build()
    with pytest.raises(RuntimeError, match=r"error -4: "):
        slab.zoom_resolved((2, 2, 2), KEFF)
    with pytest.raises(RuntimeError, match=r"error -4: "):
        slab.refine(2, 2, 2)
    slab.close()


# ---- 9. the pybind surface --------------------------------------------------------------------------------------------------------------
def test_pybind_zoom_resolved():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    inp = synthetic_inputs(8, 6, 1, 2, seed=90, void_frac=0.0)
    s = ns.NeutFEM(1, 1, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    s.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        s.set_bc(int(a), ns.BCType(int(t)), 0.0)
    s.get_D()[...] = inp["D"]; s.get_SigR()[...] = inp["SigR"]; s.get_NSF()[...] = inp["NSF"]; s.get_Chi()[...] = inp["Chi"]; s.get_SigS()[...] = inp["SigS"]
    s.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    s.set_tol(1e-10, 1e-9, 1e-9, 1000, 2000)
    s.BuildMatrices()
    errors = []
    for call in (lambda: s.zoom_resolved([2, 2]), lambda: s.zoom_resolved([2, 2], adjoint=True), lambda: s.get_zoom_info()):
        with pytest.raises(RuntimeError) as ei:
            call()
        errors.append(str(ei.value))
    assert "SolveKeff" in errors[0] and "SolveAdjoint" in errors[1]
    k = s.SolveKeff()
    flux = s.get_flux().copy()
    z = s.zoom_resolved([2, 2])
    assert z.shape == (2, 12, 16)
    info = s.get_zoom_info()
    assert info["converged"] == 1 and info["n_cells"] == 192 and info["n_outer"] >= 2
    h = make_hip(inp, 1, 1)
    h.set_tol(1e-10, 1e-9, 1e-9, 1000, 2000)
    kh, _ = h.solve_keff()
    assert abs(kh - k) <= 1e-12 * k
    f, res = h.zoom_resolved((2, 2), kh)
    assert rel_l2(z, f.get_phi().reshape(2, -1, f.n_loc)[:, :, 0]) <= 1e-9
    assert abs(info["phi_int"] - res["phi_int"]) <= 1e-9 * abs(res["phi_int"])
    f.close(); h.close()
    assert np.array_equal(s.get_flux(), flux) and s.GetLastKeff() == k
    with pytest.raises(RuntimeError) as ei:
        s.zoom_resolved([2, 2, 2, 2], adjoint=True)               # still no adjoint solve
    errors.append(str(ei.value))
    s.SolveAdjoint(True, True)
    adj = s.get_flux_adj().copy()
    za = s.zoom_resolved([2, 1], adjoint=True)
    assert za.shape == (2, 6, 16) and np.isfinite(za).all() and np.abs(za).max() > 0
    assert np.array_equal(s.get_flux(), flux) and np.array_equal(s.get_flux_adj(), adj) and s.GetLastKeff() == k
    assert s.zoom_resolved([0, -3]).shape == (2, 6, 8)            # clamped like project_flux clamps
    assert all("outside the accelerated hot path" not in e for e in errors)
