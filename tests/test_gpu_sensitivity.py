"""GPU tests of the sensitivity maps (nf_sensitivity, HipSolver.sensitivity, sensitivity_maps) against the numpy yardstick of
tests/sens_exact.py: the kernels on injected fields, the boundary types, the grid-stride wrap, the skipped outputs and the state of the
handle, the first-order prediction end to end, the errors and the pybind surface."""
import ctypes as C

import numpy as np
import pytest

from helpers import degenerate_inputs, make_hip, rel_l2, synthetic_inputs
from project_exact import random_coefficients
from sens_exact import bilinear_mass, currents, flat_inputs, perturbed_block, predicted_dk, sens_maps
from subcrit_exact import ref_from_inputs
from zoom_exact import ref_unbuilt

pytestmark = pytest.mark.gpu

KEFF = 0.9
MAPS = ("D", "SigR", "NSF", "Chi", "SigS")
MASS_BAR = 1e-13          # products and sums of <= 27 terms (the zoom's load vector, the same kind of arithmetic, measures 1.6e-15)
TIGHT = (1e-12, 1e-11, 1e-11, 2000, 4000)
MIRROR = 2


def _trim(dim, n=(9, 7, 5)):
    return n[0], n[1] if dim >= 2 else 1, n[2] if dim == 3 else 1


def _field(ng, ne, nloc, seed):
    """random coefficients with positive cell means (DOF 0 in 0.5 .. 1.5), as _field of test_gpu_zoom.py: Nrm stays away from zero"""
    c = random_coefficients(ng, ne, nloc, seed=seed).reshape(ng, ne, nloc)
    c[:, :, 0] = np.random.default_rng(seed + 1000).uniform(0.5, 1.5, (ng, ne))
    return c.reshape(ng, ne * nloc)


def _with_mirrors(inp, attrs):
    out = dict(inp)
    out["bc_type"] = np.array([MIRROR if int(a) in attrs else int(t) for a, t in zip(inp["bc_attr"], inp["bc_type"])], int)
    return out


_REF = {}


def _reference(key, inp, rt, p):
    """(built RefScipy, phi, phi+, yardstick maps at k = 0.9) of one case, computed once"""
    if key not in _REF:
        r = ref_from_inputs(inp, rt, p)
        ng = int(inp["ng"])
        phi, adj = _field(ng, r.ne, r.nloc, 7 + rt), _field(ng, r.ne, r.nloc, 107 + p)
        _REF[key] = (r, phi, adj, sens_maps(r, KEFF, phi, adj))
    return _REF[key]


def _current_distance(c, r):
    """relative L2 distance between the yardstick's current of a converged flux and the existing nf_get_J of that solve (at its best
    scaling: nf_get_J reports the raw group solutions, the flux is their normalised iterate; nf_get_J's sign is -A^-1 B^T phi)"""
    c.set_tol(*TIGHT)
    c.solve_keff()
    Jg = c.get_J().ravel()
    Jy = -currents(r, c.get_phi()).ravel()
    return rel_l2(Jg, (Jg @ Jy) / (Jy @ Jy) * Jy)


def _compare(c, r, phi, adj, ref, label):
    """inject the fields, compare every map; the bar of dD is 10 x _current_distance (floor 1e-13), measured first (the solve overwrites the flux)"""
    dist = _current_distance(c, r)
    bar_d = max(10.0 * dist, 1e-13)
    c.set_phi(phi); c.set_phi_adj(adj)
    out = c.sensitivity(KEFF)
    res = out["result"]
    errs = {w: rel_l2(out[w], ref[w]) for w in MAPS}
    e_nrm = abs(res["norm"] - ref["Nrm"]) / abs(ref["Nrm"])
    print(f"sens {label}: " + " ".join(f"{w}={errs[w]:.2e}" for w in MAPS) + f" Nrm={e_nrm:.2e} | get_J vs yardstick {dist:.2e} -> dD bar {bar_d:.2e}")
    assert res["keff"] == KEFF and res["n_cells"] == r.ne
    assert e_nrm <= MASS_BAR, e_nrm
    for w in ("SigR", "SigS", "NSF", "Chi"):
        assert errs[w] <= MASS_BAR, (w, errs[w])
    assert errs["D"] <= bar_d, (errs["D"], bar_d)
    for g in range(r.ng):
        assert not out["SigS"][g, g].any()
    return errs, dist


# ---- 1. the kernels against the yardstick, injected fields ------------------------------------------------------------------------------
ORDERS = [(dim, rt, rt) for dim in (1, 2, 3) for rt in (0, 1, 2)] + [(2, 1, 0), (2, 2, 1)]


@pytest.mark.parametrize("dim,rt,p", ORDERS)
def test_maps_match_yardstick(dim, rt, p):
    """non-uniform 9 x 7 x 5 cells (trimmed per dimension), 3 groups (a down-scatter chain and one up-scatter block), every face Dirichlet,
    random phi / phi+ with positive cell means, k = 0.9"""
    nx, ny, nz = _trim(dim)
    inp = synthetic_inputs(nx, ny, nz, 3, seed=20 + dim)
    r, phi, adj, ref = _reference(("dir", dim, rt, p), inp, rt, p)
    c = make_hip(inp, rt, p)
    _compare(c, r, phi, adj, ref, f"dim={dim} RT{rt}-P{p}")
    c.close()


# ---- 2. boundaries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,rt", [(2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2)])
def test_mirror_faces_carry_no_dirichlet_term(dim, rt):
    """mirrors on attributes 1 and 4 (2D) / 1, 4 and 5 (3D): b vanishes on those faces"""
    nx, ny, nz = _trim(dim)
    attrs = (1, 4) if dim == 2 else (1, 4, 5)
    inp = _with_mirrors(synthetic_inputs(nx, ny, nz, 3, seed=20 + dim), attrs)
    r, phi, adj, ref = _reference(("mirror", dim, rt), inp, rt, rt)
    c = make_hip(inp, rt, rt)
    _compare(c, r, phi, adj, ref, f"mirrors dim={dim} RT{rt}-P{rt}")
    c.close()
    # the yardstick itself: cells that touch mirror faces only carry no boundary term, the faces left Dirichlet still contribute
    touched = np.zeros((r.nz, r.ny, r.nx), bool)
    for d in range(dim):
        for upper in (False, True):
            if r.bc.get(r._attr(d, upper)) == 0:
                idx = [slice(None)] * 3; idx[2 - d] = -1 if upper else 0
                touched[tuple(idx)] = True
    assert not ref["b"][:, ~touched.ravel()].any() and np.abs(ref["b"][:, touched.ravel()]).max() > 0


@pytest.mark.parametrize("n", [(5, 1, 3), (1, 6, 1)])
@pytest.mark.parametrize("rt", [0, 1, 2])
def test_degenerate_meshes(n, rt):
    """one cell along an axis: its lower and upper face are both Dirichlet, the lines have one cell"""
    inp = degenerate_inputs(*n)
    r, phi, adj, ref = _reference(("deg", n, rt), inp, rt, rt)
    c = make_hip(inp, rt, rt)
    _compare(c, r, phi, adj, ref, f"degenerate {n} RT{rt}-P{rt}")
    c.close()


# ---- 3. wrap and size ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rt", [((300, 1500), 0), ((40, 30), 1)])
def test_larger_grids(n, rt):
    """2D at 300 x 1500 = 450 000 cells, more than the 1024 blocks x 256 threads the launches are capped at (the grid stride wraps), and
    RT1-P1 at 40 x 30 (several blocks).  The yardstick is too slow there: m alone (dSigR, dNSF, dChi, Nrm), vectorised"""
    inp = synthetic_inputs(n[0], n[1], 1, 2, seed=31)
    c = make_hip(inp, rt, rt)
    r = ref_unbuilt(inp, rt, rt)
    phi, adj = _field(2, c.ne, c.n_loc, 3), _field(2, c.ne, c.n_loc, 4)
    c.set_phi(phi); c.set_phi_adj(adj)
    out = c.sensitivity(KEFF, which=("SigR", "NSF", "Chi"))
    assert set(out) == {"SigR", "NSF", "Chi", "result"}
    m = bilinear_mass(r, phi, adj)
    nrm = float(np.einsum("ge,he,ghe->", r.Chi, r.NSF, m))
    cc = -KEFF * KEFF / nrm
    ref = dict(SigR=cc * np.einsum("gge->ge", m), NSF=-(cc / KEFF) * np.einsum("ge,ghe->he", r.Chi, m), Chi=-(cc / KEFF) * np.einsum("he,ghe->ge", r.NSF, m))
    assert abs(out["result"]["norm"] - nrm) <= MASS_BAR * abs(nrm)
    for w in ("SigR", "NSF", "Chi"):
        assert rel_l2(out[w], ref[w]) <= MASS_BAR, (w, rel_l2(out[w], ref[w]))
    c.close()


@pytest.mark.parametrize("rt", [0, 1, 2])
def test_grid_stride_wraps_in_every_kernel(rt):
    """the 9 x 7 x 5 case of test_maps_match_yardstick with the launches held to one block (option sens_grid): 315 cells on 256 threads, so
    k_sens_norm, k_sens_mass and k_sens_current all take a second trip of their grid stride, against the full yardstick.  dD at the floor
    of its bar, 1e-13"""
    inp = synthetic_inputs(9, 7, 5, 3, seed=23)
    r, phi, adj, ref = _reference(("dir", 3, rt, rt), inp, rt, rt)
    c = make_hip(inp, rt, rt)
    c.set_option("sens_grid", 1)
    c.set_phi(phi); c.set_phi_adj(adj)
    out = c.sensitivity(KEFF)
    assert abs(out["result"]["norm"] - ref["Nrm"]) <= MASS_BAR * abs(ref["Nrm"])
    for w in MAPS:
        assert rel_l2(out[w], ref[w]) <= MASS_BAR, (w, rel_l2(out[w], ref[w]))
    c.close()


# ---- 4. skipped outputs and state ---------------------------------------------------------------------------------------------------------
def _warm(s):
    v, k = C.c_int(), C.c_double()
    s._chk(s.L.nf_get_warm_state(s.h, C.byref(v), C.byref(k)))
    return v.value, k.value


def test_skipped_outputs_and_state():
    inp = synthetic_inputs(9, 7, 1, 3, seed=41)
    c = make_hip(inp, 1, 1)
    c.set_tol(1e-8, 1e-7, 1e-7, 500, 2000)
    c.solve_keff()                                                # nf_get_J has something to report
    adj = _field(3, c.ne, c.n_loc, 5)
    c.set_phi_adj(adj)
    before = (c.get_phi().copy(), c.get_phi_adj().copy(), _warm(c), c.get_J().copy(), c.info("last_outer"), c.info("last_cg_total"))
    full = c.sensitivity(KEFF)
    again = c.sensitivity(KEFF)
    for w in MAPS:
        assert np.array_equal(full[w], again[w]), w
    assert full["result"] == again["result"]
    for left_out in MAPS:
        part = c.sensitivity(KEFF, which=tuple(w for w in MAPS if w != left_out))
        assert left_out not in part
        for w in MAPS:
            if w != left_out:
                assert np.array_equal(part[w], full[w]), (left_out, w)
        assert part["result"] == full["result"]
    only = c.sensitivity(KEFF, which=())
    assert set(only) == {"result"} and only["result"] == full["result"]
    after = (c.get_phi(), c.get_phi_adj(), _warm(c), c.get_J(), c.info("last_outer"), c.info("last_cg_total"))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert np.array_equal(before[3], after[3]) and before[4:] == after[4:]
    c.close()


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [0, 1])
def test_first_order_prediction_end_to_end(rt):
    """solve_keff, solve_adjoint, sensitivity on the 9 x 7 case; the predicted dk of +1 % SigR_1, -1 % D_0, +1 % nuSigf_1 on rows 2-4 x
    columns 3-6 against a second solve_keff on the perturbed input: within 2 % (3 x the yardstick's own first-order error)"""
    base = flat_inputs(synthetic_inputs(9, 7, 1, 2, seed=8))
    pert = perturbed_block(base)
    tol = (1e-10, 1e-9, 1e-10, 2000, 1000)
    c = make_hip(base, rt, rt); c.set_tol(*tol)
    k, n = c.solve_keff()
    ka, na = c.solve_adjoint(True, True)
    assert n < 2000 and na < 2000, (n, na)                        # both converged within max_outer
    pred = predicted_dk(c.sensitivity(k), base, pert)
    d = make_hip(pert, rt, rt); d.set_tol(*tol)
    k2, _ = d.solve_keff()
    true = k2 - k
    print(f"sens end to end RT{rt}-P{rt}: k={k:.10f} k_adj={ka:.10f} outers={n}/{na} predicted dk={pred:.6e} true dk={true:.6e} ({abs(pred / true - 1):.2%})")
    assert abs(true) > 1e-5 and abs(pred - true) <= 0.02 * abs(true), (pred, true)
    c.close(); d.close()


# ---- 6. errors and the pybind surface -----------------------------------------------------------------------------------------------------
def test_errors():
    from neutfem_amd.capi import HipSolver, HipTeam
    inp = synthetic_inputs(6, 5, 1, 2, seed=81)
    u = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    u.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    with pytest.raises(RuntimeError, match=r"error -5: .*nf_build"):
        u.sensitivity(KEFF)
    u.close()
    c = make_hip(inp)
    with pytest.raises(RuntimeError, match=r"error -5: .*no adjoint flux \(nf_solve_adjoint or nf_set_phi_adj first\)"):
        c.sensitivity(KEFF)
    c.set_phi_adj(np.ones((2, c.n_phi)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"error -1: .*keff"):
            c.sensitivity(bad)
    c.set_phi(np.zeros((2, c.n_phi)))
    with pytest.raises(RuntimeError, match=r"error -6: "):
        c.sensitivity(KEFF)                                       # Nrm = 0
    c.set_phi(np.full((2, c.n_phi), 1e308)); c.set_phi_adj(np.full((2, c.n_phi), 1e308))
    with pytest.raises(RuntimeError, match=r"error -6: "):
        c.sensitivity(KEFF)                                       # Nrm = inf
    with pytest.raises(ValueError):
        c.sensitivity(KEFF, which=("D", "Sigma"))
    c.set_phi(np.ones((2, c.n_phi))); c.set_phi_adj(np.ones((2, c.n_phi)))
    assert np.isfinite(c.sensitivity(KEFF)["D"]).all()            # the handle stays usable
    c.close()
    s3 = synthetic_inputs(4, 4, 6, 2, seed=83)
    team = HipTeam(0, 0, 2, s3["x_breaks"], s3["y_breaks"], s3["z_breaks"], [(0, 3), (3, 6)])
    team.upload_xs_global(s3["D"], s3["SigR"], s3["NSF"], s3["Chi"], s3["SigS"]); team.build()
    for s in team.slabs:
        s.set_phi_adj(np.ones((2, s.n_phi)))
        with pytest.raises(RuntimeError, match=r"error -4: "):
            s.sensitivity(KEFF)
    team.close()


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_pybind_sensitivity_maps(dim):
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    nx, ny, nz = _trim(dim, (8, 6, 4))
    inp = synthetic_inputs(nx, ny, nz, 2, seed=90 + dim, void_frac=0.0)
    s = ns.NeutFEM(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    s.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        s.set_bc(int(a), ns.BCType(int(t)), 0.0)
    s.get_D()[...] = inp["D"]; s.get_SigR()[...] = inp["SigR"]; s.get_NSF()[...] = inp["NSF"]; s.get_Chi()[...] = inp["Chi"]; s.get_SigS()[...] = inp["SigS"]
    s.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    s.set_tol(1e-10, 1e-9, 1e-9, 1000, 2000)
    with pytest.raises(RuntimeError, match="BuildMatrices"):
        s.sensitivity_maps()
    s.BuildMatrices()
    with pytest.raises(RuntimeError, match="SolveKeff"):
        s.sensitivity_maps()
    with pytest.raises(RuntimeError):
        s.get_sensitivity_info()
    k = s.SolveKeff()
    with pytest.raises(RuntimeError, match="SolveAdjoint"):
        s.sensitivity_maps()
    s.SolveAdjoint(True, True)
    flux, adj = s.get_flux().copy(), s.get_flux_adj().copy()
    maps = s.sensitivity_maps()
    assert set(maps) == set(MAPS)
    for w in ("D", "SigR", "NSF", "Chi"):
        assert maps[w].shape == s.get_D().shape, w
    assert maps["SigS"].shape == s.get_SigS().shape
    info = s.get_sensitivity_info()
    assert info["keff"] == k == s.GetLastKeff() and info["n_cells"] == nx * ny * nz and np.isfinite(info["norm"]) and info["norm"] != 0
    assert np.array_equal(s.get_flux(), flux) and np.array_equal(s.get_flux_adj(), adj)
    h = make_hip(inp)                                             # RT0-P0: the mirrors are the whole fields
    h.set_phi(flux.reshape(2, -1)); h.set_phi_adj(adj.reshape(2, -1))
    out = h.sensitivity(k)
    for w in MAPS:
        assert np.array_equal(maps[w].ravel(), out[w].ravel()), w
    assert out["result"]["norm"] == info["norm"]
    h.close()
