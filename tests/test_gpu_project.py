"""GPU tests of the sub-cell projection (nf_project_flux / nf_project_power, pybind project_flux / project_power) against the
quadrature yardstick of tests/project_exact.py: exactness for every order and dimension, conservation, P0 replication, the power
sum, the adjoint field, the value of the reconstruction against a solve on the refined mesh, slab teams, pybind shapes, errors and
a 256^3 run."""
import ctypes as C

import numpy as np
import pytest

from helpers import load_inputs, make_hip, rel_l2, synthetic_inputs
from project_exact import coarse_means, dof0, power_reference, project_reference, random_coefficients

pytestmark = pytest.mark.gpu

NF_ERR_ARG, NF_ERR_STATE = -1, -5
ORDERS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
MESH = {1: (7, 1, 1), 2: (5, 4, 1), 3: (5, 3, 4)}
REFINE = {1: [(1, 1, 1), (2, 1, 1), (3, 1, 1)], 2: [(1, 1, 1), (2, 3, 1), (3, 2, 1)], 3: [(1, 1, 1), (2, 3, 1), (3, 2, 4)]}


def _full(a, s):
    """a projected field trimmed by dimension -> (..., NZ, NY, NX)"""
    lead = a.shape[:a.ndim - s.dim]
    return a.reshape(lead + (1,) * (3 - s.dim) + a.shape[a.ndim - s.dim:])


@pytest.mark.parametrize("rt,p", ORDERS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_exact_conservative_and_power(dim, rt, p):
    nx, ny, nz = MESH[dim]
    inp = synthetic_inputs(nx, ny, nz, 2, seed=dim + 3 * rt + p)
    s = make_hip(inp, rt, p)
    nloc = s.n_loc
    c = random_coefficients(2, s.ne, nloc, seed=100 + dim)
    s.set_phi(c)
    ksf = np.random.default_rng(5).uniform(0.1, 2.0, (2, s.ne))
    for r in REFINE[dim]:
        f = _full(s.project_flux(r), s)
        ref = project_reference(c, dim, p, nx, ny, nz, r)
        assert f.shape == ref.shape
        assert rel_l2(f, ref) <= 1e-13, (r, rel_l2(f, ref))
        cm = coarse_means(f, nx, ny, nz, r)
        np.testing.assert_allclose(cm, dof0(c, nloc), rtol=1e-13, atol=1e-13 * np.abs(c).max())
        if r == (1, 1, 1):
            assert np.array_equal(f.reshape(2, -1), dof0(c, nloc))
        if p == 0:
            rep = np.repeat(np.repeat(np.repeat(c.reshape(2, nz, ny, nx), r[2], 1), r[1], 2), r[0], 3)
            assert np.array_equal(f, rep)
        assert np.array_equal(_full(s.project_flux(r, group=1), s), f[1])
        pw = _full(s.project_power(ksf, r), s)
        assert rel_l2(pw, power_reference(f, ksf, nx, ny, nz, r)) <= 1e-14
    assert np.array_equal(s.get_phi(), c)                         # the handle's flux is untouched
    s.close()


def test_adjoint_field():
    inp = synthetic_inputs(6, 5, 1, 2, seed=4)
    s = make_hip(inp, 1, 1)
    r = (2, 3, 1)
    ones = np.ones((2, s.ne * s.n_loc))
    a0 = s.project_flux(r, adjoint=True)
    assert rel_l2(a0, project_reference(ones, 2, 1, 6, 5, 1, r)[:, 0]) <= 1e-13
    s.set_tol(1e-9, 1e-8, 1e-8, 500, 2000)
    s.solve_keff()
    s.solve_adjoint()
    adj = s.get_phi_adj()
    a1 = s.project_flux(r, adjoint=True)
    assert rel_l2(a1, project_reference(adj, 2, 1, 6, 5, 1, r)[:, 0]) <= 1e-13
    assert rel_l2(a1, s.project_flux(r)) > 1e-3                  # not the direct flux
    ksf = np.random.default_rng(1).uniform(0.5, 1.5, (2, s.ne))
    assert rel_l2(s.project_power(ksf, r, adjoint=True), power_reference(a1[:, None], ksf, 6, 5, 1, r)[0]) <= 1e-14
    s.close()


def _refined_inputs(inp, f=2):
    out = dict(inp)
    for key in ("x_breaks", "y_breaks"):
        b = inp[key]
        out[key] = np.concatenate([np.linspace(b[i], b[i + 1], f + 1)[:-1] for i in range(len(b) - 1)] + [b[-1:]])
    for key in ("D", "SigR", "NSF", "Chi", "SigS"):
        out[key] = np.repeat(np.repeat(inp[key], f, axis=-1), f, axis=-2)
    return out


def test_reconstruction_beats_replication():
    """IAEA-2D at RT2-P2: the projection of the coarse solution is closer to the cell means of a solve on the mesh refined by 2
    (same materials and BCs) than the plain replication of the coarse cell means"""
    inp = load_inputs("iaea2d")
    tol = (1e-9, 1e-8, 1e-8, 1000, 4000)
    s = make_hip(inp, 2, 2); s.set_tol(*tol)
    kc, _ = s.solve_keff()
    fine = make_hip(_refined_inputs(inp), 2, 2); fine.set_tol(*tol)
    kf, _ = fine.solve_keff()
    ny, nx = inp["D"].shape[1:]
    truth = dof0(fine.get_phi(), 9).reshape(2, 2 * ny, 2 * nx)
    proj = s.project_flux((2, 2, 1))
    c0 = dof0(s.get_phi(), 9).reshape(2, ny, nx)
    rep = np.repeat(np.repeat(c0, 2, axis=1), 2, axis=2)
    norm = lambda a: a / a.sum()                                  # equal fine cells: the same total on every field
    e_proj, e_rep = rel_l2(norm(proj), norm(truth)), rel_l2(norm(rep), norm(truth))
    assert e_proj < e_rep, f"projection {e_proj:.3e} vs replication {e_rep:.3e} (k coarse {kc:.7f}, fine {kf:.7f})"
    s.close(); fine.close()


@pytest.mark.parametrize("nslabs", [2, 4])
def test_slabs_concatenate_to_the_undivided_mesh(nslabs):
    from neutfem_amd.capi import HipTeam
    nx, ny, nz, rt, p = 5, 4, 16, 1, 1
    inp = synthetic_inputs(nx, ny, nz, 2, seed=8)
    u = make_hip(inp, rt, p)
    step = nz // nslabs
    planes = [(k, k + step) for k in range(0, nz, step)]
    t = HipTeam(rt, p, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], planes)
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    t.build()
    c = random_coefficients(2, u.ne, u.n_loc, seed=9).reshape(2, nz, ny * nx * u.n_loc)
    ksf = np.random.default_rng(2).uniform(0.1, 1.0, (2, nz, ny * nx))
    u.set_phi(c)
    for sl, (k0, k1) in zip(t.slabs, planes):
        sl.set_phi(np.ascontiguousarray(c[:, k0:k1]))
    r = (2, 3, 2)
    fu, pu = u.project_flux(r), u.project_power(ksf, r)
    ft = np.concatenate([sl.project_flux(r) for sl in t.slabs], axis=1)
    pt = np.concatenate([sl.project_power(np.ascontiguousarray(ksf[:, k0:k1]), r) for sl, (k0, k1) in zip(t.slabs, planes)], axis=0)
    assert ft.shape == fu.shape and np.array_equal(ft, fu)
    assert pt.shape == pu.shape and np.array_equal(pt, pu)
    t.close(); u.close()


def _pybind(rt, p, dim, ng=2):
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as m
    inp = synthetic_inputs(*MESH[dim], ng, seed=12)
    s = m.NeutFEM(rt, p, ng, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    s.set_verbosity(m.VerbosityLevel.SILENT)
    s.set_linear_solver(m.LinearSolverType.BICGSTAB)
    for a in inp["bc_attr"]:
        s.set_bc(int(a), m.BCType.DIRICHLET, 0.0)
    for name in ("D", "SigR", "NSF", "Chi"):
        getattr(s, "get_" + name)()[...] = inp[name]
    s.get_SigS()[...] = inp["SigS"]
    s.get_KSF()[...] = np.random.default_rng(3).uniform(0.5, 1.5, inp["D"].shape)
    s.set_tol(1e-8, 1e-7, 1e-7, 500, 2000)
    s.BuildMatrices()
    return m, s, inp


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_pybind_shapes_and_refine_rules(dim):
    m, s, inp = _pybind(1, 1, dim)
    s.SolveKeff()
    nx, ny, nz = MESH[dim]
    full = (nz, ny, nx)[3 - dim:]
    f1 = s.project_flux([])
    assert f1.shape == (2,) + full and np.array_equal(f1, s.get_flux())
    assert np.array_equal(s.project_flux([1, 1, 1]), f1) and np.array_equal(s.project_flux([0, -3, 0]), f1)
    f = s.project_flux([2, 3, 2])
    r = (2, 3 if dim >= 2 else 1, 2 if dim == 3 else 1)          # ry ignored in 1D, rz below 3D (SolveCoarse's rule)
    want = (nz * r[2], ny * r[1], nx * r[0])[3 - dim:]
    assert f.shape == (2,) + want
    f3 = f.reshape((2, nz * r[2], ny * r[1], nx * r[0]))
    np.testing.assert_allclose(coarse_means(f3, nx, ny, nz, r), s.get_flux().reshape(2, -1), rtol=1e-12, atol=1e-12 * np.abs(f).max())
    pw = s.project_power([2, 3, 2])
    assert pw.shape == want
    assert rel_l2(pw, power_reference(f3, np.asarray(s.get_KSF()).reshape(2, -1), nx, ny, nz, r).reshape(want)) <= 1e-14
    k_before = s.GetLastKeff()
    assert np.array_equal(s.project_flux([2, 3, 2]), f) and s.GetLastKeff() == k_before


def test_pybind_p0_view_edit_and_adjoint():
    m, s, inp = _pybind(0, 0, 2)
    s.SolveKeff()
    v = s.get_flux()
    v[0, 1, 2] = 7.5                                              # P0: get_flux() is a writable view of the flux
    f = s.project_flux([2, 2])
    assert (f[0, 2:4, 4:6] == 7.5).all()
    assert (s.project_flux([3, 1], adjoint=True) == 1.0).all()   # no adjoint solve yet: all ones
    s.SolveAdjoint()
    a = s.project_flux([1, 1], adjoint=True)
    assert np.array_equal(a, s.get_flux_adj())
    assert np.array_equal(s.project_flux([2, 2]), f)              # the adjoint call gave the device flux back
    s.reset_flux()
    assert (s.project_flux([2, 2], adjoint=True) == 1.0).all()


def test_errors_leave_the_handle_usable():
    from neutfem_amd.capi import HipSolver
    inp = synthetic_inputs(6, 5, 1, 2, seed=6)
    raw = HipSolver(1, 1, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    raw.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    buf = raw.vector(raw.ne * 16)
    ksf = np.ones(2 * raw.ne)
    kp = ksf.ctypes.data_as(C.POINTER(C.c_double))
    assert raw.L.nf_project_flux(raw.h, 1, 1, 1, 0, 0, buf.ptr) == NF_ERR_STATE      # before nf_build
    assert raw.L.nf_project_power(raw.h, 1, 1, 1, 0, kp, buf.ptr) == NF_ERR_STATE
    buf.free(); raw.close()
    s = make_hip(inp, 1, 1)
    s.set_tol(1e-9, 1e-8, 1e-8, 500, 2000)
    k0, _ = s.solve_keff()
    phi0 = s.get_phi()
    buf = s.vector(s.ne * 16 * 2)
    L, h = s.L, s.h
    assert L.nf_project_flux(h, 2, 2, 1, 0, 2, buf.ptr) == NF_ERR_ARG                 # g = ng
    assert L.nf_project_flux(h, 2, 2, 1, 0, -2, buf.ptr) == NF_ERR_ARG
    assert L.nf_project_flux(h, 0, 2, 1, 0, 0, buf.ptr) == NF_ERR_ARG                 # factor < 1
    assert L.nf_project_flux(h, 2, 2, 2, 0, 0, buf.ptr) == NF_ERR_ARG                 # rz on a 2D mesh
    bad = ksf.copy(); bad[7] = np.nan
    assert L.nf_project_power(h, 2, 2, 1, 0, bad.ctypes.data_as(C.POINTER(C.c_double)), buf.ptr) == NF_ERR_ARG
    bad[7] = np.inf
    assert L.nf_project_power(h, 2, 2, 1, 0, bad.ctypes.data_as(C.POINTER(C.c_double)), buf.ptr) == NF_ERR_ARG
    assert L.nf_project_flux(h, 2, 2, 1, 0, -1, buf.ptr) == 0
    buf.free()
    assert np.array_equal(s.get_phi(), phi0)
    s.reset_flux()
    k1, _ = s.solve_keff()
    assert abs(k1 - k0) <= 1e-8 * k0
    s.close()


def test_size_256cube():
    """256^3 RT0-P0, 2 groups, refine (2, 2, 2) into a device buffer, one group at a time: a fixed-seed sample of fine cells is the
    coarse value (P0), and every coarse cell's sub-cell mean is its value"""
    from neutfem_amd.capi import HipSolver
    n, ng, N = 256, 2, 256 ** 3
    b = np.linspace(0.0, 256.0, n + 1)
    s = HipSolver(0, 0, ng, b, b, b)
    one = np.ones(ng * N)
    s.upload_xs(one, one * 0.05, one * 0.02, np.concatenate([np.ones(N), np.zeros(N)]), np.zeros(ng * ng * N))
    del one
    s.build()
    c = np.random.default_rng(21).uniform(0.5, 2.0, (ng, N))
    s.set_phi(c)
    NE = N * 8
    buf = s.vector(NE)
    pick = np.random.default_rng(22).integers(0, NE, 20000)
    for g in range(ng):
        s._chk(s.L.nf_project_flux(s.h, 2, 2, 2, 0, g, buf.ptr))
        f = buf.download()
        Z, rem = np.divmod(pick, 512 * 512); Y, X = np.divmod(rem, 512)
        e = ((Z // 2) * n + Y // 2) * n + X // 2
        assert np.array_equal(f[pick], c[g, e])
        cm = coarse_means(f.reshape(512, 512, 512), n, n, n, (2, 2, 2))
        assert np.abs(cm - c[g]).max() <= 1e-13 * 2.0
        del f, cm
    buf.free()
    s.close()
