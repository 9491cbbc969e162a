"""The group sweep after a fixed number of outers, against its fixed-work twin (tests/sweep_exact.py).

A converged solve cannot tell a Gauss-Seidel sweep from one that reads the old iterate, runs the groups backwards or takes the transposed
blocks by mistake where those still converge: the fixed point is the same.  Two outers per phase of solve_subcritical can: three groups with
scatter blocks above and below the diagonal (sweep_exact.three_group_inputs), max_outer = 2, every group solver of the sweep (dense S^-1,
CG to 1e-14 standing in, the diagonal S^-1 fused into k_group_rhs, and the stand-in on two linked slabs), flux and integrals against the
twin at the bars tests/test_gpu_subcritical.py applies at these tolerances.

The CPU test states the condition that keeps the GPU tests from passing vacuously: on both undivided meshes each wrong variant of the twin
(jacobi, descending, transposed) lies at least 1000 x the flux bar away from the right one after each phase.  Measured (n_outer = 2): jacobi
and descending 2.3e-3 / 1.9e-3 (RT0-P0) and 6.8e-4 / 3.8e-4 (RT1-P1) -- the two coincide, as they must under k_group_rhs's g' < g rule --
and transposed 3e-2 to 5e-2.

Measured on an MI355X, the largest error over the routes of a mesh (bar); the figures enter no assertion:
  RT0-P0 (6, 5, 3)      flux 1.7e-15 (1e-8), integrals 4.1e-16 (1e-9); the diagonal path: flux 1.1e-16, integrals 1.4e-16
  RT1-P1 (4, 3, 2)      flux 4.4e-15 (1e-8), integrals 3.5e-15 (1e-9)
  two linked slabs      flux 1.6e-15 (1e-8), integrals 3.8e-16 (1e-9)
The eight tests take 1.5 s together."""
import functools

import numpy as np
import pytest

from helpers import make_hip, rel_l2
from subcrit_exact import ref_from_inputs
from sweep_exact import fixed_work_subcritical, integrals, three_group_inputs
from test_gpu_driver_forms import DIRECT_TYPE, LAST_DIRECT, ROUTES
from test_gpu_subcritical import HET_FLUX_BAR, HET_SCALAR_BAR, HET_TOL

N_OUTER = 2
TOL = HET_TOL[:3] + (N_OUTER,) + HET_TOL[4:]
MESHES = {"RT0": ((6, 5, 3), 0), "RT1": ((4, 3, 2), 1), "SLAB": ((6, 5, 6), 0)}
SLAB_PLANES = [(0, 3), (3, 6)]


# ---- the twins: once per mesh, shared by the routes, never modified ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(mesh):
    return three_group_inputs(*MESHES[mesh][0])


@functools.lru_cache(maxsize=None)
def _ref(mesh):
    return ref_from_inputs(_inputs(mesh), MESHES[mesh][1], MESHES[mesh][1])


@functools.lru_cache(maxsize=None)
def _source(mesh):
    src = np.random.default_rng(3).uniform(0.5, 1.5, (3, _ref(mesh).ne))
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def _twin(mesh, **wrong):
    out = fixed_work_subcritical(_ref(mesh), _source(mesh), N_OUTER, **wrong)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("mesh", ["RT0", "RT1"])
def test_twin_tells_the_wrong_sweeps_apart(mesh):
    """each wrong variant is at least 1000 x the flux bar away from the right sweep after each phase: the GPU tests below cannot pass on a
    sweep that is Jacobi, runs backwards or takes the transposed blocks"""
    right = _twin(mesh)
    for wrong in ("jacobi", "descending", "transposed"):
        for phase, (a, b) in enumerate(zip(_twin(mesh, **{wrong: True}), right)):
            d = rel_l2(a, b)
            print(f"{mesh} {wrong} phase {phase}: {d:.3e} from the Gauss-Seidel sweep")
            assert d >= 1000 * HET_FLUX_BAR, (mesh, wrong, phase, d)
    assert np.array_equal(_twin(mesh, jacobi=True)[1], _twin(mesh, descending=True)[1])


# ---- the GPU against the twin --------------------------------------------------------------------------------------------------------
def _check(label, res, phi, r, twin, last_direct, want_direct):
    assert res["n_outer"] == res["n_outer_nofission"] == N_OUTER, (label, res)
    assert res["converged"] == 0, (label, res)
    assert last_direct == want_direct, (label, last_direct)
    e = rel_l2(phi, twin[1])
    print(f"{label}: flux {e:.3e} (bar {HET_FLUX_BAR:.1e})")
    assert e <= HET_FLUX_BAR, (label, e)
    (phi0_int, _), (phi_int, production) = integrals(r, twin[0]), integrals(r, twin[1])
    for key, ex in (("phi_int", phi_int), ("phi_int_nofission", phi0_int), ("production", production)):
        e = abs(res[key] - ex) / abs(ex)
        print(f"{label}: {key} {e:.3e} (bar {HET_SCALAR_BAR:.1e})")
        assert e <= HET_SCALAR_BAR, (label, key, res[key], ex)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,route", [("RT0", "dense"), ("RT0", "standin"), ("RT0", "diag"), ("RT1", "dense"), ("RT1", "standin")])
def test_two_outers_match_the_twin(mesh, route):
    rt = MESHES[mesh][1]
    s = make_hip(_inputs(mesh), rt, rt)
    if route == "diag":
        want = 1                                                  # 90 unknowns < 200: inner_plan's explicit-S branch, dense S^-1 (unused by the diagonal path)
    else:
        kind, opts = ROUTES[route]
        s.set_linear_solver(DIRECT_TYPE)
        for k, v in opts.items():
            s.set_option(k, v)
        want = LAST_DIRECT[kind]
    s.set_tol(*TOL); s.upload_source(_source(mesh))
    res = s.solve_subcritical(use_diag=route == "diag")
    if route == "diag":
        twin = fixed_work_subcritical(_ref(mesh), _source(mesh), N_OUTER, sinv=[s.diagonal_cache(g) for g in range(3)])
    else:
        twin = _twin(mesh)
    phi, last_direct = s.get_phi(), s.info("last_direct")
    s.close()
    _check(f"{mesh} {route}", res, phi, _ref(mesh), twin, last_direct, want)


@pytest.mark.gpu
def test_two_outers_on_linked_slabs_match_the_twin():
    """two linked slabs of three planes each, the stand-in (a slab team has no dense S^-1), against the twin of the undivided mesh"""
    from neutfem_amd.capi import HipTeam
    inp = _inputs("SLAB")
    t = HipTeam(0, 0, 3, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], SLAB_PLANES)
    t.set_linear_solver(DIRECT_TYPE)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); t.build()
    for k, v in ROUTES["standin"][1].items():
        t.head.set_option(k, v)
    t.set_tol(*TOL); t.upload_source(_source("SLAB").reshape(3, 6, 5, 6))
    res = t.solve_subcritical()
    phi, last_direct = t.get_phi_local().reshape(3, -1), t.head.info("last_direct")
    t.close()
    _check("SLAB standin", res, phi, _ref("SLAB"), _twin("SLAB"), last_direct, LAST_DIRECT["standin"])
