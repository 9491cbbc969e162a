"""A Schur apply depends on its arguments alone: whatever ran before on the same handle -- a CG solve in any of its forms (fused, lean,
split dot product, chunked pass, single reduction), a timed apply, the current reconstruction -- leaves nothing behind that a later
apply could pick up.  The smallest shapes that still have at least four planes per slab, more than one tile row and three directions."""
import numpy as np
import pytest

from helpers import make_hip, synthetic_inputs
from neutfem_amd.capi import HipTeam

pytestmark = pytest.mark.gpu

LAUNCH_PATH = dict(resident=0, cg_fuse3=0)                        # the launch path with the fused + lean CG, not the one-launch solves


def fixed_outers(n):
    return (0.0, 1e-10, 1e-10, n, 2000)                           # exactly n outers, inner solves converged


def make_team(inp, counts, **opts):
    """slabs of counts[i] planes each, built as tests/test_gpu_slabs.py builds them"""
    edges = np.concatenate([[0], np.cumsum(counts)])
    t = HipTeam(0, 0, int(inp["ng"]), inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], list(zip(edges[:-1], edges[1:])))
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    t.build()
    for s in t.slabs:
        for key, value in opts.items():
            s.set_option(key, value)
    return t


@pytest.mark.parametrize("opts", [{}, dict(cg_lean=0), dict(cg_fuse=0),
                                  dict(split_dot=2, cg_lean=0, nt_min_cells=0),       # the z.w route
                                  dict(s_long=1, split_dot=1, cg_lean=0)],            # the chunked route
                         ids=["lean", "fused", "plain", "zw", "chunked"])
def test_undivided_apply_is_independent_of_earlier_solves(opts):
    inp = synthetic_inputs(12, 10, 9, 2, seed=5)
    s = make_hip(inp)
    for key, value in {**LAUNCH_PATH, **opts}.items():
        s.set_option(key, value)
    rng = np.random.default_rng(7)
    x, rhs = rng.standard_normal(s.n_phi), rng.standard_normal(s.n_phi)
    y0 = s.schur_apply(0, x)
    s.solve_group(0, rhs, 1e-10, 200)
    s.set_tol(*fixed_outers(3)); _, n = s.solve_keff()
    assert n == 3
    s.time_schur_apply(0, 2)
    y1 = s.schur_apply(0, x)
    assert np.isfinite(y0).all() and np.array_equal(y0, y1)
    s.close()


@pytest.mark.parametrize("counts", [[6, 6], [4, 4, 4]], ids=["2slabs", "3slabs"])
@pytest.mark.parametrize("single", [1, 0], ids=["one_reduction", "two_reductions"])
def test_team_apply_is_independent_of_solves_and_current_reconstruction(counts, single):
    inp = synthetic_inputs(10, 8, 12, 2, seed=5)
    t = make_team(inp, counts, cg_single_reduce=single, **(dict(endpoint_weights=1) if single else {}))
    x = np.random.default_rng(7).standard_normal((12, 8, 10))
    y0 = t.schur_apply(0, x)
    t.set_tol(*fixed_outers(3)); _, n = t.solve_keff()
    assert n == 3 and t.head.info("cg_reductions") == (1 if single else 2)
    y1 = t.schur_apply(0, x)
    t.get_J_local()                                               # the emit pass of the z lines: an endpoint phase outside CG
    y2 = t.schur_apply(0, x)
    assert np.isfinite(y0).all() and np.array_equal(y0, y1) and np.array_equal(y0, y2)
    t.close()


def test_team_apply_with_y_pass_beside_x_pass_has_the_same_bits():
    """xy_overlap = 1 (the default, which slabs of this size take): the y pass on a stream of its own into a vector of its own,
    added by the accumulation pass -- the same bits as the passes one after the other, before and after a solve"""
    inp = synthetic_inputs(10, 8, 12, 2, seed=5)
    x = np.random.default_rng(7).standard_normal((12, 8, 10))
    res = []
    for xy in (1, 0):
        t = make_team(inp, [6, 6], xy_overlap=xy)
        y0 = t.schur_apply(0, x)
        t.set_tol(*fixed_outers(3)); _, n = t.solve_keff()
        y1 = t.schur_apply(0, x)
        assert n == 3 and np.array_equal(y0, y1)
        res.append(y0)
        t.close()
    assert np.isfinite(res[0]).all() and np.array_equal(res[0], res[1])


def test_higher_order_apply_is_independent_of_earlier_solves():
    """RT1-P1 (bubble moments, nb > 0), undivided"""
    inp = synthetic_inputs(10, 8, 6, 2, seed=5)
    s = make_hip(inp, 1, 1)
    for key, value in LAUNCH_PATH.items():
        s.set_option(key, value)
    x = np.random.default_rng(7).standard_normal(s.n_phi)
    y0 = s.schur_apply(0, x)
    s.set_tol(*fixed_outers(2)); _, n = s.solve_keff()
    assert n == 2
    y1 = s.schur_apply(0, x)
    assert np.isfinite(y0).all() and np.array_equal(y0, y1)
    s.close()
