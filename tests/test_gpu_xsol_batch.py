"""Batched x_sol update of the fused CG (option xsol_batch = M; CgFuse and nf_xsol_ring.h): the x pass writes each new direction into the
next slot of a ring of M buffers and touches x_sol in every M-th iteration only, applying the M deferred updates oldest first; k_cg_flush
applies what is pending when the solve ends.  Same fma chain per cell, so everything is compared BIT FOR BIT with a handle that runs
xsol_batch = 1 -- after the launch-plan report has confirmed that the solve runs the fused form with the M under test.

Meshes (RT0-P0): the shapes at which the x pass changes code path -- (256, 4, 4) two chunks per lane, the benchmark's instantiation;
(130, 8, 16) second chunk partial; (40, 6, 5) several lines per wave; (520, 3, 2) eight chunks per lane -- each with and without the table
of distinct lines.  One case also goes against the oracle's CG at the bar of tests/test_gpu_variants.py, so that the two handles cannot be
wrong together."""
import functools

import numpy as np
import pytest

from helpers import make_hip
from neutfem_amd.capi import HipSolver
from test_gpu_line_dict import block_inputs
from test_gpu_variants import A, CLASSIC, R, _inputs, _ref_cg, _set, _solves

pytestmark = pytest.mark.gpu

FUSED = dict(CLASSIC, cg_lean=0)                                  # as tests/test_gpu_cg_forms.py forces the form
MESHES = [(256, 4, 4), (130, 8, 16), (40, 6, 5), (520, 3, 2)]
# material blocks per mesh: a direction takes its table when at most a quarter of its lines are distinct
BLOCKS = {(256, 4, 4): (25, 2, 2), (130, 8, 16): (13, 2, 4), (40, 6, 5): (4, 3, 5), (520, 3, 2): (52, 3, 2)}
TABLES = [dict(), dict(line_dict=1, nt_min_cells=0)]
BATCHES = [2, 4, 8]
FIXED3 = (0.0, 1e-11, 1e-11, 3, 3000)                             # exactly 3 outers, inner CG converged


@functools.lru_cache(maxsize=None)
def _blocks(shape):
    """piecewise-constant cross-sections on a uniform mesh: x lines repeat, so the table of distinct lines engages where it is asked for"""
    return block_inputs(shape, BLOCKS[shape])


def _handle(shape, M, extra=None, conditioned=True, rt=0, blocks=False):
    s = make_hip(_blocks(shape) if blocks else _inputs(shape, 2, conditioned), rt, rt)
    _set(s, dict(FUSED, xsol_batch=M, **(extra or {})))
    return s


def _planned(s, M, dict_on=None):
    plan = s.apply_plan(True)
    assert plan["form"] == "fused" and plan["xsol_batch"] == M, plan
    if dict_on is not None:
        assert plan["x"]["dict"] == int(dict_on), plan
    return plan


@functools.lru_cache(maxsize=None)
def _rhs(shape):
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(11)
    b = [np.abs(rng.standard_normal(n)) for _ in range(2)]
    for a in b:
        a.setflags(write=False)
    return b


@pytest.mark.parametrize("M", BATCHES)
@pytest.mark.parametrize("tab", TABLES, ids=["plain", "table"])
@pytest.mark.parametrize("shape", MESHES, ids=["x".join(map(str, m)) for m in MESHES])
def test_every_final_count_and_reuse_bit_equal(shape, tab, M):
    new, old = _handle(shape, M, tab, blocks=True), _handle(shape, 1, tab, blocks=True)
    _planned(new, M, bool(tab)); _planned(old, 1, bool(tab))
    b = _rhs(shape)
    # tol 0: the solve ends at maxit, so the final count takes every residue modulo M, and a multiple more
    for maxit in range(1, 2 * M + 3):
        for batch in (1, 3):                                      # host checks inside a ring period
            new.set_option("cg_batch", batch); old.set_option("cg_batch", batch)
            xn, nn, _ = new.solve_group(0, b[0], 0.0, maxit)
            xo, no, _ = old.solve_group(0, b[0], 0.0, maxit)
            assert nn == no == maxit, (maxit, batch, nn, no)
            assert np.array_equal(xn, xo), (maxit, batch, float(np.abs(xn - xo).max()))
    # converged, two groups in turn on one handle, twice: the ring is reused across groups and solves
    for batch in (0, 1, 3):
        new.set_option("cg_batch", batch); old.set_option("cg_batch", batch)
        for rep in range(2):
            for g in range(2):
                xn, nn, rn = new.solve_group(g, b[g], 1e-10, 5000)
                xo, no, ro = old.solve_group(g, b[g], 1e-10, 5000)
                assert nn == no and nn > 2 * M and rn == ro and rn < 1e-10, (batch, rep, g, nn, no, rn, ro)
                assert np.array_equal(xn, xo), (batch, rep, g, float(np.abs(xn - xo).max()))
    new.close(); old.close()


@pytest.mark.parametrize("M", BATCHES)
def test_against_the_oracle(M):
    (shape, rt) = A
    s = _handle(shape, M)
    _planned(s, M)
    _solves(s, _ref_cg(shape, rt), f"xsol_batch {M}")               # equal iteration counts, rel_l2 < 1e-10
    s.close()


@pytest.mark.parametrize("M", BATCHES)
def test_fixed_work_keff_bit_equal(M):
    shape = A[0]
    out = []
    for m in (M, 1):
        s = _handle(shape, m, conditioned=False); s.set_tol(*FIXED3)
        _planned(s, m)
        k, n = s.solve_keff()
        assert n == 3
        out.append((k, s.history()["k"].copy(), s.history()["cg"].copy(), s.get_phi().copy()))
        s.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][3], out[1][3]), float(np.abs(out[0][3] - out[1][3]).max())


@pytest.mark.parametrize("M", BATCHES)
def test_with_void_cells_bit_equal(M):
    shape = (130, 8, 16)
    inp = _inputs(shape, 2, True)
    mask = np.zeros(shape[::-1], dtype=np.uint8); mask[3:9, 2:5, 40:77] = 1; mask[0, :, :5] = 1
    out = []
    for m in (M, 1):
        s = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
        s.set_linear_solver(6)
        for a, t in zip(inp["bc_attr"], inp["bc_type"]):
            s.set_bc(int(a), int(t))
        s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
        s.set_void(mask, 0.5)
        _set(s, dict(FUSED, xsol_batch=m)); s.build()
        _planned(s, m)
        res = [s.solve_group(0, _rhs(shape)[0], 0.0, M + 1), s.solve_group(1, _rhs(shape)[1], 1e-10, 5000)]
        out.append(res); s.close()
    for (xn, nn, rn), (xo, no, ro) in zip(*out):
        assert nn == no and rn == ro and np.array_equal(xn, xo), (nn, no, float(np.abs(xn - xo).max()))


def test_higher_orders_and_other_forms_keep_one_buffer():
    (shape, rt) = R
    s = _handle(shape, 4, rt=rt)
    plan = s.apply_plan(True)
    assert plan["form"] == "fused" and plan["xsol_batch"] == 1, plan   # RT1-P1: the x pass has no batched instantiation
    s.close()
    s = make_hip(_inputs(A[0], 2, True)); _set(s, dict(CLASSIC, xsol_batch=4))
    plan = s.apply_plan(True)
    assert plan["form"] == "lean" and plan["xsol_batch"] == 1, plan
    assert s.apply_plan(False)["xsol_batch"] == 1
    s.set_option("cg_lean", 0)
    assert s.apply_plan(True)["xsol_batch"] == 4
    s.set_option("xsol_batch", -1)                                 # automatic: small meshes stay with one buffer
    assert s.apply_plan(True)["xsol_batch"] == 1
    s.set_option("xsol_batch", 0)
    assert s.apply_plan(True)["xsol_batch"] == 1
    s.close()
