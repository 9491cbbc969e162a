"""The outer step of the power iteration (nf_outer.h: outer_step, cheb_next, cheb_update) on every loop that runs it, past the point where
the Chebyshev schedule restarts.

The acceleration starts at outer 2 and restarts after 15 steps, so outer 17 is the first of the second round (the adjoint starts at outer 5:
outer 20).  The other tests that compare the loops with each other stop after six outers; a loop whose schedule wrapped one step early or
late would pass them.  Here every loop runs 20 outers with the stop tests off (tolerances 0) on the (12, 10, 6) RT0-P0 two-group mesh of
tests/test_gpu_driver_forms.py, forced with the options of tests/test_gpu_paths.py and tests/test_gpu_variants.py:

  host loop (solve_keff_impl)                       last_path 0   the reference of the full-Schur loops
  resident kernel (k_resident_keff)                 last_path 2   k-history against the host loop, 1e-9
  one XCD (k_keff_xcd)                              last_path 3   k-history against the host loop, 1e-9
  diagonal path, device loop (k_outer_logic, k_normalize_fission)   last_path 1   against the diagonal path's host loop (outer_dev = 0), 1e-12

The bars are those the six-outer comparisons use.  The two host loops are held to the CPU oracle's k-history as well (1e-9, the bar of
tests/test_gpu_variants.py against the oracle): every loop takes the schedule from the one header, so a wrong restart length moves them
together and only a reference with a ChebyshevAccel of its own sees it.  After 20 outers the iteration is still far from converged (the
oracle's dk is 8e-6 there), so a restart one step early or late is far above rounding.  solve_adjoint(True, False) -- k free,
accelerated from outer 5 -- runs 22 outers.

Measured on an MI355X (the figures enter no assertion; the parent commit's library gives the same ones, so 20 outers do not make the
paths drift): resident and k_keff_xcd against the host loop 6.7e-16 (1e-9), the diagonal path's device loop against its host loop 1.9e-14
(1e-12), the host loops against the oracle 2.9e-15 and 8.4e-13 (1e-9).  A library built with a restart length of 14 fails the two
comparisons with the oracle from outer 17 on (k off by 8e-6 .. 1.2e-4; the diagonal path by up to 6.8 %).  The whole file runs in 1.5 s."""
import functools

import numpy as np
import pytest

from helpers import make_hip, make_oracle, synthetic_inputs

pytestmark = pytest.mark.gpu

SHAPE, SEED = (12, 10, 6), 4
OUTERS = 20
TOL = (0.0, 0.0, 0.0, OUTERS, 3000)                              # no stop test fires, of the outer iteration or of the inner CG
HOST = dict(resident=0, keff_xcd=0, cg_xcd=0)
LOOPS = {
    "host": (HOST, False, 0),
    "resident": (dict(resident=1, resident_max_dofs=100000), False, 2),
    "xcd": (dict(resident=0, cg_fuse3=1, cg_fuse3_max_cells=4 << 20, cg_xcd=1, keff_xcd=1, cg_xcd_min_cells=0, cg_xcd_max_cells=1 << 30), False, 3),
    "diag-host": (dict(outer_dev=0), True, 0),
    "diag-device": (dict(outer_dev=1), True, 1),
}


@functools.lru_cache(maxsize=None)
def _run(loop):
    opts, diag, path = LOOPS[loop]
    s = make_hip(synthetic_inputs(*SHAPE, 2, seed=SEED))
    for k, v in opts.items():
        s.set_option(k, v)
    s.set_tol(*TOL)
    k, n = s.solve_keff(False, (), diag)
    h = s.history()
    out = dict(k=k, n=n, path=s.info("last_path"), hk=h["k"].copy(), want_path=path)
    s.close()
    return out


@pytest.mark.parametrize("loop", list(LOOPS))
def test_every_loop_runs_its_own_kernels_for_twenty_outers(loop):
    r = _run(loop)
    assert r["path"] == r["want_path"], (loop, r["path"])
    assert r["n"] == OUTERS and len(r["hk"]) == OUTERS and np.all(np.isfinite(r["hk"]))
    assert r["k"] == r["hk"][-1]


@functools.lru_cache(maxsize=None)
def _oracle(diag):
    o = make_oracle(synthetic_inputs(*SHAPE, 2, seed=SEED)); o.set_tol(*TOL)
    o.SolveKeff(False, (), diag); h = o.history()
    assert h["n_outer"] == OUTERS
    return h["k"].copy()


@pytest.mark.parametrize("loop", ["host", "diag-host"])
def test_host_loops_follow_the_oracle_through_the_restart(loop):
    """the anchor of the comparisons below: the oracle has its own ChebyshevAccel, so a schedule that is wrong in every loop alike fails here"""
    ref, r = _oracle(LOOPS[loop][1]), _run(loop)
    err = np.abs(r["hk"] / ref - 1)
    print(f"{loop}: k-history against the oracle, largest relative difference {err.max():.3e} at outer {int(err.argmax())} (1e-9)")
    np.testing.assert_allclose(r["hk"], ref, rtol=1e-9)


@pytest.mark.parametrize("loop", ["resident", "xcd"])
def test_full_schur_loops_follow_the_host_loop_through_the_restart(loop):
    ref, r = _run("host"), _run(loop)
    err = np.abs(r["hk"] / ref["hk"] - 1)
    print(f"{loop}: k-history against the host loop, largest relative difference {err.max():.3e} at outer {int(err.argmax())} (1e-9); "
          f"outers 16..19: {err[16:].max():.3e}")
    np.testing.assert_allclose(r["hk"], ref["hk"], rtol=1e-9)


def test_diagonal_device_loop_follows_its_host_loop_through_the_restart():
    ref, r = _run("diag-host"), _run("diag-device")
    err = np.abs(r["hk"] / ref["hk"] - 1)
    print(f"diagonal path: device loop against host loop, largest relative difference {err.max():.3e} at outer {int(err.argmax())} (1e-12)")
    np.testing.assert_allclose(r["hk"], ref["hk"], rtol=1e-12)


def test_adjoint_with_free_k_runs_through_its_restart():
    s = make_hip(synthetic_inputs(*SHAPE, 2, seed=SEED))
    for k, v in HOST.items():
        s.set_option(k, v)
    s.set_tol(0.0, 0.0, 0.0, 22, 3000)
    s.solve_keff()
    k, n = s.solve_adjoint(True, False)
    h = s.history()
    assert n == 22 and len(h["k"]) == 22
    assert np.all(np.isfinite(h["k"])) and np.all(np.isfinite(h["dk"])) and np.all(np.isfinite(h["dphi"])) and np.isfinite(k)
    assert np.all(np.isfinite(s.get_phi_adj()))
    s.close()
