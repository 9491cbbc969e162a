"""CPU checks of the yardstick of the lambda-mode tests (tests/modes_exact.py): the exact spectrum against what is known, the adjoint
spectrum against the direct one, and the numpy twin of the block iteration on every case the GPU tests run -- its outer counts are what
keeps the max_outer of tests/test_gpu_modes.py honest."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_inputs, make_oracle, synthetic_inputs
from modes_exact import exact_modes, iteration_matrix, mode_residual, start_block, start_harmonics, twin_modes
from subcrit_exact import homogeneous_inputs, ref_from_inputs


@pytest.fixture(scope="module")
def iaea2d():
    return ref_from_inputs(load_inputs("iaea2d"), 0, 0)


@pytest.fixture(scope="module")
def syn884():
    inp = synthetic_inputs(8, 8, 4, 2, seed=4)
    return inp, ref_from_inputs(inp, 0, 0)


def test_iaea2d_exact_spectrum(iaea2d):
    """k0 against the golden power iteration (stopped at dk < 1e-10, dphi < 1e-10: the eigenvalue is then good to about
    dk / (1 - dominance ratio) = 1e-10 / 0.013 < 1e-8), and the leading spectrum the issue quotes: a degenerate first harmonic pair"""
    with open(os.path.join(GOLDEN, "golden_iaea2d.json")) as f:
        run = [r for r in json.load(f)["runs"] if r["tol"][0] == 1e-10 and not r["coarse"] and not r["diag"] and r["rt"] == 0][0]
    k, phi = exact_modes(iaea2d, 4)
    print(k, k[0] - run["keff"])
    assert abs(k[0] - run["keff"]) <= 1e-8
    assert np.abs(k - [1.028986, 1.015486, 1.015486, 0.999342]).max() <= 1e-6 and abs(k[1] - k[2]) <= 1e-10
    assert abs(k[1] / k[0] - 0.987) <= 5e-4
    for i in range(4):
        assert mode_residual(iaea2d, phi[:, i], k[i]) <= 1e-12


def test_adjoint_spectrum_equals_direct(iaea2d, syn884):
    for r in (iaea2d, syn884[1]):
        kd, _ = exact_modes(r, 4); ka, va = exact_modes(r, 4, adjoint=True)
        assert np.abs(ka - kd).max() <= 1e-12 * kd[0]
        assert mode_residual(r, va[:, 0], ka[0], adjoint=True) <= 1e-12


def test_start_block():
    assert start_harmonics(4, 3, 2, 8) == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (0, 2, 0), (1, 0, 1)]
    assert start_harmonics(4, 1, 1, 4) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)]
    r = ref_from_inputs(homogeneous_inputs(2, 2, n=(4, 3, 2)), 1, 1)
    Q = start_block(r, 5)
    assert np.linalg.matrix_rank(Q) == 5 and np.all(Q[:, 0].reshape(2, -1, r.nloc)[:, :, 0] == 1.0) and np.all(Q.reshape(2, -1, r.nloc, 5)[:, :, 1:] == 0.0)


def _twin(r, m, guard, tol, adjoint=False, sinv=None):
    A = iteration_matrix(r, adjoint, sinv)
    tw = twin_modes(A, start_block(r, m + guard), m, tol[0], tol[1], tol[3])
    k, _ = exact_modes(r, m, adjoint, sinv)
    ex = max(mode_residual(r, tw["phi"][:, i], tw["k"][i], adjoint, sinv) for i in range(m))
    print("outers", tw["n_outer"], "dk", np.abs(tw["k"] - k).max(), "residual", tw["residual"].max(), ex)
    return tw, np.abs(tw["k"] - k).max(), ex


# outer counts of the twin; the GPU runs the same algorithm with another summation order and an inner solve of finite accuracy
HOMOGENEOUS_OUTERS = {(1, 0): 3, (1, 1): 10, (1, 2): 11, (2, 0): 21, (2, 1): 21, (2, 2): 24, (3, 0): 26, (3, 1): 27, (3, 2): 27}


@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_twin_homogeneous(dim, rt):
    r = ref_from_inputs(homogeneous_inputs(dim, 2, n=(4, 3, 2)), rt, rt)
    tw, dk, ex = _twin(r, 2 if dim == 1 else 3, 2, (1e-13, 1e-11, 1e-11, 500))
    assert tw["converged"] and abs(tw["n_outer"] - HOMOGENEOUS_OUTERS[(dim, rt)]) <= 1 and tw["n_outer"] <= 500 // 4
    assert dk <= 1e-13 and ex <= 1e-11


def test_twin_heterogeneous(syn884):
    tol = (1e-11, 1e-10, 1e-10, 400)
    inp, r = syn884
    tw, dk, ex = _twin(r, 3, 2, tol)
    assert tw["converged"] and abs(tw["n_outer"] - 58) <= 2 and dk <= 1e-11 and ex <= 1e-10
    tw, dk, ex = _twin(r, 3, 2, tol, adjoint=True)
    assert tw["converged"] and abs(tw["n_outer"] - 57) <= 2 and dk <= 1e-11 and ex <= 1e-10
    o = make_oracle(inp)                                          # the diagonal route's system, S_g replaced by the diagonal cache
    o.BuildMatrices(); o.SolveKeff(use_diagonal_solver=True)
    tw, dk, ex = _twin(r, 3, 2, tol, sinv=[np.array(o.diag_cache(g)) for g in range(2)])
    assert tw["converged"] and abs(tw["n_outer"] - 222) <= 5 and dk <= 1e-11 and ex <= 1e-10       # the slowest of the CG-route cases: max_outer 400
    r1 = ref_from_inputs(synthetic_inputs(6, 5, 3, 2, seed=4), 1, 1)
    tw, dk, ex = _twin(r1, 3, 2, tol)
    assert tw["converged"] and abs(tw["n_outer"] - 56) <= 2 and dk <= 1e-11 and ex <= 1e-10


def test_twin_iaea2d_degenerate_pair(iaea2d):
    tw, dk, ex = _twin(iaea2d, 3, 3, (1e-9, 1e-8, 1e-8, 2000))
    assert tw["converged"] and abs(tw["n_outer"] - 303) <= 10 and dk <= 1e-9 and ex <= 1e-8


def test_twin_small_cases():
    """the 2D case of the state / error / pybind tests, with guards and as a plain power iteration (b = 1)"""
    r = ref_from_inputs(synthetic_inputs(12, 10, 1, 2, seed=3), 0, 0)
    tw, dk, ex = _twin(r, 2, 2, (1e-10, 1e-8, 1e-8, 500))
    assert tw["converged"] and tw["n_outer"] <= 125 and ex <= 1e-8
    tw, dk, ex = _twin(r, 1, 0, (1e-10, 1e-8, 1e-8, 2000))
    assert tw["converged"] and tw["n_outer"] <= 500 and ex <= 1e-8
