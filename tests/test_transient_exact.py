"""CPU tests that pin the yardstick of the transient tests (tests/transient_exact.py): a homogeneous one-group medium, where one
implicit-Euler step is a scalar recurrence, and the null transient of a converged eigenpair."""
import numpy as np
import pytest

from helpers import rel_l2, synthetic_inputs
from subcrit_exact import homogeneous_inputs, ref_from_inputs
from transient_exact import SIX_BETA, SIX_LAMBDA, TWO_GROUP_V, ExactTransient, fundamental_mode, homogeneous_recurrence, mass_weights


@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_homogeneous_one_group_recurrence(dim, rt):
    eps, v, dt, beta, lam = 0.004, 3e5, 0.02, 0.0065, 0.08
    inp = homogeneous_inputs(dim, 1, n=(4, 3, 2))
    r = ref_from_inputs(inp, rt, rt)
    k0, phi0 = fundamental_mode(r)
    ex = ExactTransient(inp, rt, rt, [v], [beta], [lam], k0, phi0)
    ex.set_xs(NSF=inp["NSF"] * (1.0 + eps))
    steps = ex.step(dt, 6)
    rec = homogeneous_recurrence(float(inp["NSF"].ravel()[0]) / k0, eps, v, dt, beta, lam, 6)
    W = mass_weights(r)
    for st, (amp, gam) in zip(steps, rec):
        assert rel_l2(st["phi"], amp * phi0) <= 1e-10
        assert rel_l2(st["c"][0], gam * W * phi0[0]) <= 1e-10
        assert abs(st["power"] - amp * (1.0 + eps)) <= 1e-10 * amp
    assert 2.5 < rec[-1][0] < 2.7                                # a_6 is about 2.61: the transient is a real one


@pytest.mark.parametrize("chi_delayed", [None, (1.0, 0.0)])
def test_null_transient(chi_delayed):
    """unperturbed cross sections from a converged eigenpair: nothing moves, with six families, also when chi_d differs from chi"""
    inp = synthetic_inputs(6, 5, 1, 2, seed=4)                    # chi = (0.8, 0.2)
    r = ref_from_inputs(inp, 1, 1)
    k0, phi0 = fundamental_mode(r)
    ex = ExactTransient(inp, 1, 1, TWO_GROUP_V, SIX_BETA, SIX_LAMBDA, k0, phi0, chi_delayed=chi_delayed)
    c0 = ex.c.copy()
    for st in ex.step(0.1, 5):
        assert abs(st["power"] - 1.0) <= 1e-10
        assert rel_l2(st["phi"], phi0) <= 1e-10
        assert rel_l2(st["c"], c0) <= 1e-10
    assert abs(ex.t - 0.5) <= 1e-15 and ex.n_steps == 5
