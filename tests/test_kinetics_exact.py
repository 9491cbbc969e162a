"""CPU tests that pin the twin of the kinetics parameters (tests/kinetics_exact.py) on the dense yardsticks: the vector forms
against w^T K0 phi and w^T F phi, the exact-perturbation identity, the discrete point-kinetics balance of every implicit-Euler step of
ExactTransient, the beta_eff split and the closed forms of a one-group homogeneous medium."""
import functools

import numpy as np
import pytest

from helpers import synthetic_inputs
from kinetics_exact import balance_residual, dense_operators, eigenpairs, kinetics_forms
from subcrit_exact import homogeneous_inputs, ref_from_inputs
from transient_exact import SIX_BETA, SIX_LAMBDA, TWO_GROUP_V, ExactTransient

THREE_GROUP_V = (1e7, 1e6, 2.2e5)


def _case(name):
    """(inputs, rt, velocities, chi_d, the group whose SigR the scenario scales)"""
    if name == "3d_rt0":
        return synthetic_inputs(6, 5, 3, 2, seed=4), 0, TWO_GROUP_V, (1.0, 0.0), 1
    if name == "3d_rt1":
        return synthetic_inputs(4, 3, 2, 2, seed=4), 1, TWO_GROUP_V, (1.0, 0.0), 1
    if name == "1d_rt2":
        return synthetic_inputs(12, 1, 1, 2, seed=4), 2, TWO_GROUP_V, (1.0, 0.0), 1
    inp = synthetic_inputs(8, 6, 1, 3, seed=6)                    # three groups, upscatter 3 -> 2 (the generator's) and 3 -> 1
    inp["SigS"][0, 2] = 0.002 * (inp["NSF"][0] > 0)
    return inp, 0, THREE_GROUP_V, (1.0, 0.0, 0.0), 2


CASES = ("3d_rt0", "3d_rt1", "1d_rt2", "2d_3g_upscatter")


def _scaled(inp, g, factor):
    sig = np.array(inp["SigR"], dtype=np.float64)
    flat = sig[g].reshape(-1); flat[:16] *= factor               # the first 16 cells of group g (all 12 of the 1D case)
    return sig


@functools.lru_cache(maxsize=None)
def _critical(name):
    inp, rt, v, chid, g = _case(name)
    r = ref_from_inputs(inp, rt, rt)
    k0, phi0, w = eigenpairs(r)
    return inp, rt, v, chid, g, k0, phi0, w


@pytest.mark.parametrize("name", CASES)
def test_vector_forms_are_the_dense_bilinear_forms(name):
    """production = w^T F phi and removal_leakage - scatter = w^T K0 phi on a random sign-mixed pair, to the rounding scale of the sums"""
    inp, rt, v, chid, g, k0, _, _ = _critical(name)
    r = ref_from_inputs(inp, rt, rt)
    rng = np.random.default_rng(3)
    w, phi = rng.standard_normal((r.ng, r.nPhi)), rng.standard_normal((r.ng, r.nPhi))
    K0, F = dense_operators(r)
    f = kinetics_forms(r, w, phi, v, SIX_BETA, k0, chi_delayed=chid)
    sc = f["scale"]
    assert abs(f["production"] - w.ravel() @ F @ phi.ravel()) <= 1e-13 * sc["production"]
    # the dense product sums the terms of the Schur complement in another order: its bar carries the size of the products behind y
    bar = 1e-12 * (np.abs(w.ravel()) @ np.abs(K0) @ np.abs(phi.ravel()))
    assert abs((f["removal_leakage"] - f["scatter"]) - w.ravel() @ K0 @ phi.ravel()) <= bar
    assert sc["scatter"] > 0.0 and f["c_amp"] == [0.0] * 6


@pytest.mark.parametrize("name", CASES)
def test_exact_perturbation(name):
    """identity 1: with (phi', k') the eigenpair of the perturbed built operator and the UNPERTURBED left eigenvector as w, rho = 1 - k0 / k'"""
    inp, rt, v, chid, g, k0, _, w = _critical(name)
    rp = ref_from_inputs(dict(inp, SigR=_scaled(inp, g, 0.97)), rt, rt)
    kp, phip, _ = eigenpairs(rp)
    f = kinetics_forms(rp, w, phip, v, SIX_BETA, k0, chi_delayed=chid)
    print(f"{name}: rho = {f['rho']:.10e}, 1 - k0/k' = {1.0 - k0 / kp:.10e}")
    assert abs(f["rho"]) > 1e-5 and abs(f["rho"] - (1.0 - k0 / kp)) <= 1e-12
    # any w: a random sign-mixed weight gives the same number.  Its bar: the dense eigen-solve leaves a residual of n eps |K0| |phi'| (n eps
    # = 4e-14 at 400 unknowns) that the conditioning of K0 (up to 1e4 on these meshes) carries into phi', on the cancellation of the forms
    wr = np.random.default_rng(5).standard_normal(w.shape)
    fr = kinetics_forms(rp, wr, phip, v, SIX_BETA, k0, chi_delayed=chid)
    cancel = (fr["scale"]["production"] / k0 + fr["scale"]["removal_leakage"] + fr["scale"]["scatter"]) / abs(fr["fw"])
    assert abs(fr["rho"] - (1.0 - k0 / kp)) <= 1e-9 * cancel


@pytest.mark.parametrize("name", CASES)
def test_discrete_point_kinetics_balance(name):
    """identity 2 after every step of the scenario of the transient tests: SigR x 0.97 in 16 cells, 3 steps of 1e-2, then x 1.05, 2 steps of
    1e-3; six families, chi_d = (1, 0[, 0]); residual <= 1e-10 |rho| fw"""
    inp, rt, v, chid, g, k0, phi0, w = _critical(name)
    ex = ExactTransient(inp, rt, rt, v, SIX_BETA, SIX_LAMBDA, k0, phi0, chi_delayed=chid)
    cur = dict(inp)
    r = ref_from_inputs(cur, rt, rt)
    prev = kinetics_forms(r, w, ex.phi, v, SIX_BETA, k0, chi_delayed=chid, c=ex.c)
    assert abs(prev["rho"]) <= 1e-10                              # the critical state: K0 phi = F phi / k0
    for factor, dt, n in ((0.97, 1e-2, 3), (1.05, 1e-3, 2)):
        cur = dict(cur, SigR=_scaled(cur, g, factor))
        ex.set_xs(SigR=cur["SigR"])
        r = ref_from_inputs(cur, rt, rt)                          # the handle's current cross sections, not the dt-shifted operator
        for st in ex.step(dt, n):
            now = kinetics_forms(r, w, st["phi"], v, SIX_BETA, k0, chi_delayed=chid, c=st["c"])
            lhs, rhs, _ = balance_residual(prev["amplitude"], now, dt, SIX_LAMBDA)
            print(f"{name} t={st['time']:.3f}: rho={now['rho']:.6e} ($ {now['rho_dollars']:.4f}) residual / (|rho| fw) = {abs(lhs - rhs) / (abs(now['rho']) * now['fw']):.2e}")
            assert abs(lhs - rhs) <= 1e-10 * abs(now["rho"]) * now["fw"]
            prev = now


@pytest.mark.parametrize("name", CASES)
def test_beta_eff_split(name):
    inp, rt, v, chid, g, k0, phi0, w = _critical(name)
    r = ref_from_inputs(inp, rt, rt)
    f = kinetics_forms(r, w, phi0, v, SIX_BETA, k0, chi_delayed=None)
    assert f["delayed_production"] == f["production"]
    for bi, b in zip(f["beta_eff_i"], SIX_BETA):                  # chi_d = chi: beta_eff,i = beta_i
        assert abs(bi - b) <= 1e-14
    fd = kinetics_forms(r, w, phi0, v, SIX_BETA, k0, chi_delayed=chid)
    print(f"{name}: beta_eff / beta with delayed neutrons born fast = {fd['beta_eff'] / sum(SIX_BETA):.4f}")
    assert fd["beta_eff"] > sum(SIX_BETA)                         # fast neutrons are worth more in these cores
    assert kinetics_forms(r, w, phi0, v, (), k0)["beta_eff"] == 0.0 and kinetics_forms(r, w, phi0, v, (), k0)["rho_dollars"] == 0.0


@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_homogeneous_one_group_closed_forms(dim, rt):
    """one group, uniform cross sections: Lambda = k0 / (v nuSigf) and beta_eff = beta whatever the weight's shape"""
    v, beta = 3e5, 0.0065
    inp = homogeneous_inputs(dim, 1, n=(4, 3, 2))
    r = ref_from_inputs(inp, rt, rt)
    k0, phi0, w = eigenpairs(r)
    f = kinetics_forms(r, w, phi0, [v], [beta], k0)
    lam_exact = k0 / (v * float(inp["NSF"].ravel()[0]))
    assert abs(f["gen_time"] - lam_exact) <= 1e-12 * lam_exact
    assert abs(f["beta_eff"] - beta) <= 1e-12 * beta and abs(f["rho"]) <= 1e-12
