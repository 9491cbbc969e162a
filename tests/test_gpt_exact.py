"""CPU tests of the generalized-adjoint yardstick (tests/gpt_exact.py): every map against central finite differences of the response ratio
over re-solved dense eigenproblems, the iteration of nf_solve_gpt against the dense Gamma+, the two orthogonality relations, and the
first-order prediction of a block perturbation against the ratio of the perturbed problem."""
import functools

import numpy as np
import pytest

from gpt_exact import dense_gamma, direct_maps, fission_of, gpt_maps, gpt_source, iterate_gamma, predicted_dR, response
from helpers import synthetic_inputs
from sens_exact import _dominant, dense_operators, dominant_pair, flat_inputs, perturbed_block
from subcrit_exact import ref_from_inputs
from test_sens_exact import CASES, FD_BAR, _probes

ITER_TOL = 1e-10
ROUNDING = 1e-13                                                  # sums of a few hundred products of O(1) terms


def weights(ng, ne, seed):
    """w_a random on a fifth of the cells (every group), w_b = 1"""
    rng = np.random.default_rng(seed)
    wa = rng.uniform(0.5, 1.5, (ng, ne)) * (rng.random(ne) < 0.2)[None, :]
    if not wa.any(): wa[:, 0] = 1.0
    return wa, np.ones((ng, ne))


def dense_ratio(r, wa, wb):
    """R of the dominant eigenvector of a built RefScipy"""
    M, F = dense_operators(r)
    return response(r, _dominant(np.linalg.solve(M, F))[1], wa, wb)[0]


@functools.lru_cache(maxsize=None)
def _case(rt, p, n):
    inp = flat_inputs(synthetic_inputs(n[0], n[1], n[2], 3, seed=11 + rt + 3 * p + n[2], void_frac=0))
    r = ref_from_inputs(inp, rt, p)
    k, phi, adj = dominant_pair(r)
    wa, wb = weights(3, r.ne, seed=5 + rt + p)
    return inp, r, k, phi, adj, wa, wb, dense_gamma(r, k, phi, adj, wa, wb)


@pytest.mark.parametrize("rt,p,n", CASES)
def test_maps_match_finite_differences(rt, p, n):
    inp, r, k, phi, adj, wa, wb, gamma = _case(rt, p, n)
    maps = gpt_maps(r, k, phi, gamma); maps.update(direct_maps(r, phi, wa, wb))
    R = response(r, phi, wa, wb)[0]
    rng = np.random.default_rng(rt + 7 * p)
    on = np.flatnonzero(wa[0])
    probes = _probes(3, r.ne, seed=rt + p)
    probes += [("Wa", (int(rng.integers(3)), int(rng.choice(on)))) for _ in range(4)] + [("Wb", (int(rng.integers(3)), int(rng.integers(r.ne)))) for _ in range(4)]
    worst = 0.0
    for key, idx in probes:
        src = dict(Wa=wa, Wb=wb).get(key, inp.get(key))
        v = src[idx]
        h = 1e-4 * max(abs(v), 1e-2)
        Rs = []
        for s in (+1.0, -1.0):
            if key in ("Wa", "Wb"):
                w = src.copy(); w[idx] = v + s * h
                Rs.append(response(r, phi, w if key == "Wa" else wa, w if key == "Wb" else wb)[0])
            else:
                q = dict(inp); q[key] = inp[key].copy(); q[key][idx] = v + s * h
                Rs.append(dense_ratio(ref_from_inputs(q, rt, p), wa, wb))
        fd = (Rs[0] - Rs[1]) / (2 * h) / R
        err = abs(fd - maps[key][idx]) / np.abs(maps[key]).max()
        worst = max(worst, err)
        assert err <= FD_BAR, (key, idx, fd, maps[key][idx], err)
    print(f"gpt FD RT{rt}-P{p} {n}: R={R:.8f} worst |FD - map| / max|map| = {worst:.2e}")
    for g in range(3):
        assert not maps["SigS"][g, g].any()


@pytest.mark.parametrize("rt,p,n", CASES)
def test_iteration_converges_to_dense_gamma(rt, p, n):
    """exact group solves, stopped at a relative change of 1e-10: the error against the dense Gamma+ is at most 10 tol / (1 - rho), rho the
    contraction of the last two changes (a linear contraction leaves tol rho / (1 - rho); the factor 10 covers the non-normal transient)"""
    _, r, k, phi, adj, wa, wb, gamma = _case(rt, p, n)
    G, ch = iterate_gamma(r, k, phi, adj, wa, wb, tol=ITER_TOL)
    rho = ch[-1] / ch[-2]
    err = np.linalg.norm(G - gamma) / np.linalg.norm(gamma)
    print(f"gpt iteration RT{rt}-P{p} {n}: {len(ch)} outers, contraction {rho:.3f}, |G - dense| / |dense| = {err:.2e}")
    assert len(ch) < 5000 and 0 < rho < 1
    assert err <= 10 * ITER_TOL / (1 - rho), (err, rho)


@pytest.mark.parametrize("rt,p,n", CASES)
def test_orthogonality(rt, p, n):
    """<S+, phi> = 0 and <Gamma+, F phi> = 0, to rounding, for the dense solution and for the iterate after 5 outers"""
    _, r, k, phi, adj, wa, wb, gamma = _case(rt, p, n)
    S = gpt_source(r, phi, wa, wb)
    assert abs((S * phi).sum()) <= ROUNDING * np.abs(S * phi).sum()
    Fp = fission_of(r, phi)
    for G in (gamma, iterate_gamma(r, k, phi, adj, wa, wb, n_outer=5)[0]):
        assert abs((G * Fp).sum()) <= ROUNDING * np.linalg.norm(G) * np.linalg.norm(Fp)
    # Gamma+ solves the singular system: the residual of the dense solution is at rounding of the terms
    M, F = dense_operators(r)
    res = (M - F / k).T @ gamma.ravel() - S.ravel()
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(S), np.linalg.norm(res) / np.linalg.norm(S)


BLOCKS = {"perturbed": [iy * 9 + ix for iy in range(2, 5) for ix in range(3, 7)], "corner": [iy * 9 + ix for iy in range(0, 2) for ix in range(0, 3)]}


def block_weights(block, ng=2, ne=63):
    wa = np.zeros((ng, ne)); wa[:, BLOCKS[block]] = 1.0
    return wa, np.ones((ng, ne))


@pytest.mark.parametrize("block", list(BLOCKS))
@pytest.mark.parametrize("rt", [0, 1])
def test_first_order_prediction(rt, block):
    """+1 % SigR_1, -1 % D_0 and +1 % nuSigf_1 on rows 2-4 x columns 3-6 of the 9 x 7 case; R = the share of a block of cells in the
    integrated flux (w_a = 1 on the block, w_b = 1): the block that is perturbed, and the corner block rows 0-1 x columns 0-2.  The
    prediction of the maps is within 3 % of the true change of R (twice the second-order remainder measured when the formulas were
    derived: 1.62 % / 1.42 % on the perturbed block, 0.81 % / 0.88 % on the corner block, RT0-P0 / RT1-P1)"""
    base = flat_inputs(synthetic_inputs(9, 7, 1, 2, seed=8))
    pert = perturbed_block(base)
    wa, wb = block_weights(block)
    r = ref_from_inputs(base, rt, rt)
    k, phi, adj = dominant_pair(r)
    G, ch = iterate_gamma(r, k, phi, adj, wa, wb, tol=ITER_TOL)
    pred = predicted_dR(gpt_maps(r, k, phi, G), base, pert)
    R0 = response(r, phi, wa, wb)[0]
    true = dense_ratio(ref_from_inputs(pert, rt, rt), wa, wb) / R0 - 1.0
    print(f"gpt first order RT{rt}-P{rt} {block} block: R={R0:.6f} predicted dR/R = {pred:.6e} true dR/R = {true:.6e} ({abs(pred / true - 1):.2%}), {len(ch)} outers")
    assert abs(true) > 1e-5 and abs(pred - true) <= 0.03 * abs(true), (pred, true)
