"""CPU tests of the sensitivity yardstick (tests/sens_exact.py): every map against central finite differences of the dense generalised
eigenvalue, and the first-order prediction of a block perturbation against the eigenvalue of the perturbed problem."""
import numpy as np
import pytest

from helpers import synthetic_inputs
from sens_exact import dense_keff, dominant_pair, flat_inputs, perturbed_block, predicted_dk, sens_maps
from subcrit_exact import ref_from_inputs

# central differences with step h = 1e-4 max(|v|, 1e-2) leave a truncation term h^2 k''' / 6; the worst |FD - map| / max|map| was 9.2e-9
# when the formulas were derived (the bar is 10 x that) and is 1.7e-9 .. 2.4e-8 per case with the probes below: truncation, not rounding
FD_BAR = 1e-7
CASES = [  # rt, p, (nx, ny, nz)
    (2, 2, (6, 1, 1)),
    (0, 0, (5, 4, 1)), (1, 1, (5, 4, 1)), (1, 0, (5, 4, 1)),
    (2, 2, (4, 3, 1)),
    (0, 0, (4, 3, 3)),
    (1, 1, (3, 3, 2)),
]


def _probes(ng, ne, seed):
    """20 probes: 4 per map.  Cell 0 (a Dirichlet corner) in every map, both scatter directions (down 1 <- 0, up ng-2 <- ng-1)"""
    rng = np.random.default_rng(seed)
    out = []
    for key in ("D", "SigR", "NSF", "Chi"):
        out.append((key, (0, 0)))
        out += [(key, (int(rng.integers(ng)), int(rng.integers(ne)))) for _ in range(3)]
    out += [("SigS", (1, 0, 0)), ("SigS", (ng - 2, ng - 1, 0)), ("SigS", (1, 0, int(rng.integers(1, ne)))), ("SigS", (ng - 2, ng - 1, int(rng.integers(1, ne))))]
    return out


@pytest.mark.parametrize("rt,p,n", CASES)
def test_maps_match_finite_differences(rt, p, n):
    inp = flat_inputs(synthetic_inputs(n[0], n[1], n[2], 3, seed=11 + rt + 3 * p + n[2], void_frac=0))
    r = ref_from_inputs(inp, rt, p)
    k, phi, adj = dominant_pair(r)
    maps = sens_maps(r, k, phi, adj)
    worst = 0.0
    for key, idx in _probes(3, r.ne, seed=rt + p):
        v = inp[key][idx]
        h = 1e-4 * max(abs(v), 1e-2)
        ks = []
        for s in (+1.0, -1.0):
            q = dict(inp); q[key] = inp[key].copy(); q[key][idx] = v + s * h
            ks.append(dense_keff(ref_from_inputs(q, rt, p)))
        fd = (ks[0] - ks[1]) / (2 * h)
        err = abs(fd - maps[key][idx]) / np.abs(maps[key]).max()
        worst = max(worst, err)
        assert err <= FD_BAR, (key, idx, fd, maps[key][idx], err)
    print(f"sens FD RT{rt}-P{p} {n}: k={k:.8f} worst |FD - map| / max|map| = {worst:.2e}")
    for g in range(3):
        assert not maps["SigS"][g, g].any()                       # the solver never reads the diagonal


@pytest.mark.parametrize("rt", [0, 1])
def test_first_order_prediction(rt):
    """+1 % SigR_1, -1 % D_0 and +1 % nuSigf_1 on the cell block rows 2-4 x columns 3-6 of the 9 x 7 case: the prediction of the maps
    against the eigenvalue of the perturbed problem, within 1 % (measured 0.66 % at RT0-P0, 0.61 % at RT1-P1; the rest is second order)"""
    base = flat_inputs(synthetic_inputs(9, 7, 1, 2, seed=8))
    pert = perturbed_block(base)
    r = ref_from_inputs(base, rt, rt)
    k, phi, adj = dominant_pair(r)
    pred = predicted_dk(sens_maps(r, k, phi, adj), base, pert)
    true = dense_keff(ref_from_inputs(pert, rt, rt)) - k
    print(f"sens first order RT{rt}-P{rt}: predicted dk = {pred:.6e} true dk = {true:.6e} ({abs(pred / true - 1):.2%})")
    assert abs(true) > 1e-5 and abs(pred - true) <= 0.01 * abs(true), (pred, true)
