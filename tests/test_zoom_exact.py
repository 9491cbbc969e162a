"""CPU tests of the zoom yardstick (tests/zoom_exact.py): the quadrature restriction against the closed form of DESIGN.md 13 and against
the sub-interval means of the projection, the sub-cell coefficients against the coarse polynomial, and the refine-1 identity on a solved
RefScipy."""
import numpy as np
import pytest

from helpers import rel_l2, synthetic_inputs
from project_exact import project_reference, random_coefficients
from subcrit_exact import ref_from_inputs
from zoom_exact import (evaluate, exact_zoom, fission_matrix, ref_unbuilt, refine_breaks, refine_inputs, restrict_coefficients, restriction_T, restriction_T_closed,
                        zoom_source_reference)

# an entry of the quadrature T is (2 i' + 1) / 2 <= 2.5 times a sum of 3 products w P_i' P_i of factors of size <= 1, each factor within a
# few ulps (node, weight, three-term recurrence): <= 2.5 * 3 * ~10 ulps < 1e-14 absolute.  The closed form is good to an ulp or two.
T_ATOL = 1e-14
MESH = {1: (5, 1, 1), 2: (4, 3, 1), 3: (3, 2, 2)}
REFINE = {1: (3, 1, 1), 2: (2, 3, 1), 3: (3, 2, 4)}


@pytest.mark.parametrize("m", [0, 1, 2])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 7])
def test_quadrature_T_equals_closed_form(r, m):
    T = restriction_T(r, m)
    for s in range(r):
        np.testing.assert_allclose(T[s], restriction_T_closed(s, r, m), rtol=0, atol=T_ATOL)
    if r == 1:
        np.testing.assert_allclose(T[0], np.eye(m + 1), rtol=0, atol=T_ATOL)


@pytest.mark.parametrize("r", [1, 2, 3, 5])
def test_row_zero_is_sub_means(r):
    """row 0 of T: the means of P_0, P_1, P_2 over the sub-interval, the formulas of sub_means"""
    T = restriction_T(r, 2)
    for s in range(r):
        al, be = (2 * s - r) / r, (2 * s + 2 - r) / r
        np.testing.assert_allclose(T[s, 0], [1.0, 0.5 * (al + be), 0.5 * (al * al + al * be + be * be - 1.0)], rtol=0, atol=T_ATOL)


@pytest.mark.parametrize("m", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_restriction_reproduces_the_coarse_polynomial(dim, m):
    """at random points of every fine cell the restricted coefficients give the value of the parent's polynomial, and their DOF 0 is the
    sub-cell mean of the projection yardstick"""
    nx, ny, nz = MESH[dim]
    r = REFINE[dim]
    nloc = (m + 1) ** dim
    c = random_coefficients(2, nx * ny * nz, nloc, seed=7 * dim + m)
    f = restrict_coefficients(c, dim, m, nx, ny, nz, r)
    means = project_reference(c, dim, m, nx, ny, nz, r).reshape(2, -1)
    np.testing.assert_allclose(f.reshape(2, -1, nloc)[:, :, 0], means, rtol=1e-13, atol=1e-13)
    rng = np.random.default_rng(5)
    NX, NY = nx * r[0], ny * r[1]
    fc, cc = f.reshape(2, -1, nloc), c.reshape(2, -1, nloc)
    for E in rng.choice(fc.shape[1], size=min(12, fc.shape[1]), replace=False):
        X, Y, Z = E % NX, (E // NX) % NY, E // (NX * NY)
        sub = (X % r[0], Y % r[1], Z % r[2]); e = ((Z // r[2]) * ny + Y // r[1]) * nx + X // r[0]
        pf = rng.uniform(-1, 1, (6, dim))
        pc = np.stack([-1.0 + (2 * sub[a] + 1 + pf[:, a]) / r[a] for a in range(dim)], axis=1)
        for g in range(2):
            np.testing.assert_allclose(evaluate(fc[g, E], dim, m, pf), evaluate(cc[g, e], dim, m, pc), rtol=1e-13, atol=1e-13)


def test_refine_inputs_keeps_coarse_breaks_and_injects():
    inp = synthetic_inputs(5, 4, 3, 2, seed=2)
    f = refine_inputs(inp, (3, 1, 2))
    assert np.array_equal(f["x_breaks"][::3], inp["x_breaks"]) and np.array_equal(f["z_breaks"][::2], inp["z_breaks"])
    assert np.array_equal(f["y_breaks"], inp["y_breaks"]) and np.all(np.diff(f["x_breaks"]) > 0)
    assert f["D"].shape == (2, 6, 4, 15) and f["SigS"].shape == (2, 2, 6, 4, 15)
    assert np.array_equal(f["NSF"][:, ::2, :, ::3], inp["NSF"]) and np.array_equal(f["NSF"][:, 1::2, :, 2::3], inp["NSF"])
    assert np.array_equal(refine_breaks(np.array([0.0]), 4), np.array([0.0]))


@pytest.mark.parametrize("dim,rt", [(1, 2), (2, 0), (2, 1), (3, 1), (3, 2)])
def test_fission_matrix_without_build_is_RefScipy_Mf(dim, rt):
    """the tables-only fission matrix equals what RefScipy.build assembles (the products are formed in another order: an ulp or two)"""
    nx, ny, nz = MESH[dim]
    inp = synthetic_inputs(nx, ny, nz, 2, seed=4)
    np.testing.assert_allclose(fission_matrix(ref_unbuilt(inp, rt, rt)), ref_from_inputs(inp, rt, rt).Mf, rtol=1e-15, atol=0)


@pytest.mark.parametrize("rt", [0, 1])
def test_refine_one_source_is_the_fission_term_and_identity(rt):
    """refine (1, 1, 1): the load vector is chi / k Mf phi entry by entry, and with a converged (phi, k) the zoom returns phi -- the
    outer iteration stopped at dphi < 1e-11, which bounds the error of phi by 1e-11 / (1 - dominance ratio) < 1e-8"""
    inp = synthetic_inputs(7, 6, 1, 2, seed=5, void_frac=0.0)
    r = ref_from_inputs(inp, rt, rt)
    r.set_tol(1e-12, 1e-11, 1e-11, 2000, 4000); r.cg_tol = 1e-13
    k = r.solve_keff()
    phi = r.phi.reshape(2, -1)
    q = zoom_source_reference(r, r, phi, k, (1, 1, 1))
    tf = (r.Mf * phi).sum(axis=0)
    np.testing.assert_allclose(q, np.repeat(r.Chi, r.nloc, axis=1) * tf[None, :] / k, rtol=1e-14, atol=0)
    z = exact_zoom(inp, rt, rt, phi, k, (1, 1, 1), rc=r, rf=r)
    assert rel_l2(z["phi"], phi) <= 1e-8, rel_l2(z["phi"], phi)


def test_zoom_beats_projection_on_a_synthetic_core():
    """RT0-P0, synthetic 10 x 8 refined (2, 3): against the eigen-solve of the refined mesh (cell means, best scaling) the zoom is at
    least twice as close as the plain injection of the coarse flux"""
    inp = synthetic_inputs(10, 8, 1, 2, seed=5, void_frac=0.0)
    ref = (2, 3, 1)
    rc = ref_from_inputs(inp, 0, 0); rc.set_tol(1e-10, 1e-9, 1e-9, 2000, 4000); k = rc.solve_keff()
    rf = ref_from_inputs(refine_inputs(inp, ref), 0, 0); rf.set_tol(1e-10, 1e-9, 1e-9, 2000, 4000); rf.solve_keff()
    phi = rc.phi.reshape(2, -1)
    z = exact_zoom(inp, 0, 0, phi, k, ref, rc=rc, rf=rf)
    proj = project_reference(phi, 2, 0, 10, 8, 1, ref).reshape(-1)
    truth = rf.phi.copy()
    def err(v):
        v = v.ravel(); s = (v @ truth) / (v @ v)
        return rel_l2(s * v, truth)
    assert err(z["phi"]) <= 0.5 * err(proj), (err(z["phi"]), err(proj))
