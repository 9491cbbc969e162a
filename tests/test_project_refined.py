"""CPU tests of the sub-cell projection yardstick (tests/project_exact.py) and of the pybind surface of project_flux / project_power
without a device."""
import numpy as np
import pytest

from project_exact import coarse_means, dof0, power_reference, project_reference, random_coefficients

ORDERS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
MESH = {1: (5, 1, 1), 2: (4, 3, 1), 3: (3, 2, 2)}
REFINE = {1: [(1, 1, 1), (2, 1, 1), (3, 1, 1)], 2: [(1, 1, 1), (2, 3, 1), (3, 2, 1)], 3: [(1, 1, 1), (2, 3, 1), (3, 2, 4)]}


def _nloc(dim, m): return (m + 1) ** dim


@pytest.mark.parametrize("rt,m", ORDERS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_reference_conserves_and_refine_one_is_dof0(dim, rt, m):
    nx, ny, nz = MESH[dim]
    nloc = _nloc(dim, m)
    c = random_coefficients(2, nx * ny * nz, nloc, seed=dim * 10 + m)
    for r in REFINE[dim]:
        f = project_reference(c, dim, m, nx, ny, nz, r)
        assert f.shape == (2, nz * r[2], ny * r[1], nx * r[0])
        np.testing.assert_allclose(coarse_means(f, nx, ny, nz, r), dof0(c, nloc), rtol=1e-13, atol=1e-13)
    f1 = project_reference(c, dim, m, nx, ny, nz, (1, 1, 1))
    np.testing.assert_allclose(f1.reshape(2, -1), dof0(c, nloc), rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_reference_p0_replicates(dim):
    nx, ny, nz = MESH[dim]
    c = random_coefficients(1, nx * ny * nz, 1, seed=3)
    r = REFINE[dim][-1]
    f = project_reference(c, dim, 0, nx, ny, nz, r)
    rep = np.repeat(np.repeat(np.repeat(c.reshape(1, nz, ny, nx), r[2], axis=1), r[1], axis=2), r[0], axis=3)
    np.testing.assert_allclose(f, rep, rtol=1e-15, atol=0)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("dim", [1, 2])
def test_reference_matches_exact_antiderivatives(dim, m):
    """the quadrature against exact integration of the Legendre series (numpy's legint), sub-cell by sub-cell"""
    from numpy.polynomial import legendre as L
    nx, ny, nz = MESH[dim]
    nloc = _nloc(dim, m)
    c = random_coefficients(1, nx * ny * nz, nloc, seed=11)
    r = (3, 2, 1) if dim == 2 else (3, 1, 1)
    f = project_reference(c, dim, m, nx, ny, nz, r)[0, 0]
    cc = c.reshape(ny, nx, nloc)
    for iy in range(ny):
        for ix in range(nx):
            if dim == 1:
                ser = cc[iy, ix]
                I = L.legint(ser)
                for a in range(r[0]):
                    lo, hi = -1 + 2 * a / r[0], -1 + 2 * (a + 1) / r[0]
                    ex = (L.legval(hi, I) - L.legval(lo, I)) / (hi - lo)
                    assert abs(f[iy, ix * r[0] + a] - ex) <= 1e-13 * max(1.0, abs(ex))
            else:
                ser2 = cc[iy, ix].reshape(m + 1, m + 1)          # [j][i]
                I = L.legint(L.legint(ser2, axis=1), axis=0)     # antiderivative in xi (axis 1) and eta (axis 0)
                for b in range(r[1]):
                    ylo, yhi = -1 + 2 * b / r[1], -1 + 2 * (b + 1) / r[1]
                    for a in range(r[0]):
                        xlo, xhi = -1 + 2 * a / r[0], -1 + 2 * (a + 1) / r[0]
                        val = lambda x, y: L.legval2d(y, x, I)
                        ex = (val(xhi, yhi) - val(xlo, yhi) - val(xhi, ylo) + val(xlo, ylo)) / ((xhi - xlo) * (yhi - ylo))
                        assert abs(f[iy * r[1] + b, ix * r[0] + a] - ex) <= 1e-13 * max(1.0, abs(ex))


def test_reference_reproduces_the_element_polynomial():
    """a cell polynomial phi(x) = 1 + x / 2 + x^2 on [0, 3], P2 coefficients: every sub-cell mean is the exact integral mean"""
    # on [0, 3]: x = 1.5 (1 + xi); phi = 1 + 0.75 (1 + xi) + 2.25 (1 + xi)^2 = 4 + 5.25 xi + 2.25 xi^2, xi^2 = (2 P2 + 1) / 3
    c = np.array([[4.0 + 0.75, 5.25, 1.5]])
    f = project_reference(c, 1, 2, 1, 1, 1, (3, 1, 1))[0, 0, 0]
    prim = lambda x: x + x * x / 4 + x ** 3 / 3
    np.testing.assert_allclose(f, [prim(b) - prim(b - 1) for b in (1.0, 2.0, 3.0)], rtol=1e-14)


def test_power_reference_weights_each_coarse_cell():
    nx, ny, nz, r = 3, 2, 1, (2, 2, 1)
    c = random_coefficients(2, nx * ny * nz, 4, seed=5)
    f = project_reference(c, 2, 1, nx, ny, nz, r)
    ksf = np.arange(1.0, 13.0).reshape(2, 6)
    p = power_reference(f, ksf, nx, ny, nz, r)
    k0 = np.repeat(np.repeat(ksf.reshape(2, ny, nx), 2, axis=1), 2, axis=2)
    np.testing.assert_allclose(p[0], (k0 * f[:, 0]).sum(axis=0), rtol=1e-15)


def test_pybind_projections_need_build_and_are_no_longer_out_of_scope():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as m
    s = m.NeutFEM(1, 1, 2, np.linspace(0, 30, 4), np.linspace(0, 20, 3), np.array([0.0]))
    s.set_verbosity(m.VerbosityLevel.SILENT)
    for name in ("project_flux", "project_power"):
        with pytest.raises(RuntimeError, match=r"call BuildMatrices\(\) first") as ei:
            getattr(s, name)([2, 2])
        assert "outside the accelerated hot path" not in str(ei.value)
        with pytest.raises(RuntimeError, match=r"call BuildMatrices\(\) first"):
            getattr(s, name)(refine=[1], adjoint=True)
    with pytest.raises(RuntimeError, match="outside the accelerated hot path"):
        s.zoom_resolved([2, 2])
