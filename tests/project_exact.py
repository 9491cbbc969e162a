"""Independent numpy yardstick of the sub-cell projection (nf_project_flux / nf_project_power).

Every sub-cell mean is a tensor 3-point Gauss-Legendre quadrature of the cell's polynomial sum_p c_p P_i(xi) P_j(eta) P_k(zeta) over the
sub-cell (exact for degree <= 5 per axis, the basis has degree <= 2), with the Legendre polynomials evaluated at the nodes -- not the
closed-form sub-interval means the kernel uses.  Coefficients come in the host layout of nf_get_phi / nf_set_phi, [g][e*nloc + p],
p = i + (m+1) j + (m+1)^2 k; xi runs with x over the cell (src/FEM.cpp:123-131).  Fine cells in the reference's order, x fastest."""
import numpy as np

_XQ, _WQ = np.polynomial.legendre.leggauss(3)


def legendre(n, x):
    """P_0..P_n at x (three-term recurrence): shape x.shape + (n + 1,)"""
    P = [np.ones_like(x), x]
    for k in range(1, n):
        P.append(((2 * k + 1) * x * P[k] - k * P[k - 1]) / (k + 1))
    return np.stack(P[:n + 1], axis=-1)


def _axis_nodes(r, m, active):
    """Legendre values at the 3 Gauss nodes of each of r equal sub-intervals of [-1, 1] and the nodes' weights (sum 1):
    (r, 3, m + 1), (3,).  An inactive axis has one node, P_0 = 1, weight 1."""
    if not active:
        return np.ones((1, 1, 1)), np.ones(1)
    lo = -1.0 + 2.0 * np.arange(r) / r
    x = lo[:, None] + (1.0 + _XQ[None, :]) / r                    # nodes of [lo, lo + 2 / r]
    return legendre(m, x), _WQ / 2.0


def project_reference(coef, dim, m, nx, ny, nz, refine):
    """coef: (ng, N * nloc) host layout.  refine = (rx, ry, rz) literally.  Returns (ng, NZ, NY, NX) sub-cell means."""
    rx, ry, rz = refine
    n1 = m + 1
    ng = coef.shape[0]
    nk, nj = (n1 if dim == 3 else 1), (n1 if dim >= 2 else 1)
    c = np.asarray(coef, dtype=np.float64).reshape(ng, nz, ny, nx, nk, nj, n1)
    Px, wx = _axis_nodes(rx, m, True)
    Py, wy = _axis_nodes(ry, m, dim >= 2)
    Pz, wz = _axis_nodes(rz, m, dim == 3)
    Py, Pz = Py[..., :nj], Pz[..., :nk]
    # tensor quadrature: sum over nodes (q, s, t) of wx_q wy_s wz_t phi(x_q, y_s, z_t), phi = sum_ijk c_kji P_i P_j P_k
    v = np.einsum("gzyxkji,aqi,bsj,ctk,q,s,t->gzcybxa", c, Px, Py, Pz, wx, wy, wz, optimize=True)
    return v.reshape(ng, nz * rz, ny * ry, nx * rx)


def power_reference(flux_fine, ksf, nx, ny, nz, refine):
    """sum_g ksf_g(e) flux_g(E): flux_fine (ng, NZ, NY, NX), ksf (ng, N) per coarse cell -> (NZ, NY, NX)"""
    rx, ry, rz = refine
    ng = flux_fine.shape[0]
    k = np.asarray(ksf, dtype=np.float64).reshape(ng, nz, 1, ny, 1, nx, 1)
    f = flux_fine.reshape(ng, nz, rz, ny, ry, nx, rx)
    return (k * f).sum(axis=0).reshape(nz * rz, ny * ry, nx * rx)


def coarse_means(fine, nx, ny, nz, refine):
    """the mean over each coarse cell's rx ry rz equal sub-cells: (..., NZ, NY, NX) -> (..., N).  Equal sub-cells: this is
    sum |sub| value / |e|, the conservation check"""
    rx, ry, rz = refine
    lead = fine.shape[:-3]
    f = fine.reshape(lead + (nz, rz, ny, ry, nx, rx))
    return f.mean(axis=(-5, -3, -1)).reshape(lead + (nz * ny * nx,))


def random_coefficients(ng, N, nloc, seed=0):
    return np.random.default_rng(seed).standard_normal((ng, N * nloc))


def dof0(coef, nloc):
    """(ng, N) cell means of host-layout coefficients"""
    return np.ascontiguousarray(coef.reshape(coef.shape[0], -1, nloc)[..., 0])
