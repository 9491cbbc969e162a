"""Exact lambda-modes of the discrete diffusion problem, for the tests of nf_solve_modes.

The matrices are the ones tests/subcrit_exact.py forms: K0 = blockdiag(S_g) - Ms and F = chi (x) Mf, assembled densely from
oracle/ref_scipy.RefScipy.  The modes are the eigenpairs of A = K0^-1 F (adjoint: K0^-T F^T) from ONE dense numpy.linalg.eig -- no
iteration, so it is the yardstick for the GPU's block power iteration.  Host DOF layout [g][e*n_loc + p], vectors over all groups.
twin_modes restates the device algorithm in numpy on the same dense A: it is what keeps the outer counts the GPU tests
allow honest.  Keep ng * n_phi at a few thousand unknowns: everything here is dense.
"""
import numpy as np

from subcrit_exact import schur_dense


def dense_operators(r, sinv=None):
    """(K0, F) of a built RefScipy; sinv: list of the diagonal S^-1 per group -- the diagonal route's system"""
    key = None if sinv is None else tuple(np.asarray(s).tobytes() for s in sinv)
    cache = r.__dict__.setdefault("_modes_cache", {})
    if key in cache:
        return cache[key]
    ng, nP, nloc = r.ng, r.nPhi, r.nloc
    K0 = np.zeros((ng * nP, ng * nP)); F = np.zeros_like(K0)
    for g in range(ng):
        blk = slice(g * nP, (g + 1) * nP)
        K0[blk, blk] = schur_dense(r, g) if sinv is None else np.diag(1.0 / np.asarray(sinv[g]))
        chi = np.repeat(r.Chi[g], nloc)
        if nloc > 1:
            chi = np.where(np.abs(chi) < 1e-14, 0.0, chi)         # the drop of k_group_rhs at inv_k = 1
        for gp in range(ng):
            if gp != g and (g, gp) in r.Ms:
                K0[blk, gp * nP:(gp + 1) * nP] -= np.diag(r.Ms[(g, gp)])
            F[blk, gp * nP:(gp + 1) * nP] = np.diag(chi * r.Mf[gp])
    cache[key] = (K0, F)
    return K0, F


def iteration_matrix(r, adjoint=False, sinv=None):
    """A = K0^-1 F (adjoint: K0^-T F^T), dense"""
    K0, F = dense_operators(r, sinv)
    return np.linalg.solve(K0.T, F.T) if adjoint else np.linalg.solve(K0, F)


def exact_modes(r, n, adjoint=False, sinv=None):
    """(k, phi): the n eigenvalues of largest real part of A, descending, and their unit eigenvectors as columns.  The leading modes of
    the cases in the tests are real; a complex one among the n is an error of the caller's case, not silently truncated"""
    w, v = np.linalg.eig(iteration_matrix(r, adjoint, sinv))
    idx = np.argsort(-w.real, kind="stable")[:n]
    assert np.abs(w[idx].imag).max() <= 1e-12 * np.abs(w[idx[0]]), w[idx]
    vec = v[:, idx]
    vec = np.real(vec * np.exp(-1j * np.angle(vec[np.abs(vec).argmax(axis=0), np.arange(len(idx))])))
    return w[idx].real, vec / np.linalg.norm(vec, axis=0)


def mode_residual(r, phi, k, adjoint=False, sinv=None):
    """||A phi - k phi|| / ||k phi|| with the dense A"""
    phi = np.asarray(phi, dtype=np.float64).ravel()
    return float(np.linalg.norm(iteration_matrix(r, adjoint, sinv) @ phi - k * phi) / np.linalg.norm(k * phi))


def start_harmonics(nx, ny, nz, nb):
    """the first nb index triples (i, j, k) with i < nx, j < ny, k < nz in order of i + j + k, then k, then j"""
    tri = sorted(((i + j + k, k, j, i) for k in range(nz) for j in range(ny) for i in range(nx)))[:nb]
    return [(i, j, k) for _, k, j, i in tri]


def start_block(r, nb):
    """the cosine block of k_modes_start in the host layout: the same value in every group, zero in the higher moments"""
    nx, ny, nz, nloc = r.nx, r.ny, r.nz, r.nloc
    x, y, z = (np.arange(n) + 0.5 for n in (nx, ny, nz))
    Q = np.zeros((r.ng * r.nPhi, nb))
    for c, (i, j, k) in enumerate(start_harmonics(nx, ny, nz, nb)):
        v = np.einsum("k,j,i->kji", np.cos(np.pi * k * z / nz), np.cos(np.pi * j * y / ny), np.cos(np.pi * i * x / nx)).ravel()
        for g in range(r.ng):
            Q[g * r.nPhi:(g + 1) * r.nPhi:nloc, c] = v
    return Q


def _sorted_eig(H):
    """eigen-decomposition ordered by descending real part; a complex pair gives the real and the imaginary part as its two columns"""
    w, v = np.linalg.eig(H)
    idx = np.argsort(-w.real, kind="stable")
    w, v = w[idx], v[:, idx]
    V = np.zeros(H.shape); j = 0
    while j < len(w):
        if abs(w[j].imag) > 0 and j + 1 < len(w):
            V[:, j], V[:, j + 1] = v[:, j].real, v[:, j].imag; j += 2
        else:
            V[:, j] = v[:, j].real; j += 1
    return w, V / np.linalg.norm(V, axis=0)


def twin_modes(A, Q0, n_modes, tol_keff, tol_flux, max_outer):
    """subspace iteration with a Rayleigh-Ritz step on the dense A from the block Q0 (n_block columns), as nf_solve_modes runs it.
    Returns dict(k, phi, residual, n_outer, converged)"""
    m = n_modes
    L = np.linalg.cholesky(Q0.T @ Q0)
    Q = Q0 @ np.linalg.inv(L).T
    kprev, conv, n_outer = None, False, 0
    for it in range(max_outer):
        Z = A @ Q
        H, G = Q.T @ Z, Z.T @ Z
        w, V = _sorted_eig(H)
        L = np.linalg.cholesky(V.T @ G @ V)
        R = Z[:, :m] - Q[:, :m] @ H[:m, :m]
        Q = Z @ (V @ np.linalg.inv(L).T)
        k = w[:m].real
        res = (np.linalg.norm(R, axis=0) / np.abs(k)).max()
        dk = np.inf if kprev is None else np.abs(k - kprev).max()
        kprev, n_outer = k, it + 1
        if res < tol_flux and dk < tol_keff and np.all(w[:m].imag == 0):
            conv = True
            break
    Zm = A @ Q[:, :m]
    w, W = _sorted_eig(Q[:, :m].T @ Zm)
    X = Q[:, :m] @ W
    resid = np.linalg.norm(Zm @ W - X * w.real, axis=0) / (np.abs(w.real) * np.linalg.norm(X, axis=0))
    return dict(k=w.real, phi=X / np.linalg.norm(X, axis=0), residual=resid, n_outer=n_outer, converged=conv and bool(np.all(w.imag == 0)))
