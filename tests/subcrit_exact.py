"""Exact solution of the fixed-source (subcritical) problem of nf_solve_subcritical, for the tests.

The discrete system is formed explicitly with oracle/ref_scipy.RefScipy (assembled A, B, C, fission and scatter matrices) and solved
with one dense numpy solve -- no iteration, so it is the yardstick for the GPU's source iteration:
    K phi = q,   K = blockdiag(S_g) - chi (x) Mf - Ms,   S_g = C_g + B A_g^-1 B^T
and K0 phi0 = q without the fission term.  q_g[e, dof 0] = Q_g(e) |e|, higher moments 0.  Host DOF layout [g][e*n_loc + p].
Keep ng * n_phi at a few thousand unknowns: K is dense.
"""
import numpy as np

from oracle.ref_scipy import RefScipy


def ref_from_inputs(inp, rt=0, p=0, NSF=None):
    """a built RefScipy of a test input dict (helpers.synthetic_inputs / load_inputs); NSF overrides the input's"""
    ng = int(inp["ng"])
    r = RefScipy(rt, p, ng, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    r.bc = {int(a): int(t) for a, t in zip(inp["bc_attr"], inp["bc_type"])}
    flat = lambda a, n: np.asarray(a, dtype=np.float64).reshape(n, -1)
    r.D, r.SigR, r.Chi = flat(inp["D"], ng), flat(inp["SigR"], ng), flat(inp["Chi"], ng)
    r.NSF = flat(inp["NSF"] if NSF is None else NSF, ng)
    r.SigS = np.asarray(inp["SigS"], dtype=np.float64).reshape(ng, ng, -1)
    r.build()
    return r


def cell_measure(r):
    return np.einsum("k,j,i->kji", r.hz, r.hy, r.hx).ravel()


def schur_dense(r, g):
    """S_g = C_g + B A_g^-1 B^T as a dense matrix (no drop threshold)"""
    return np.diag(r.C[g]) + r.B @ r.lu[g].solve(r.BT.toarray())


def exact_subcritical(r, src, sinv=None):
    """exact phi / phi0 and the integrals of nf_subcrit_result for the source src (ng, cells).  sinv: list of the diagonal S^-1 per
    group (nf_get_diagonal_cache) -- the diagonal path's system, S_g replaced by diag(1 / sinv_g)"""
    ng, nP, nloc = r.ng, r.nPhi, r.nloc
    vol = cell_measure(r)
    src = np.asarray(src, dtype=np.float64).reshape(ng, -1)
    q = np.zeros(ng * nP)
    for g in range(ng):
        q[g * nP:(g + 1) * nP][0::nloc] = src[g] * vol
    K0 = np.zeros((ng * nP, ng * nP))
    for g in range(ng):
        blk = slice(g * nP, (g + 1) * nP)
        K0[blk, blk] = schur_dense(r, g) if sinv is None else np.diag(1.0 / np.asarray(sinv[g]))
        for gp in range(ng):
            if gp != g and (g, gp) in r.Ms:
                K0[blk, gp * nP:(gp + 1) * nP] -= np.diag(r.Ms[(g, gp)])
    K = K0.copy()
    for g in range(ng):
        chi = np.repeat(r.Chi[g], nloc)
        if nloc > 1:
            chi = np.where(np.abs(chi) < 1e-14, 0.0, chi)
        for gp in range(ng):
            K[g * nP:(g + 1) * nP, gp * nP:(gp + 1) * nP] -= np.diag(chi * r.Mf[gp])     # chi_g tf: per DOF, tf = sum_g' Mf_g' phi_g'
    phi, phi0 = np.linalg.solve(K, q), np.linalg.solve(K0, q)
    mean = lambda v: v.reshape(ng, -1, nloc)[:, :, 0]
    phi_int = float((mean(phi) * vol).sum()); phi_int0 = float((mean(phi0) * vol).sum())
    production = float((r.NSF * vol * mean(phi)).sum()); source = float((src * vol).sum())
    return dict(phi=phi.reshape(ng, nP), phi0=phi0.reshape(ng, nP), M=phi_int / phi_int0, k_source=production / (production + source),
                phi_int=phi_int, phi_int_nofission=phi_int0, production=production, source=source, q=q.reshape(ng, nP))


def homogeneous_inputs(dim, ng, n=(4, 3, 2), bc_type=2):
    """uniform cross sections on a uniform mesh (n cells per active axis), every face of type bc_type; 2 groups: fission in both,
    chi = (1, 0), downscatter 1 -> 2"""
    nx, ny, nz = n[0], n[1] if dim >= 2 else 1, n[2] if dim == 3 else 1
    shape = (nz, ny, nx)[3 - dim:]
    D = np.array([1.3, 0.4])[:ng]; SigR = np.array([0.03, 0.09])[:ng]; NSF = np.array([0.006, 0.11])[:ng]
    full = lambda v: np.stack([np.full(shape, x) for x in v])
    Chi = np.zeros((ng,) + shape); Chi[0] = 1.0
    SigS = np.zeros((ng, ng) + shape)
    if ng == 2:
        SigS[1, 0] = 0.02
    attrs = {1: (1, 2), 2: (1, 2, 3, 4), 3: (1, 2, 3, 4, 5, 6)}[dim]
    return dict(x_breaks=np.linspace(0.0, 2.0 * nx, nx + 1), y_breaks=np.linspace(0.0, 2.5 * ny, ny + 1) if dim >= 2 else np.array([0.0]),
                z_breaks=np.linspace(0.0, 3.0 * nz, nz + 1) if dim == 3 else np.array([0.0]), D=full(D), SigR=full(SigR), NSF=full(NSF),
                Chi=Chi, SigS=SigS, bc_attr=np.array(attrs), bc_type=np.full(len(attrs), bc_type), ng=ng)
