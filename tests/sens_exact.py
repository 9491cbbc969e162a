"""Independent numpy yardstick of the sensitivity maps (nf_sensitivity), over oracle/ref_scipy.RefScipy.

The generalised eigenproblem M phi = (1/k) F phi is formed densely from the explicit A, B, C, Mf and Ms of a built RefScipy:
    M = blockdiag(S_g) - Ms (off-diagonal blocks only: the solver never reads SigS[g <- g]),   S_g = C_g + B A_g^-1 B^T,
    F[g, g'] = diag(chi_g) Mf_g'.
First-order perturbation theory gives, for a parameter p, dk/dp = -k^2 phi+^T (dM/dp - (1/k) dF/dp) phi / (phi+^T F phi); sens_maps
evaluates these bilinear forms cell by cell with lu.solve, Ahat, _faces, _geom and the Dirichlet integrals of RefScipy.build -- not
the chain blocks the kernels use.  The 1e-14 drop thresholds of the build are ignored.  Host DOF layout [g][e*n_loc + p]."""
import numpy as np

from subcrit_exact import cell_measure, schur_dense


def dense_operators(r):
    """(M, F) of a built RefScipy, (ng n_phi)^2 each"""
    ng, nP, nloc = r.ng, r.nPhi, r.nloc
    M = np.zeros((ng * nP, ng * nP)); F = np.zeros_like(M)
    for g in range(ng):
        blk = slice(g * nP, (g + 1) * nP)
        M[blk, blk] = schur_dense(r, g)
        chi = np.repeat(r.Chi[g], nloc)
        for gp in range(ng):
            bp = slice(gp * nP, (gp + 1) * nP)
            if gp != g and (g, gp) in r.Ms:
                M[blk, bp] -= np.diag(r.Ms[(g, gp)])
            F[blk, bp] = np.diag(chi * r.Mf[gp])
    return M, F


def _dominant(A):
    w, v = np.linalg.eig(A)
    i = int(np.argmax(w.real))
    x = v[:, i].real
    return float(w[i].real), x * np.sign(x.sum())


def dense_keff(r):
    """the dominant eigenvalue k of M^-1 F"""
    M, F = dense_operators(r)
    return _dominant(np.linalg.solve(M, F))[0]


def dominant_pair(r):
    """(k, phi, phi+) with phi, phi+ (ng, n_phi): the dominant direct and left eigenvectors, each scaled to unit 2-norm"""
    M, F = dense_operators(r)
    k, phi = _dominant(np.linalg.solve(M, F))
    ka, adj = _dominant(np.linalg.solve(M.T, F.T))
    assert abs(ka - k) <= 1e-10 * abs(k), (k, ka)
    return k, phi.reshape(r.ng, r.nPhi), adj.reshape(r.ng, r.nPhi)


def mass_weights(r):
    """W_p(e) = detJ(e) C-hat_pp, (ne, n_loc)"""
    return cell_measure(r)[:, None] / 2.0 ** r.dim * np.diag(r.Chat)[None, :]


def currents(r, field):
    """A_g^-1 B^T field_g for every group: (ng, n_J), the reference DOF order"""
    field = np.asarray(field, dtype=np.float64).reshape(r.ng, r.nPhi)
    return np.stack([r.lu[g].solve(r.BT @ field[g]) for g in range(r.ng)])


def dirichlet_integral(r, a, f, ix, iy, iz):
    """I_f(a) of RefScipy.build: the build adds I 2 D to the diagonal of face DOF f of a Dirichlet face of direction a"""
    if r.dim == 1: return 1.0
    area = [r.hy[iy] * r.hz[iz], r.hx[ix] * r.hz[iz], r.hx[ix] * r.hy[iy]][a]
    if r.dim == 2: return 2 * (2 / (2 * f + 1)) / area
    return 4 * (2 / (2 * (f % (r.k + 1)) + 1)) * (2 / (2 * (f // (r.k + 1)) + 1)) / area


def bilinear_mass(r, phi, adj):
    """m[g, g', e] = sum_p phi+_g[e, p] W_p(e) phi_g'[e, p]"""
    W = mass_weights(r)
    p = np.asarray(phi, dtype=np.float64).reshape(r.ng, r.ne, r.nloc); a = np.asarray(adj, dtype=np.float64).reshape(r.ng, r.ne, r.nloc)
    return np.einsum("gep,ep,hep->ghe", a, W, p)


def sens_maps(r, k, phi, adj):
    """dict(D, SigR, NSF, Chi (ng, ne), SigS (ng, ng, ne), Nrm, J, Jadj, m, a, b): the absolute derivatives dk/dp per cell of a built RefScipy
    for the fields phi / adj (ng, n_phi) and the eigenvalue k"""
    ng, ne, nper, d = r.ng, r.ne, r.nper, r.dim
    m = bilinear_mass(r, phi, adj)
    Nrm = float(np.einsum("ge,he,ghe->", r.Chi, r.NSF, m))
    c = -k * k / Nrm
    J, Ja = currents(r, phi), currents(r, adj)
    a = np.zeros((ng, ne)); b = np.zeros((ng, ne))
    n_dir = [r.nx, r.ny, r.nz]
    for iz in range(r.nz):
        for iy in range(r.ny):
            for ix in range(r.nx):
                e = iz * r.nx * r.ny + iy * r.nx + ix
                idx = r._faces(ix, iy, iz); fac, _ = r._geom(ix, iy, iz)
                pos = (ix, iy, iz)
                for dd in range(d):
                    blk = idx[dd * nper:(dd + 1) * nper]
                    for g in range(ng):
                        a[g, e] += fac[dd] * (Ja[g, blk] @ (r.Ahat[dd] @ J[g, blk]))
                    for upper in (False, True):
                        if r.bc.get(r._attr(dd, upper)) != 0 or pos[dd] != (n_dir[dd] - 1 if upper else 0): continue
                        for f in range(r.nf):
                            dof = blk[(r.nf if upper else 0) + f]
                            b[:, e] += dirichlet_integral(r, dd, f, ix, iy, iz) * Ja[:, dof] * J[:, dof]
    out = dict(Nrm=Nrm, J=J, Jadj=Ja, m=m, a=a, b=b)
    out["SigR"] = c * np.einsum("gge->ge", m)
    S = -c * m
    for g in range(ng): S[g, g] = 0.0
    out["SigS"] = S
    out["NSF"] = -(c / k) * np.einsum("ge,ghe->he", r.Chi, m)
    out["Chi"] = -(c / k) * np.einsum("he,ghe->ge", r.NSF, m)
    out["D"] = c * (a / r.D ** 2 - 2.0 * b)
    return out


def predicted_dk(maps, base, pert):
    """sum over the maps of map * (perturbed - base) for the input dicts base / pert"""
    ng = maps["SigR"].shape[0]
    dk = 0.0
    for key in ("D", "SigR", "NSF", "Chi"):
        dk += float((maps[key] * (np.asarray(pert[key], float) - np.asarray(base[key], float)).reshape(ng, -1)).sum())
    dk += float((maps["SigS"] * (np.asarray(pert["SigS"], float) - np.asarray(base["SigS"], float)).reshape(ng, ng, -1)).sum())
    return dk


def flat_inputs(inp):
    """a test input dict with its cross sections as (ng, cells) / (ng, ng, cells) float arrays (copies)"""
    ng = int(inp["ng"])
    out = dict(inp)
    for key in ("D", "SigR", "NSF", "Chi"):
        out[key] = np.array(inp[key], dtype=np.float64).reshape(ng, -1)
    out["SigS"] = np.array(inp["SigS"], dtype=np.float64).reshape(ng, ng, -1)
    return out


def perturbed_block(base, nx=9, ny=7):
    """+1 % SigR_1, -1 % D_0 and +1 % nuSigf_1 on the cell block rows 2-4 x columns 3-6 (the first-order tests), on a flat (ng, cells) input dict"""
    cells = np.array([iy * nx + ix for iy in range(2, 5) for ix in range(3, 7)])
    pert = dict(base)
    for key in ("SigR", "D", "NSF"):
        pert[key] = base[key].copy()
    pert["SigR"][1, cells] *= 1.01; pert["D"][0, cells] *= 0.99; pert["NSF"][1, cells] *= 1.01
    return pert
