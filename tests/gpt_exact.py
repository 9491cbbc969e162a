"""Independent numpy yardstick of the generalized adjoint and the response-ratio maps (nf_solve_gpt, nf_gpt_sensitivity),
over oracle/ref_scipy.RefScipy and the helpers of sens_exact.py / subcrit_exact.py.

With M phi = (1/k) F phi formed densely (sens_exact.dense_operators), two weight fields w_a, w_b (ng, cells) and
    <w, phi> = sum_g sum_e w[g, e] |e| phibar_g(e),   R = <w_a, phi> / <w_b, phi>,
    S+ = w_a |e| / <w_a, phi> - w_b |e| / <w_b, phi> on the DOF-0 rows (0 on the higher moments),
the generalized adjoint solves (M - F / k)^T Gamma+ = S+ with <Gamma+, F phi> = 0, and
    (1/R) dR/dp = -Gamma+^T (dM/dp - (1/k) dF/dp) phi:
the bilinear forms of sens_exact.sens_maps on (phi, Gamma+) with c = -1 in place of -k^2 / Nrm.  Host DOF layout [g][e*n_loc + p]."""
import numpy as np

from sens_exact import dense_operators, sens_maps
from subcrit_exact import cell_measure, schur_dense


def load_vector(r, w):
    """w (ng, cells) as a load vector (ng, n_phi): DOF 0 of cell e gets w[g, e] |e|, the higher moments 0"""
    w = np.asarray(w, dtype=np.float64).reshape(r.ng, r.ne)
    q = np.zeros((r.ng, r.ne, r.nloc))
    q[:, :, 0] = w * cell_measure(r)[None, :]
    return q.reshape(r.ng, r.nPhi)


def response(r, phi, wa, wb):
    """(R, <w_a, phi>, <w_b, phi>)"""
    phi = np.asarray(phi, dtype=np.float64).reshape(r.ng, r.nPhi)
    a, b = float((load_vector(r, wa) * phi).sum()), float((load_vector(r, wb) * phi).sum())
    return a / b, a, b


def gpt_source(r, phi, wa, wb):
    """S+ (ng, n_phi); <S+, phi> = 0 by construction"""
    _, a, b = response(r, phi, wa, wb)
    return load_vector(r, wa) / a - load_vector(r, wb) / b


def fission_of(r, phi):
    """F phi (ng, n_phi): chi_g(e) tf, tf = sum_g' Mf_g' phi_g' (no drop)"""
    phi = np.asarray(phi, dtype=np.float64).reshape(r.ng, r.nPhi)
    tf = sum(r.Mf[g] * phi[g] for g in range(r.ng))
    return np.stack([np.repeat(r.Chi[g], r.nloc) * tf for g in range(r.ng)])


def deflate(r, G, phi, adj):
    """G - (<G, F phi> / <phi+, F phi>) phi+"""
    Fp = fission_of(r, phi)
    adj = np.asarray(adj, dtype=np.float64).reshape(r.ng, r.nPhi)
    return G - ((G * Fp).sum() / (adj * Fp).sum()) * adj


def dense_gamma(r, k, phi, adj, wa, wb):
    """Gamma+ (ng, n_phi): the minimum-norm solution of the singular system (M - F / k)^T x = S+ (lstsq), then the deflation"""
    M, F = dense_operators(r)
    x = np.linalg.lstsq((M - F / k).T, gpt_source(r, phi, wa, wb).ravel(), rcond=None)[0]
    return deflate(r, x.reshape(r.ng, r.nPhi), phi, adj)


def iterate_gamma(r, k, phi, adj, wa, wb, n_outer=None, tol=None, max_outer=5000):
    """The iteration of nf_solve_gpt with exact group solves, from Gamma = 0: per outer the adjoint fission term of the previous iterate,
    one Gauss-Seidel sweep from the last group to the first on the transposed scatter blocks, in place, then the deflation.  Runs n_outer
    outers, or until the relative change is below tol.  Returns (Gamma (ng, n_phi), the relative change of every outer)"""
    ng, nP = r.ng, r.nPhi
    phi = np.asarray(phi, dtype=np.float64).reshape(ng, nP); adj = np.asarray(adj, dtype=np.float64).reshape(ng, nP)
    Sinv = [np.linalg.inv(schur_dense(r, g)) for g in range(ng)]
    chi = [np.repeat(r.Chi[g], r.nloc) for g in range(ng)]
    src = gpt_source(r, phi, wa, wb)
    Fp = fission_of(r, phi); den = (adj * Fp).sum()
    G = np.zeros((ng, nP)); changes = []
    for it in range(n_outer if n_outer is not None else max_outer):
        old = G.copy()
        tfa = sum(chi[g] * G[g] for g in range(ng))                # F^T Gamma = Mf_g' (sum_g chi_g Gamma_g)
        for g in range(ng - 1, -1, -1):
            rhs = r.Mf[g] * tfa / k + src[g]
            for gp in range(ng):
                if gp != g and (gp, g) in r.Ms:
                    rhs = rhs + r.Ms[(gp, g)] * G[gp]              # transposed block: Ms[g' <- g] acts on Gamma_g'
            G[g] = Sinv[g] @ rhs
        G = G - ((G * Fp).sum() / den) * adj
        changes.append(float(np.linalg.norm(G - old) / np.linalg.norm(G)))
        if tol is not None and changes[-1] < tol:
            break
    return G, changes


def gpt_maps(r, k, phi, gamma):
    """dict(D, SigR, NSF, Chi (ng, ne), SigS (ng, ng, ne)): (1/R) dR/dp per cell, composed from the m, a, b of sens_exact.sens_maps on
    (phi, Gamma+) with c = -1"""
    s = sens_maps(r, k, phi, gamma)
    m, a, b = s["m"], s["a"], s["b"]
    c = -1.0
    out = dict(gamma_F_phi=s["Nrm"])
    out["SigR"] = c * np.einsum("gge->ge", m)
    S = -c * m
    for g in range(r.ng): S[g, g] = 0.0
    out["SigS"] = S
    out["NSF"] = -(c / k) * np.einsum("ge,ghe->he", r.Chi, m)
    out["Chi"] = -(c / k) * np.einsum("he,ghe->ge", r.NSF, m)
    out["D"] = c * (a / r.D ** 2 - 2.0 * b)
    return out


def direct_maps(r, phi, wa, wb):
    """(1/R) dR/dw_a[g, e] = |e| phibar_g(e) / <w_a, phi> and (1/R) dR/dw_b[g, e] = -|e| phibar_g(e) / <w_b, phi>"""
    _, a, b = response(r, phi, wa, wb)
    v = np.asarray(phi, dtype=np.float64).reshape(r.ng, r.ne, r.nloc)[:, :, 0] * cell_measure(r)[None, :]
    return dict(Wa=v / a, Wb=-v / b)


def predicted_dR(maps, base, pert):
    """first-order (1/R) dR: sum over the cross-section maps of map * (perturbed - base) for the input dicts base / pert"""
    ng = maps["SigR"].shape[0]
    d = 0.0
    for key in ("D", "SigR", "NSF", "Chi"):
        d += float((maps[key] * (np.asarray(pert[key], float) - np.asarray(base[key], float)).reshape(ng, -1)).sum())
    d += float((maps["SigS"] * (np.asarray(pert["SigS"], float) - np.asarray(base["SigS"], float)).reshape(ng, ng, -1)).sum())
    return d
