"""Independent numpy yardstick of the zoom (nf_refine / nf_zoom_source / nf_zoom_resolved), over oracle/ref_scipy.RefScipy.

The coarse fission source is restricted to every fine cell by 3-point Gauss-Legendre quadrature of the coarse polynomial against the fine
Legendre basis (exact: degree <= 2 + 2 per axis) -- not the closed-form matrix T the kernel uses -- and loaded with the fine mesh's own
fission matrix RefScipy.Mf; the fixed-source system without fission, K0 phi = q, is then solved exactly (dense) or by Gauss-Seidel
sweeps with RefScipy.cg at 1e-13.  Host DOF layout [g][e*n_loc + p], p = i + (m+1) j + (m+1)^2 k; fine cells in the order of
nf_project_flux (x fastest)."""
import numpy as np

from project_exact import _WQ, _XQ, legendre
from oracle.ref_scipy import RefScipy
from subcrit_exact import cell_measure, ref_from_inputs, schur_dense

DENSE_MAX = 4000                                                  # unknowns (all groups) up to which K0 is formed and solved densely


def _r3(refine):
    return tuple(int(f) for f in refine) + (1,) * (3 - len(refine))


def refine_breaks(b, r):
    """every cell of the break array b cut into r equal parts: b[i] + a (b[i+1] - b[i]) / r, every coarse break kept exactly"""
    b = np.asarray(b, dtype=np.float64)
    if len(b) < 2:
        return b.copy()
    out = np.empty((len(b) - 1) * r + 1)
    for a in range(r):
        out[a:-1:r] = b[:-1] + a * (b[1:] - b[:-1]) / r
    out[-1] = b[-1]
    return out


def refine_inputs(inp, refine):
    """the input dict of the mesh refined by `refine` = (rx[, ry[, rz]]): subdivided breaks, every fine cell with its parent's cross
    sections (np.repeat)"""
    rx, ry, rz = _r3(refine)
    nx = len(inp["x_breaks"]) - 1; ny = max(len(inp["y_breaks"]) - 1, 1); nz = max(len(inp["z_breaks"]) - 1, 1)
    dim = 3 if nz > 1 else (2 if ny > 1 else 1)
    assert (dim >= 2 or ry == 1) and (dim == 3 or rz == 1)
    out = dict(inp)
    out["x_breaks"] = refine_breaks(inp["x_breaks"], rx); out["y_breaks"] = refine_breaks(inp["y_breaks"], ry)
    out["z_breaks"] = refine_breaks(inp["z_breaks"], rz)
    for key in ("D", "SigR", "NSF", "Chi", "SigS"):
        a = np.asarray(inp[key], dtype=np.float64)
        lead = a.size // (nx * ny * nz)
        f = np.repeat(np.repeat(np.repeat(a.reshape(lead, nz, ny, nx), rz, axis=1), ry, axis=2), rx, axis=3)
        shape = (nz * rz, ny * ry, nx * rx)[3 - dim:]
        out[key] = f.reshape(((inp["ng"], inp["ng"]) if key == "SigS" else (int(inp["ng"]),)) + shape)
    return out


def restriction_T(r, m):
    """(r, m+1, m+1): T[s][i'][i], the Legendre coefficients on sub-interval s of r equal parts of [-1, 1] of the polynomial P_i, by
    quadrature: c'_i' = (2 i' + 1) / 2 int_{-1}^{1} P_i(xi_s(x)) P_i'(x) dx, xi_s(x) = -1 + (2 s + 1 + x) / r"""
    lo = -1.0 + 2.0 * np.arange(r) / r
    xi = lo[:, None] + (1.0 + _XQ[None, :]) / r                   # (r, 3) coarse coordinate of the fine nodes
    Pc = legendre(max(m, 1), xi)[..., :m + 1]                     # (r, 3, m+1)   P_i at them
    Pf = legendre(max(m, 1), _XQ)[..., :m + 1]                    # (3, m+1)      P_i' at the nodes of the fine cell
    nrm = (2.0 * np.arange(m + 1) + 1.0) / 2.0
    return np.einsum("q,qa,sqi,a->sai", _WQ, Pf, Pc, nrm)


def restriction_T_closed(s, r, m):
    """the closed form of DESIGN.md 13: mu = (al + be) / 2, w = 1 / r"""
    al, be = (2 * s - r) / r, (2 * s + 2 - r) / r
    mu, w = (al + be) / 2, 1.0 / r
    T = np.array([[1.0, mu, (3 * mu * mu + w * w - 1) / 2], [0.0, w, 3 * mu * w], [0.0, 0.0, w * w]])
    return T[:m + 1, :m + 1]


def restrict_coefficients(coef, dim, m, nx, ny, nz, refine):
    """coef (ng, N nloc) of the coarse mesh -> (ng, NF nloc): on every fine cell the Legendre coefficients of its parent's polynomial"""
    rx, ry, rz = _r3(refine)
    n1 = m + 1
    ng = coef.shape[0]
    nk, nj = (n1 if dim == 3 else 1), (n1 if dim >= 2 else 1)
    c = np.asarray(coef, dtype=np.float64).reshape(ng, nz, ny, nx, nk, nj, n1)
    Tx = restriction_T(rx, m)
    Ty = restriction_T(ry, m) if dim >= 2 else np.ones((1, 1, 1))
    Tz = restriction_T(rz, m) if dim == 3 else np.ones((1, 1, 1))
    f = np.einsum("gzyxkji,aIi,bJj,cKk->gzcybxaKJI", c, Tx, Ty, Tz, optimize=True)
    return f.reshape(ng, -1)


def evaluate(coef_cell, dim, m, pts):
    """the polynomial of one cell (nloc coefficients) at reference points pts (n, dim)"""
    n1 = m + 1
    P = [legendre(max(m, 1), pts[:, a])[..., :n1] for a in range(dim)]
    c = np.asarray(coef_cell).reshape(((n1,) * dim))              # [k][j][i]
    if dim == 1: return np.einsum("i,ni->n", c, P[0])
    if dim == 2: return np.einsum("ji,ni,nj->n", c, P[0], P[1])
    return np.einsum("kji,ni,nj,nk->n", c, P[0], P[1], P[2])


def ref_unbuilt(inp, rt=0, p=0):
    """RefScipy of a test input dict with its cross sections but WITHOUT build(): tables, sizes and geometry only (enough for the load
    vector; building the matrices of a few thousand high-order cells takes minutes)"""
    ng = int(inp["ng"])
    r = RefScipy(rt, p, ng, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    flat = lambda a: np.asarray(a, dtype=np.float64).reshape(ng, -1)
    r.D, r.SigR, r.NSF, r.Chi = flat(inp["D"]), flat(inp["SigR"]), flat(inp["NSF"]), flat(inp["Chi"])
    return r


def _mass(r):
    """per DOF the factor RefScipy.build puts into Mf next to nuSigf: |e| for P0, detJ diag(C-hat) otherwise; shape (n_phi,)"""
    vol = cell_measure(r)
    if r.m == 0:
        return vol.copy()
    return (vol[:, None] / 2.0 ** r.dim * np.diag(r.Chat)[None, :]).ravel()


def fission_matrix(r):
    """RefScipy.Mf (ng, n_phi) from the tables alone, for an instance that was not built (test_zoom_exact checks it against build())"""
    return np.repeat(r.NSF, r.nloc, axis=1) * _mass(r)[None, :]


def zoom_source_reference(rc, rf, coef, keff, refine, adjoint=False):
    """q (ng, n_phi of the fine mesh): chi_g / k sum_g' Mf'_g' c'_g' with the fine mesh's fission matrix rf.Mf (adjoint: nuSigf_g / k
    sum_g' Mchi'_g' c'_g').  rc / rf: RefScipy of the coarse / refined mesh (rf built, or ref_unbuilt: then fission_matrix stands in for
    Mf), coef (ng, n_phi coarse)"""
    cf = restrict_coefficients(np.asarray(coef).reshape(rc.ng, -1), rc.dim, rc.m, rc.nx, rc.ny, rc.nz, refine)
    nloc = rf.nloc
    if not adjoint:
        tf = ((rf.Mf if hasattr(rf, "Mf") else fission_matrix(rf)) * cf).sum(axis=0); wout = rf.Chi
    else:
        tf = (np.repeat(rf.Chi, nloc, axis=1) * _mass(rf)[None, :] * cf).sum(axis=0); wout = rf.NSF
    return np.repeat(wout, nloc, axis=1) * tf[None, :] / keff


def _k0_dense(r, adjoint):
    ng, nP = r.ng, r.nPhi
    K0 = np.zeros((ng * nP, ng * nP))
    for g in range(ng):
        blk = slice(g * nP, (g + 1) * nP)
        K0[blk, blk] = schur_dense(r, g)
        for gp in range(ng):
            key = (gp, g) if adjoint else (g, gp)
            if gp != g and key in r.Ms:
                K0[blk, gp * nP:(gp + 1) * nP] -= np.diag(r.Ms[key])
    return K0


def solve_k0(r, q, adjoint=False, sweeps=200):
    """phi (ng, n_phi) with S_g phi_g = q_g + sum_{g' != g} Ms[g <- g'] phi_g' (adjoint: the transposed blocks): one dense solve up to
    DENSE_MAX unknowns, else Gauss-Seidel sweeps with RefScipy.cg at 1e-13 until the sweep changes nothing beyond 1e-13"""
    ng, nP = r.ng, r.nPhi
    q = np.asarray(q, dtype=np.float64).reshape(ng, nP)
    if ng * nP <= DENSE_MAX:
        return np.linalg.solve(_k0_dense(r, adjoint), q.ravel()).reshape(ng, nP)
    r.cg_tol, r.cg_max = 1e-13, 20 * nP
    phi = np.zeros((ng, nP))
    for _ in range(sweeps):
        old = phi.copy()
        for g in range(ng):
            rhs = q[g].copy()
            for gp in range(ng):
                key = (gp, g) if adjoint else (g, gp)
                if gp != g and key in r.Ms:
                    rhs += r.Ms[key] * phi[gp]
            phi[g] = r.cg(g, rhs)[0]
        if np.linalg.norm(phi - old) <= 1e-13 * np.linalg.norm(phi):
            break
    return phi


def integrals(r, q, phi):
    """the scalar fields of nf_zoom_result"""
    nloc, vol = r.nloc, cell_measure(r)
    mean = phi.reshape(r.ng, -1, nloc)[:, :, 0]
    return dict(source=float(q.reshape(r.ng, -1, nloc)[:, :, 0].sum()), phi_int=float((mean * vol).sum()),
                production=float((r.NSF * vol * mean).sum()), n_cells=r.ne)


def exact_zoom(inp, rt, p, coef, keff, refine, adjoint=False, rc=None, rf=None):
    """the whole zoom on the CPU: dict(q, phi (ng, n_phi fine), rf, source, phi_int, production, n_cells)"""
    rc = rc or ref_from_inputs(inp, rt, p)
    rf = rf or ref_from_inputs(refine_inputs(inp, refine), rt, p)
    q = zoom_source_reference(rc, rf, coef, keff, refine, adjoint)
    phi = solve_k0(rf, q, adjoint)
    return dict(q=q, phi=phi, rc=rc, rf=rf, **integrals(rf, q, phi))
