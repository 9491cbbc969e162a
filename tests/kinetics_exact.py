"""Numpy twin of nf_kinetics_params / nf_transient_kinetics, for the tests.

The bilinear forms of the point-kinetics balance restated on oracle/ref_scipy.RefScipy with the definitions of include/neutfem_hip.h:
K0 = blockdiag(S_g) - Ms (the built operator), F = chi (x) Mf, W = tests/transient_exact.mass_weights, chi_d per DOF as
ExactTransient.chi_d forms it, every product the plain dot product of coefficient vectors in the host DOF layout [g][e*n_loc + p].
No drop of chi / k.  kinetics_forms() works on vectors (S_g phi_g through the sparse factors, so the 3D RT2-P2 cases of the GPU tests stay
cheap) and returns, next to every form, the sum of the absolute values of its terms: the rounding scale of that sum.  dense_operators()
gives K0 and F as dense matrices for the eigenpairs and for the CPU tests that pin the vector forms against w^T K0 phi and w^T F phi.
"""
from types import SimpleNamespace

import numpy as np

from subcrit_exact import schur_dense
from transient_exact import ExactTransient, mass_weights

RAW = ("production", "delayed_production", "removal_leakage", "scatter", "amplitude")


def dense_operators(r):
    """(K0, F) of the built RefScipy, (ng n_phi)^2 each; keep ng n_phi at a few thousand"""
    ng, nP, nloc = r.ng, r.nPhi, r.nloc
    K0 = np.zeros((ng * nP, ng * nP)); F = np.zeros_like(K0)
    for g in range(ng):
        blk = slice(g * nP, (g + 1) * nP)
        K0[blk, blk] = schur_dense(r, g)
        chi = np.repeat(r.Chi[g], nloc)
        for gp in range(ng):
            if gp != g and (g, gp) in r.Ms:
                K0[blk, gp * nP:(gp + 1) * nP] -= np.diag(r.Ms[(g, gp)])
            F[blk, gp * nP:(gp + 1) * nP] = np.diag(chi * r.Mf[gp])
    return K0, F


def eigenpairs(r):
    """(k, phi, w) of the built RefScipy by dense eigen-solves: the largest eigenvalue of K0^-1 F with its right eigenvector phi and the left
    eigenvector w (K0^T w = F^T w / k), both (ng, n_phi), unit norm, signed so that their sums are positive"""
    K0, F = dense_operators(r)
    out = []
    for A in (np.linalg.solve(K0, F), np.linalg.solve(K0.T, F.T)):
        lam, V = np.linalg.eig(A)
        i = int(np.argmax(lam.real))
        v = V[:, i].real
        out.append((float(lam[i].real), (v * np.sign(v.sum()) / np.linalg.norm(v)).reshape(r.ng, r.nPhi)))
    assert abs(out[0][0] - out[1][0]) <= 1e-10 * abs(out[0][0])
    return out[0][0], out[0][1], out[1][1]


def delayed_spectrum(r, chi_delayed):
    """chi_d per group and DOF (ng, n_phi): ExactTransient.chi_d on the given ng values (None: the handle's Chi per cell)"""
    shim = SimpleNamespace(chid=None if chi_delayed is None else np.asarray(chi_delayed, dtype=np.float64), nloc=r.nloc)
    return ExactTransient.chi_d(shim, r)


def derived(raw, beta, k0):
    """the derived fields, in exactly the expressions of include/neutfem_hip.h, from a dict of raw forms"""
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    fw = raw["production"] / k0
    rho = (raw["production"] / k0 - raw["removal_leakage"] + raw["scatter"]) / fw
    bi = [float(b) * raw["delayed_production"] / raw["production"] for b in beta]
    be = 0.0
    for b in bi:
        be += b
    return dict(fw=fw, rho=rho, beta_eff_i=bi, beta_eff=be, gen_time=raw["amplitude"] / fw, rho_dollars=0.0 if be == 0.0 else rho / be)


def kinetics_forms(r, w, phi, velocity, beta, k0, chi_delayed=None, c=None, y=None):
    """every field of nf_pk_result but keff / time / the flags, plus "scale": {form: sum of |terms|} and "y" (ng, n_phi) = S_g phi_g.
    w, phi: (ng, n_phi); c: (I, n_phi) precursors or None (c_amp = 0); y: S_g phi_g if the caller has it already"""
    ng, nP, nloc = r.ng, r.nPhi, r.nloc
    w, phi = np.asarray(w, dtype=np.float64).reshape(ng, nP), np.asarray(phi, dtype=np.float64).reshape(ng, nP)
    v = np.asarray(velocity, dtype=np.float64).reshape(ng)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    if y is None:
        y = np.stack([r.schur_apply(g, phi[g]) for g in range(ng)])
    chi, chid, W = np.repeat(r.Chi, nloc, axis=1), delayed_spectrum(r, chi_delayed), mass_weights(r)
    tf, atf = (r.Mf * phi).sum(axis=0), np.abs(r.Mf * phi).sum(axis=0)
    xw, xd = (chi * w).sum(axis=0), (chid * w).sum(axis=0)
    axw, axd = np.abs(chi * w).sum(axis=0), np.abs(chid * w).sum(axis=0)
    raw, scale = {}, {}
    raw["production"], scale["production"] = float(xw @ tf), float(axw @ atf)
    raw["delayed_production"], scale["delayed_production"] = float(xd @ tf), float(axd @ atf)
    raw["removal_leakage"], scale["removal_leakage"] = float((w * y).sum()), float(np.abs(w * y).sum())
    s = sa = 0.0
    for (g, gp), M in sorted(r.Ms.items()):
        if g != gp:
            t = w[g] * M * phi[gp]
            s += float(t.sum()); sa += float(np.abs(t).sum())
    raw["scatter"], scale["scatter"] = s, sa
    t = W[None, :] * w * phi / v[:, None]
    raw["amplitude"], scale["amplitude"] = float(t.sum()), float(np.abs(t).sum())
    out = dict(raw)
    out.update(derived(raw, beta, k0))
    if c is None:
        out["c_amp"], scale["c_amp"] = [0.0] * beta.size, [0.0] * beta.size
    else:
        c = np.asarray(c, dtype=np.float64).reshape(beta.size, nP)
        out["c_amp"], scale["c_amp"] = [float(xd @ ci) for ci in c], [float(axd @ np.abs(ci)) for ci in c]
    out["scale"], out["y"] = scale, y
    return out


def balance_residual(prev_amplitude, now, dt, lam):
    """identity 2 after a completed implicit-Euler step: (lhs, rhs, size) with lhs = (T^{n+1} - T^n) / dt,
    rhs = (rho - beta_eff) fw + sum_i lambda_i C_i^{n+1} and size = |production| / k0 + |removal_leakage| + |scatter|, the terms rho fw is the
    difference of; `now` is a result dict (twin or GPU) that holds keff or takes k0 from fw"""
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    lhs = (now["amplitude"] - prev_amplitude) / dt
    rhs = (now["rho"] - now["beta_eff"]) * now["fw"] + float(sum(l * ci for l, ci in zip(lam, now["c_amp"])))
    size = abs(now["fw"]) + abs(now["removal_leakage"]) + abs(now["scatter"])
    return lhs, rhs, size
