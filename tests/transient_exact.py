"""Exact implicit-Euler stepper of the space-time kinetics system of nf_transient_step, for the tests.

The discrete system is formed explicitly with oracle/ref_scipy.RefScipy, as tests/subcrit_exact.py forms the fixed-source one: the step
operator is the built operator of the cross sections with SigR_g + 1 / (v_g dt), and one step is ONE dense numpy solve of
    (blockdiag(S_g^dt) - chi~ (x) Mf / k0 - Ms) phi^{n+1} = q,      q_g = W phi_g^n / (v_g dt) + chi_d,g sum_i lambda_i c_i^n / (1 + lambda_i dt)
    chi~_g = chi_g - chi_d,g a(dt),   a(dt) = sum_i beta_i / (1 + lambda_i dt),   c_i^{n+1} = (c_i^n + dt beta_i tf(phi^{n+1}) / k0) / (1 + lambda_i dt)
-- no iteration, so it is the yardstick for the GPU's rebalanced source iteration.  chi~ / k0 below 1e-14 is dropped at P >= 1, as
k_group_rhs drops it.  W_p(e) = detJ(e) C-hat_pp (|e| at P0), no drop.  Precursors live in tf-space: one vector of n_phi values per family.
Host DOF layout [g][e*n_loc + p].  Keep ng * n_phi at a few thousand unknowns: the step matrix is dense.
"""
import numpy as np
import scipy.linalg as sla

from subcrit_exact import cell_measure, ref_from_inputs, schur_dense

# six precursor families of the tests (beta_i, lambda_i in 1/s) and two-group velocities (cm/s)
SIX_BETA = (2e-4, 1e-3, 1.2e-3, 2.5e-3, 1.5e-3, 5e-4)
SIX_LAMBDA = (0.0127, 0.0317, 0.115, 0.311, 1.4, 3.87)
TWO_GROUP_V = (1e7, 2.2e5)


def mass_weights(r):
    """W_p(e) = detJ(e) C-hat_pp with C-hat_pp = prod_t 2 / (2 i_t + 1) (Legendre mass), host layout [e*n_loc + p]"""
    n, d = r.m + 1, r.dim
    c = np.array([np.prod([2.0 / (2.0 * ((q // n ** t) % n) + 1.0) for t in range(d)]) for q in range(r.nloc)])
    vol = cell_measure(r)
    return vol.copy() if r.nloc == 1 else (vol[:, None] / 2.0 ** d * c[None, :]).ravel()


def fundamental_mode(r):
    """(k, phi) of the built RefScipy by a dense eigen-solve of K0^-1 F; phi (ng, n_phi) signed so that its sum is positive"""
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
    w, V = np.linalg.eig(np.linalg.solve(K0, F))
    i = int(np.argmax(w.real))
    phi = V[:, i].real
    phi *= np.sign(phi.sum()) / np.linalg.norm(phi)
    return float(w[i].real), phi.reshape(ng, nP)


class ExactTransient:
    """begin at construction (phi0, equilibrium precursors, t = 0); set_xs() perturbs the core; step() advances and returns one dict per step"""

    def __init__(self, inp, rt, p, velocity, beta, lam, keff, phi0, chi_delayed=None):
        self.inp, self.rt, self.p = dict(inp), rt, p
        self.v = np.asarray(velocity, dtype=np.float64)
        self.beta, self.lam = np.asarray(beta, dtype=np.float64).reshape(-1), np.asarray(lam, dtype=np.float64).reshape(-1)
        self.k0 = float(keff)
        r = ref_from_inputs(self.inp, rt, p)
        self.ng, self.nP, self.nloc = r.ng, r.nPhi, r.nloc
        self.vol, self.W = cell_measure(r), mass_weights(r)
        self.chid = None if chi_delayed is None else np.asarray(chi_delayed, dtype=np.float64)
        self.phi = np.asarray(phi0, dtype=np.float64).reshape(self.ng, self.nP).copy()
        tf = (r.Mf * self.phi).sum(axis=0)
        self.c = self.beta[:, None] * tf[None, :] / (self.lam[:, None] * self.k0)
        self.P0 = self._production(r, self.phi)
        self.t, self.n_steps, self._op = 0.0, 0, None

    def _mean(self, phi): return phi.reshape(self.ng, -1, self.nloc)[:, :, 0]
    def _production(self, r, phi): return float((r.NSF * self.vol * self._mean(phi)).sum())

    def set_xs(self, **xs):
        self.inp.update(xs); self._op = None

    def _operator(self, dt):
        if self._op is not None and self._op[0] == dt:
            return self._op[1:]
        shift = (1.0 / (self.v * dt)).reshape((self.ng,) + (1,) * (np.asarray(self.inp["SigR"]).ndim - 1))
        r = ref_from_inputs(dict(self.inp, SigR=np.asarray(self.inp["SigR"]) + shift), self.rt, self.p)
        ng, nP = self.ng, self.nP
        K0 = np.zeros((ng * nP, ng * nP))
        for g in range(ng):
            blk = slice(g * nP, (g + 1) * nP)
            K0[blk, blk] = schur_dense(r, g)
            for gp in range(ng):
                if gp != g and (g, gp) in r.Ms:
                    K0[blk, gp * nP:(gp + 1) * nP] -= np.diag(r.Ms[(g, gp)])
        chid = self.chi_d(r)
        chit = np.repeat(r.Chi, self.nloc, axis=1) - chid * float((self.beta / (1.0 + self.lam * dt)).sum())
        if self.nloc > 1:
            chit = np.where(np.abs(chit / self.k0) < 1e-14, 0.0, chit)
        for g in range(ng):
            for gp in range(ng):
                K0[g * nP:(g + 1) * nP, gp * nP:(gp + 1) * nP] -= np.diag(chit[g] * r.Mf[gp] / self.k0)
        if not np.all(np.isfinite(K0)):
            raise FloatingPointError("the step matrix holds non-finite values")
        self._op = (dt, r, chid, sla.lu_factor(K0))             # the full step matrix, fission included: factored once per (dt, cross sections)
        return self._op[1:]

    def chi_d(self, r):
        """delayed spectrum per group and DOF (ng, n_phi): the given ng values in every cell, or the handle's Chi"""
        per_cell = r.Chi if self.chid is None else np.repeat(self.chid[:, None], r.ne, axis=1)
        return np.repeat(per_cell, self.nloc, axis=1)

    def step(self, dt, n_steps=1):
        out = []
        ng, nP, nloc = self.ng, self.nP, self.nloc
        for _ in range(n_steps):
            r, chid, lu = self._operator(dt)
            delayed = (self.lam[:, None] * self.c / (1.0 + self.lam[:, None] * dt)).sum(axis=0) if self.lam.size else np.zeros(nP)
            q = self.W[None, :] * self.phi / (self.v[:, None] * dt) + chid * delayed[None, :]
            phi = sla.lu_solve(lu, q.ravel()).reshape(ng, nP)
            if not np.all(np.isfinite(phi)):
                raise FloatingPointError("the dense step produced non-finite values")
            tf = (r.Mf * phi).sum(axis=0)
            self.c = (self.c + dt * self.beta[:, None] * tf[None, :] / self.k0) / (1.0 + self.lam[:, None] * dt)
            self.phi = phi; self.t += dt; self.n_steps += 1
            P = self._production(r, phi)
            out.append(dict(phi=phi.copy(), c=self.c.copy(), time=self.t, power=P / self.P0, production=P,
                            phi_int=float((self._mean(phi) * self.vol).sum()),
                            precursors=float(self.c.reshape(self.c.shape[0], -1, nloc)[:, :, 0].sum()) if self.lam.size else 0.0))
        return out


def homogeneous_recurrence(s, eps, v, dt, beta, lam, n):
    """one-group homogeneous medium, one family, nuSigf scaled by 1 + eps at t = 0: the flux stays a_n phi0 and the precursors gamma_n W phi0;
    s = nuSigf / k0.  Returns [(a_1, gamma_1), ..., (a_n, gamma_n)]"""
    sp, a = (1.0 + eps) * s, beta / (1.0 + lam * dt)
    amp, gam, out = 1.0, beta * s / lam, []
    for _ in range(n):
        amp = (amp / (v * dt) + lam * gam / (1.0 + lam * dt)) / (s + 1.0 / (v * dt) - (1.0 - a) * sp)
        gam = (gam + dt * beta * sp * amp) / (1.0 + lam * dt)
        out.append((amp, gam))
    return out
