"""Fixed-work twin of the group sweep (group_sweep of neutfem_hip.hip), for the tests.

The exact twins of the drivers (subcrit_exact, zoom_exact, transient_exact) are fixed points: a sweep that read the old iterate where it
should read the new one, or ran the groups in the wrong order, reaches the same fixed point a few outers later and no assertion on a
converged solve notices.  After a FIXED NUMBER of outers the iterates differ (gpt_exact.iterate_gamma takes the same remedy), so this twin
follows the iteration of nf_solve_subcritical outer by outer with exact group solves and returns the iterate it has then.

Host DOF layout [g][e*n_loc + p], operators from oracle/ref_scipy.RefScipy as in subcrit_exact."""
import numpy as np

from subcrit_exact import cell_measure, schur_dense


def three_group_inputs(nx, ny, nz):
    """helpers.synthetic_inputs with three groups and the second up-scatter block of tests/test_gpu_transient.py: scatter blocks above and
    below the diagonal, which is what makes the order of the sweep and old / new visible"""
    from helpers import synthetic_inputs
    inp = synthetic_inputs(nx, ny, nz, 3, seed=6)
    inp["SigS"][0, 2] = 0.002 * (inp["NSF"][0] > 0)
    return inp


def fixed_work_subcritical(r, src, n_outer, sinv=None, *, jacobi=False, descending=False, transposed=False):
    """n_outer outers from phi = 0 with the fission term off, then n_outer outers with fission at scale 1; returns the flux (ng, n_phi)
    after each phase.  Each outer forms tf = sum_g Mf_g phi_g from the previous iterate and sweeps the groups in ascending order:
    rhs_g = scale chi_g tf + sum_{g' != g} Ms[(g, g')] phi_g' + q_g with g' < g from this sweep and g' > g from the previous iterate, then
    phi_g = S_g^-1 rhs_g (inverse of subcrit_exact.schur_dense, or diag(sinv[g]): the diagonal path).
    The wrong variants, for the tests' own check that they are told apart: jacobi reads every g' from the previous iterate; descending
    sweeps from the last group to the first under the same g' < g rule; transposed takes Ms[(g', g)]."""
    ng, nP, nloc = r.ng, r.nPhi, r.nloc
    vol = cell_measure(r)
    src = np.asarray(src, dtype=np.float64).reshape(ng, -1)
    q = np.zeros((ng, nP))
    q[:, 0::nloc] = src * vol[None, :]
    if sinv is None:
        Sinv = [np.linalg.inv(schur_dense(r, g)) for g in range(ng)]
        solve = lambda g, b: Sinv[g] @ b
    else:
        solve = lambda g, b: np.asarray(sinv[g]) * b
    chi = [np.repeat(r.Chi[g], nloc) for g in range(ng)]
    if nloc > 1:
        chi = [np.where(np.abs(c) < 1e-14, 0.0, c) for c in chi]   # the drop of k_group_rhs
    order = range(ng - 1, -1, -1) if descending else range(ng)
    phi, out = np.zeros((ng, nP)), []
    for scale in (0.0, 1.0):
        for _ in range(n_outer):
            old, new = phi, phi.copy()
            tf = sum(r.Mf[g] * old[g] for g in range(ng))
            for g in order:
                rhs = scale * chi[g] * tf + q[g]
                for gp in range(ng):
                    key = (gp, g) if transposed else (g, gp)
                    if gp != g and key in r.Ms:
                        rhs = rhs + r.Ms[key] * (new if gp < g and not jacobi else old)[gp]
                new[g] = solve(g, rhs)
            phi = new
        out.append(phi.copy())
    return out


def integrals(r, phi):
    """(phi_int, production) of a flux as nf_subcrit_result has them (subcrit_exact.exact_subcritical's expressions)"""
    mean = np.asarray(phi).reshape(r.ng, -1, r.nloc)[:, :, 0]
    vol = cell_measure(r)
    return float((mean * vol).sum()), float((r.NSF * vol * mean).sum())
