"""IAEA-3D resampled 256^3, NSF x 0.9: ms per outer of nf_solve_subcritical vs nf_solve_keff on the same handle, bench tolerances.
Run from the repository root on an MI355X after build(); prints one JSON line (profiles/subcrit_vs_keff_256cube.json)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
from neutfem_amd import cases
from neutfem_amd.capi import HipSolver

case = cases.iaea3d_resampled(256)
s = HipSolver(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], 0)
s.set_linear_solver(6)
for a, t in case["bc"]:
    s.set_bc(a, t)
nsf = case["NSF"] * 0.9
s.upload_xs(case["D"], case["SigR"], nsf, case["Chi"], case["SigS"]); s.build()
sync = lambda: s._chk(s.L.nf_synchronize(s.h))
# SolveKeff: 2 warm-up outers, then exactly 20 timed outers (tol_keff = 0), CG tol 1e-4 / 1000 as bench.py
s.set_tol(0.0, 1e-4, 1e-4, 2, 1000); s.solve_keff()
s.set_tol(0.0, 1e-4, 1e-4, 20, 1000); sync(); t0 = time.perf_counter(); k, n = s.solve_keff(); sync(); dt_k = time.perf_counter() - t0
cg_k = int(s.history()["cg"].sum())
# converged k of the scaled core (drivers' tolerances) for the contraction estimate
s.set_tol(1e-5, 1e-4, 1e-4, 200, 1000); kc, nk = s.solve_keff()
src = np.where(case["NSF"][1] > 0, 1.0, 0.0); src = np.stack([src, np.zeros_like(src)])
s.upload_source(src)
s.set_tol(1e-5, 1e-4, 1e-4, 200, 1000)
sync(); t0 = time.perf_counter(); r = s.solve_subcritical(); sync(); dt_s = time.perf_counter() - t0
no = r["n_outer"] + r["n_outer_nofission"]
line = dict(case="iaea3d_resampled_256cube_nsf_x0.9", cells=int(s.ne), groups=int(s.ng), tol="set_tol(1e-5,1e-4,1e-4,200,1000)",
            keff_ms_per_outer=1e3 * dt_k / n, keff_cg_per_outer=cg_k / n, keff_outers_timed=n, keff_converged=kc, keff_outers_to_converge=nk,
            subcrit_ms_per_outer=1e3 * dt_s / no, subcrit_cg_per_outer=r["cg_total"] / no, subcrit_outers=no,
            subcrit_n_outer=r["n_outer"], subcrit_n_outer_nofission=r["n_outer_nofission"], subcrit_converged=r["converged"],
            M=r["M"], k_source=r["k_source"], ratio=r["ratio"], subcrit_wall_s=dt_s)
print(json.dumps(line))
s.close()
