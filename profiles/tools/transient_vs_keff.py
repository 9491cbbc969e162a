"""IAEA-3D resampled 256^3, 2 groups, six precursor families, group-2 SigR lowered by 1 % in one assembly: ms per outer of a step of
nf_transient_step against ms per outer of nf_solve_keff on the same handle in the same session, outers per step with the rebalance on
(5 steps of 1e-2 s) and off (capped at 200 outers; argv[2] steps, default 5), the build time of the step operator and the device memory the
transient holds, at the drivers' tolerances.  Run from the repository root on an MI355X after build(); prints progress lines and, last,
one JSON line (profiles/transient_vs_keff_256cube.json)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
from neutfem_amd import cases
from neutfem_amd.capi import HipSolver, mem_info

NC = int(sys.argv[1]) if len(sys.argv) > 1 else 256
OFF_STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
BETA = (2e-4, 1e-3, 1.2e-3, 2.5e-3, 1.5e-3, 5e-4); LAMBDA = (0.0127, 0.0317, 0.115, 0.311, 1.4, 3.87); V = (1e7, 2.2e5)
TOL = (1e-5, 1e-4, 1e-4, 200, 1000); DT = 1e-2
case = cases.iaea3d_resampled(NC)
s = HipSolver(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], 0)
s.set_linear_solver(6)
for a, t in case["bc"]:
    s.set_bc(a, t)
xs = lambda sigr: (case["D"], sigr, case["NSF"], case["Chi"], case["SigS"])
sync = lambda: s._chk(s.L.nf_synchronize(s.h))
s.upload_xs(*xs(case["SigR"])); sync(); t0 = time.perf_counter(); s.build(); sync(); build_s = time.perf_counter() - t0
# SolveKeff: 2 warm-up outers, then exactly 10 timed outers (tol_keff = 0), CG tol 1e-4 / 1000 as bench.py
s.set_tol(0.0, 1e-4, 1e-4, 2, 1000); s.solve_keff()
s.set_tol(0.0, 1e-4, 1e-4, 10, 1000); sync(); t0 = time.perf_counter(); k, n = s.solve_keff(); sync(); dt_k = time.perf_counter() - t0
cg_k = int(s.history()["cg"].sum())
print(f"keff: {1e3 * dt_k / n:.1f} ms per outer, {cg_k / n:.1f} CG per outer", flush=True)
s.set_tol(*TOL); kc, nk = s.solve_keff()
phi0 = s.get_phi().copy()
print(f"keff converged: k = {kc:.8f} in {nk} outers", flush=True)
# the perturbation: the footprint of one 20 cm assembly (150 .. 170 cm in x and y, beside the core's centre) over the fuelled planes, group 2
fuel = case["NSF"][1] > 0
ax, ay = (np.searchsorted(case[b], (150.0, 170.0)) for b in ("x_breaks", "y_breaks"))
sel = np.zeros_like(fuel); sel[:, ay[0]:ay[1], ax[0]:ax[1]] = True; sel &= fuel
sigr = case["SigR"].copy(); sigr[1][sel] *= 0.99


def run(rebalance, n_steps, max_outer):
    s.upload_xs(*xs(case["SigR"])); s.build(); s.set_phi(phi0)
    s.set_option("transient_rebalance", rebalance)
    s.set_tol(TOL[0], TOL[1], TOL[2], max_outer, TOL[4])
    free0 = mem_info(0)[0]
    s.transient_begin(V, BETA, LAMBDA, kc, chi_delayed=(1.0, 0.0))
    s.upload_xs(*xs(sigr)); s.build()
    steps = []
    for i in range(n_steps):
        sync(); t0 = time.perf_counter(); r, p = s.transient_step(DT, 1); sync(); dt = time.perf_counter() - t0
        steps.append(dict(wall_s=dt, n_outer=r["n_outer"], cg_total=r["cg_total"], power=float(p[0]), unconverged=r["n_unconverged"], rebalance=r["rebalance"]))
        print(f"rebalance {rebalance} step {i + 1}: {steps[-1]}", flush=True)
    held = free0 - mem_info(0)[0]
    s.transient_end()
    return steps, held


on, held = run(1, 5, TOL[3])
later = on[1:]                                                    # the first step's call also builds the step operator
ms_outer = 1e3 * sum(x["wall_s"] for x in later) / sum(x["n_outer"] for x in later)
cg_outer = sum(x["cg_total"] for x in later) / sum(x["n_outer"] for x in later)
twin_build_s = on[0]["wall_s"] - 1e-3 * ms_outer * on[0]["n_outer"]
off, _ = run(0, OFF_STEPS, 200)
line = dict(case=f"iaea3d_resampled_{NC}cube", cells=int(s.ne), groups=int(s.ng), tol="set_tol(1e-5,1e-4,1e-4,200,1000)", dt=DT, families=6,
            perturbation=f"group-2 SigR x 0.99 in {int(sel.sum())} cells (one assembly)",
            keff_ms_per_outer=1e3 * dt_k / n, keff_cg_per_outer=cg_k / n, keff_converged=kc, keff_outers_to_converge=nk,
            step_ms_per_outer=ms_outer, step_cg_per_outer=cg_outer,
            step_ms_per_outer_at_keff_cg_rate=ms_outer * (cg_k / n) / cg_outer,
            outers_per_step_rebalance_on=[x["n_outer"] for x in on], unconverged_on=sum(x["unconverged"] for x in on),
            power_on=[x["power"] for x in on], last_f_on=[x["rebalance"] for x in on],
            outers_per_step_rebalance_off_capped_200=[x["n_outer"] for x in off], unconverged_off=sum(x["unconverged"] for x in off),
            power_off=[x["power"] for x in off],
            handle_build_s=build_s, step_operator_build_s=twin_build_s, device_bytes_held=int(held))
print(json.dumps(line))
s.close()
