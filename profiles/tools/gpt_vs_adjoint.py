"""IAEA-3D resampled 256^3, 2 groups: ms and CG iterations per outer of nf_solve_gpt against nf_solve_adjoint on the same
handle at the drivers' tolerances, a whole nf_solve_gpt, a whole nf_gpt_sensitivity, and the copy yardstick nf_time_device_copy of the same
process.  R = the share of the central third of the core (all groups) in the integrated flux.
  python profiles/tools/gpt_vs_adjoint.py [--n 256] [--out FILE.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python profiles/tools/gpt_vs_adjoint.py --trace
(--trace: a short solve only -- 12 outers of nf_solve_gpt after 12 of nf_solve_keff and of nf_solve_adjoint -- so that the trace holds the
four streaming kernels, k_gpt_response, k_gpt_source, k_gpt_defl_dot, k_gpt_defl_update, next to the copy kernel)
  python profiles/tools/gpt_vs_adjoint.py --merge RUN.json TRACE.json TRACE_kernel_stats.csv --out profiles/gpt_vs_adjoint_256cube.json
folds the kernel averages of the trace into the record (no GPU needed) with the algorithmic bytes per launch
  k_gpt_response 8 N ng 3 read;  k_gpt_source 8 N ng 3 read + 8 ng nphi written;  k_gpt_defl_dot 8 ng (nphi + N) + 8 nphi read;
  k_gpt_defl_update 8 ng nphi (3 read + 2 written).
Run from the repository root on an MI355X after build()."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--merge", nargs=3, metavar=("RUN_JSON", "TRACE_JSON", "STATS_CSV"))
ap.add_argument("--out", default=None)
a = ap.parse_args()

if a.merge:
    run, trace = (json.load(open(p)) for p in a.merge[:2])
    N, ng, nphi = run["cells"], run["groups"], run["n_phi"]
    nbytes = {"k_gpt_response": 8 * N * ng * 3, "k_gpt_source": 8 * N * ng * 3 + 8 * ng * nphi, "k_gpt_defl_dot": 8 * ng * (nphi + N) + 8 * nphi,
              "k_gpt_defl_update": 8 * ng * nphi * 5}
    rows = []
    for r in csv.DictReader(open(a.merge[2])):
        m = re.match(r"(?:void )?(?:nf::)?(k_gpt_\w+|k_block_finalize|k_fission|k_group_rhs)", r["Name"])
        if not m: continue
        kn, avg = m.group(1), float(r["AverageNs"])
        row = dict(kernel=kn, calls=int(r["Calls"]), avg_us=avg / 1e3, min_us=float(r["MinNs"]) / 1e3, total_ms=float(r["TotalDurationNs"]) / 1e6)
        if kn in nbytes:
            row.update(bytes=nbytes[kn], gbps=nbytes[kn] / avg, frac_of_copy=nbytes[kn] / avg / trace["copy_gbps"], frac_of_8tbs=nbytes[kn] / avg / 8000.0)
        rows.append(row)
    run["trace"] = dict(copy_gbps=trace["copy_gbps"], gpt_outers=trace["gpt_outers"], kernels=rows)
    json.dump(run, open(a.out, "w"), indent=1)
    print(json.dumps(run))
    sys.exit(0)

sys.path.insert(0, os.getcwd())
from neutfem_amd import cases
from neutfem_amd.capi import HipSolver

case = cases.iaea3d_resampled(a.n)
s = HipSolver(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], 0)
s.set_linear_solver(6)
for at, t in case["bc"]:
    s.set_bc(at, t)
s.upload_xs(case["D"], case["SigR"], case["NSF"], case["Chi"], case["SigS"]); s.build()
sync = lambda: s._chk(s.L.nf_synchronize(s.h))
TOL = (1e-5, 1e-4, 1e-4, 200, 1000)
n, ng = a.n, s.ng
wa = np.zeros((ng, n, n, n)); wa[:, n // 3:2 * n // 3, n // 3:2 * n // 3, n // 3:2 * n // 3] = 1.0
wa = wa.reshape(ng, -1); wb = np.ones((ng, s.ne))


def timed(call):
    sync(); t0 = time.perf_counter(); out = call(); sync()
    return time.perf_counter() - t0, out


if a.trace:
    s.set_tol(0.0, 1e-4, 1e-4, 12, 1000)
    k, _ = s.solve_keff(); s.solve_adjoint(True, True)
    r = s.solve_gpt(wa, wb, k)
    doc = dict(copy_gbps=s.time_device_copy(1 << 30, 20), gpt_outers=r["n_outer"], gpt_cg=r["cg_total"])
else:
    s.set_tol(*TOL)
    dt_k, (k, nk) = timed(s.solve_keff)
    print(f"keff: k = {k:.8f} in {nk} outers, {dt_k:.1f} s", flush=True)
    dt_a, (ka, na) = timed(lambda: s.solve_adjoint(True, True))
    cg_a = s.info("last_cg_total")
    print(f"adjoint: {na} outers, {1e3 * dt_a / na:.1f} ms and {cg_a / na:.1f} CG per outer", flush=True)
    runs = {}
    for mo in (2, 12):                                            # the difference is ten whole outers: the set-up cancels
        s.set_tol(TOL[0], TOL[1], TOL[2], mo, TOL[4])
        runs[mo] = timed(lambda: s.solve_gpt(wa, wb, k))
        print(f"gpt max_outer {mo}: {runs[mo][0]:.2f} s, cg {runs[mo][1]['cg_total']}", flush=True)
    ms_gpt = 1e3 * (runs[12][0] - runs[2][0]) / 10
    cg_gpt = (runs[12][1]["cg_total"] - runs[2][1]["cg_total"]) / 10
    s.set_tol(*TOL)
    dt_g, r = timed(lambda: s.solve_gpt(wa, wb, k))
    print(f"gpt: {r}, {dt_g:.1f} s", flush=True)
    dt_s, out = timed(lambda: s.gpt_sensitivity(k)["result"])
    copy = s.time_device_copy(1 << 30, 20)
    doc = dict(case=f"iaea3d_resampled_{n}cube", cells=int(s.ne), groups=int(ng), n_phi=int(s.n_phi), tol="set_tol(1e-5,1e-4,1e-4,200,1000)",
               response="share of the central third of the core per axis, all groups", keff=k, keff_outers=nk, keff_wall_s=dt_k,
               adjoint_outers=na, adjoint_ms_per_outer=1e3 * dt_a / na, adjoint_cg_per_outer=cg_a / na,
               gpt_ms_per_outer=ms_gpt, gpt_cg_per_outer=cg_gpt, gpt_ms_per_outer_at_adjoint_cg_rate=ms_gpt * (cg_a / na) / cg_gpt,
               gpt_result=r, gpt_wall_s=dt_g, gpt_sensitivity_wall_s_host_arrays=dt_s, gamma_F_phi=out["norm"], copy_gbps=copy,
               cg_form=int(s.info("cg_form")))
if a.out:
    json.dump(doc, open(a.out, "w"), indent=1)
print(json.dumps(doc))
s.close()
