"""Bandwidth of k_kin_forms and cost of a whole nf_transient_kinetics:
  256cube_rt0p0: 256^3 RT0-P0 x 2 groups x 6 families;   128cube_rt2p2: 128^3 RT2-P2 x 2 groups x 6 families
(downscatter 0 -> 1, every face Dirichlet, a transient begun on random positive fields: the precursors are at their equilibrium).
One case per process (--case), under a kernel-trace run of its own (no counters mixed in):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python profiles/tools/kinetics_bw.py --case CASE --out CASE.json
The script brackets whole calls by HIP events on the handle's stream after two warm-up calls (median of 10): nf_transient_kinetics, and
nf_solve_group held to CG_ITS iterations (tol 0) for the time of one CG iteration on the same handle.  In the same process it calls
nf_sensitivity without maps (k_sens_norm, the read-only sibling) as often, and takes the copy yardstick nf_time_device_copy.
  python profiles/tools/kinetics_bw.py --merge A.json:A_kernel_stats.csv B.json:B_kernel_stats.csv --out profiles/kinetics_bw.json
folds the kernel averages of the trace into the rows (no GPU needed) with the algorithmic-byte model:
  k_kin_forms  8 n_phi (4 ng + 1 + I + b) + 8 N ng read  (w, phi, y, Mf of every group, W, the I precursor vectors, the b non-empty scatter
               blocks; chi once per cell)
  k_sens_norm  8 N ng (2 nloc + 2) read
Run from the repository root on an MI355X after build()."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys

import numpy as np

CASES = {"256cube_rt0p0": (256, 0, 2), "128cube_rt2p2": (128, 2, 2)}
REPS, CG_ITS = 10, 20
BETA = (2e-4, 1e-3, 1.2e-3, 2.5e-3, 1.5e-3, 5e-4)
LAMBDA = (0.0127, 0.0317, 0.115, 0.311, 1.4, 3.87)
VELOCITY = (1e7, 2.2e5)


def make(n, rt, ng):
    from neutfem_amd.capi import HipSolver
    b = np.linspace(0.0, float(n), n + 1)
    s = HipSolver(rt, rt, ng, b, b, b)
    N = n ** 3
    one = np.ones(ng * N)
    chi = np.zeros(ng * N); chi[:N] = 1.0
    sigs = np.zeros(ng * ng * N); sigs[ng * N:(ng + 1) * N] = 0.02          # downscatter 0 -> 1 only
    for a in (1, 2, 3, 4, 5, 6):
        s.set_bc(a, 0)
    s.upload_xs(one, 0.05 * one, 0.02 * one, chi, sigs)
    del one, chi, sigs
    s.build()
    rng = np.random.default_rng(0)
    for setter in (s.set_phi, s.set_phi_adj):                     # one group at a time on the host: 128^3 RT2-P2 is 0.45 GB per group
        setter(np.concatenate([rng.uniform(0.5, 2.0, N * s.n_loc) for _ in range(ng)]))
    return s


def timed(hip, s, call):
    st = C.c_void_p(s.L.nf_stream(s.h))
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    call(); call()
    ms = []
    for _ in range(REPS):
        hip.hipEventRecord(e0, st); call(); hip.hipEventRecord(e1, st); hip.hipEventSynchronize(e1)
        f = C.c_float(); hip.hipEventElapsedTime(C.byref(f), e0, e1); ms.append(f.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)))


def run_case(name):
    sys.path.insert(0, os.getcwd())
    from neutfem_amd.capi import PkResult, SensResult
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    n, rt, ng = CASES[name]
    s = make(n, rt, ng)
    s.transient_begin(VELOCITY, BETA, LAMBDA, 1.0, chi_delayed=(1.0, 0.0))
    pk, sens = PkResult(), SensResult()
    rows = dict(transient_kinetics_call=timed(hip, s, lambda: s._chk(s.L.nf_transient_kinetics(s.h, C.byref(pk)))),
                sens_norm_call=timed(hip, s, lambda: s._chk(s.L.nf_sensitivity(s.h, 1.0, None, None, None, None, None, C.byref(sens)))))
    rhs, x = s.vector(), s.vector()
    rhs.upload(np.random.default_rng(1).uniform(0.5, 2.0, s.n_phi))
    its = C.c_int()
    cg = timed(hip, s, lambda: s._chk(s.L.nf_solve_group(s.h, 0, rhs.ptr, x.ptr, 0.0, CG_ITS, C.byref(its), None)))
    rows["cg_iteration"] = dict(ms_median=cg["ms_median"] / CG_ITS, ms_min=cg["ms_min"] / CG_ITS, iterations_per_call=its.value, form=int(s.info("cg_form")))
    rhs.free(); x.free()
    copy = s.time_device_copy(1 << 30, 20)
    doc = dict(case=name, cells=s.ne, nloc=s.n_loc, groups=ng, n_phi=s.n_phi, families=len(BETA), scatter_blocks=1, production=pk.production, rho=pk.rho,
               gen_time=pk.gen_time, beta_eff=pk.beta_eff, copy_gbps=copy, reps=REPS + 2, calls=rows)
    s.transient_end(); s.close()
    return doc


def kernel_bytes(doc):
    N, ng, nloc, nphi, I, b = doc["cells"], doc["groups"], doc["nloc"], doc["n_phi"], doc["families"], doc["scatter_blocks"]
    return {"k_kin_forms": 8 * nphi * (4 * ng + 1 + I + b) + 8 * N * ng, "k_sens_norm": 8 * N * ng * (2 * nloc + 2)}


def merge(pairs, out):
    cases = []
    for pair in pairs:
        jpath, cpath = pair.split(":")
        with open(jpath) as fh:
            doc = json.load(fh)
        nbytes = kernel_bytes(doc)
        kernels = []
        with open(cpath) as fh:
            rows = list(csv.DictReader(fh))
        for r in rows:
            m = re.match(r"(?:void )?(?:nf::)?(k_kin_forms|k_sens_norm|k_finalize|k_tr_weights)", r["Name"])
            if not m: continue
            kn = m.group(1)
            avg = float(r["AverageNs"])
            row = dict(kernel=r["Name"].split("(")[0], calls=int(r["Calls"]), avg_us=avg / 1e3, min_us=float(r["MinNs"]) / 1e3, total_ms=float(r["TotalDurationNs"]) / 1e6)
            if kn in nbytes:
                row.update(bytes=nbytes[kn], gbps=nbytes[kn] / avg)
                row["frac_of_copy"] = row["gbps"] / doc["copy_gbps"]; row["frac_of_8tbs"] = row["gbps"] / 8000.0
            kernels.append(row)
        by = {re.match(r"(?:void )?(?:nf::)?(\w+)", k["kernel"]).group(1): k for k in kernels}
        if "k_kin_forms" in by and "k_sens_norm" in by:
            doc["kin_forms_vs_sens_norm_frac_of_copy"] = by["k_kin_forms"]["frac_of_copy"] / by["k_sens_norm"]["frac_of_copy"]
        doc["call_over_cg_iteration"] = doc["calls"]["transient_kinetics_call"]["ms_median"] / doc["calls"]["cg_iteration"]["ms_median"]
        doc["kernels"] = kernels
        cases.append(doc)
    with open(out, "w") as fh:
        json.dump(dict(cases=cases), fh, indent=1)
    print(json.dumps(dict(cases=cases)))


ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=sorted(CASES))
ap.add_argument("--merge", nargs="+", metavar="JSON:STATS_CSV")
ap.add_argument("--out", default=os.path.join("profiles", "kinetics_bw.json"))
a = ap.parse_args()
if a.merge:
    merge(a.merge, a.out)
else:
    doc = run_case(a.case or "256cube_rt0p0")
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))
