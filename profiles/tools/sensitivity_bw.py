"""Bandwidth of the sensitivity kernels and cost of a whole nf_sensitivity, outputs on the device:
  256cube_rt0p0: 256^3 RT0-P0 x 2 groups;   128cube_rt2p2: 128^3 RT2-P2 x 2 groups   (downscatter 0 -> 1, every face Dirichlet).
One case per process (--case), so that a `rocprofv3 --kernel-trace --stats` run of its own over this script separates the k_flux_to_J
launches of the two cases:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python profiles/tools/sensitivity_bw.py --case CASE --out CASE.json
The script itself brackets whole calls (mass maps only, dD only, all five) by HIP events on the handle's stream after two warm-up calls --
upper bounds that hold the host-side work of the call -- and takes the copy yardstick nf_time_device_copy in the same process.
  python profiles/tools/sensitivity_bw.py --merge A.json:A_kernel_stats.csv B.json:B_kernel_stats.csv --out profiles/sensitivity_bw.json
folds the kernel averages of the trace into the rows (no GPU needed) with the algorithmic-byte model:
  k_sens_norm    8 N ng (2 nloc + 2) read
  k_sens_mass    8 N ng (2 nloc + 2) read + 8 N (3 ng + ng^2) written                (all four mass maps)
  k_sens_current 8 (2 nJ + N) read + 8 N written, per group
  k_flux_to_J    8 (nphi + nJ) per field and group, spread over its 3 (m+1)^2 launches (one per direction and transverse mode): the moments
                 read, the current written (its factor reads and its in-place sweeps over the faces are not counted: a lower bound)
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
REPS = 10


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
    from neutfem_amd.capi import SensResult
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    n, rt, ng = CASES[name]
    s = make(n, rt, ng)
    N = s.ne
    bufs = [s.vector(ng * N) for _ in range(4)] + [s.vector(ng * ng * N)]
    ptr = [b.ptr for b in bufs]
    res = SensResult()
    call = lambda args: s._chk(s.L.nf_sensitivity(s.h, 0.9, *args, C.byref(res)))
    rows = dict(mass_maps_call=timed(hip, s, lambda: call([None] + ptr[1:])),
                dD_call=timed(hip, s, lambda: call([ptr[0], None, None, None, None])),
                all_maps_call=timed(hip, s, lambda: call(ptr)))
    copy = s.time_device_copy(1 << 30, 20)
    doc = dict(case=name, cells=N, nloc=s.n_loc, groups=ng, n_phi=s.n_phi, n_J=s.n_J, flux_to_J_launches_per_field=3 * (rt + 1) ** 2, norm=res.norm, copy_gbps=copy, reps=REPS + 2, calls=rows)
    for b in bufs: b.free()
    s.close()
    return doc


def kernel_bytes(doc):
    N, ng, nloc, nphi, nJ = doc["cells"], doc["groups"], doc["nloc"], doc["n_phi"], doc["n_J"]
    read = 8 * N * ng * (2 * nloc + 2)
    return {"k_sens_norm": read, "k_sens_mass": read + 8 * N * (3 * ng + ng * ng), "k_sens_current": 8 * (2 * nJ + N) + 8 * N, "k_flux_to_J": 8 * (nphi + nJ) // doc["flux_to_J_launches_per_field"],
            "k_sens_scalars": 0}


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
            m = re.match(r"(?:void )?(?:nf::)?(k_sens_\w+|k_flux_to_J)", r["Name"])
            if not m: continue
            kn = m.group(1)
            if kn not in nbytes: continue
            avg = float(r["AverageNs"])
            row = dict(kernel=r["Name"].split("(")[0], calls=int(r["Calls"]), avg_us=avg / 1e3, min_us=float(r["MinNs"]) / 1e3, total_ms=float(r["TotalDurationNs"]) / 1e6,
                       bytes=nbytes[kn], gbps=nbytes[kn] / avg)
            if nbytes[kn]:
                row["frac_of_copy"] = row["gbps"] / doc["copy_gbps"]; row["frac_of_8tbs"] = row["gbps"] / 8000.0
            kernels.append(row)
        # kernel time of one call with all five maps.  The trace holds reps calls of each kind (mass maps only, dD only, all five):
        # k_sens_norm and k_sens_scalars ran in all three kinds, the other kernels in two of them
        short = lambda name: re.match(r"(?:void )?(?:nf::)?(\w+)", name).group(1)
        per_call = {}
        for k in kernels:
            kinds = 3 if short(k["kernel"]) in ("k_sens_norm", "k_sens_scalars") else 2
            per_call[short(k["kernel"])] = per_call.get(short(k["kernel"]), 0.0) + k["total_ms"] * 1e3 / (kinds * doc["reps"])
        doc["kernels"] = kernels
        doc["all_maps_call_kernel_us"] = per_call
        doc["flux_to_J_share_of_kernel_time"] = per_call.get("k_flux_to_J", 0.0) / max(sum(per_call.values()), 1e-30)
        cases.append(doc)
    with open(out, "w") as fh:
        json.dump(dict(cases=cases), fh, indent=1)
    print(json.dumps(dict(cases=cases)))


ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=sorted(CASES))
ap.add_argument("--merge", nargs="+", metavar="JSON:STATS_CSV")
ap.add_argument("--out", default=os.path.join("profiles", "sensitivity_bw.json"))
a = ap.parse_args()
if a.merge:
    merge(a.merge, a.out)
else:
    doc = run_case(a.case or "256cube_rt0p0")
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))
