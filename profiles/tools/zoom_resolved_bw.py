"""Bandwidth of k_zoom_source and cost of a whole nf_zoom_resolved:
  128^3 RT0-P0 x 2 groups, refine 2 (fine 256^3) and 64^3 RT1-P1 x 2 groups, refine 2: nf_zoom_source next to nf_project_flux (all groups)
  at the same shape and next to the copy yardstick nf_time_device_copy of the same run;
  nf_zoom_resolved 128^3 -> 256^3 RT0-P0 at the drivers' tolerances (1e-5, 1e-4, 1e-4, 200, 1000; CG pushed): wall time, outers, CG total.
Calls are bracketed by HIP events on the handle's stream after two warm-up calls; nf_zoom_source also sums and reads back the source total
inside the interval, so that figure is an upper bound of the kernel time (`rocprofv3 --kernel-trace --stats` over this script with
--kernels-only gives the kernels alone).  Algorithmic bytes of k_zoom_source: 8 N ng (nloc + 2) read + 8 N R ng nloc written, R = rx ry rz.
Run from the repository root on an MI355X after build(); writes profiles/zoom_resolved.json (or --out) and prints the same JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from neutfem_amd.capi import HipSolver

try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
REPS = 10


def make(n, rt, p, ng):
    b = np.linspace(0.0, float(n), n + 1)
    s = HipSolver(rt, p, ng, b, b, b)
    N = n ** 3
    one = np.ones(ng * N)
    chi = np.zeros(ng * N); chi[:N] = 1.0
    sigs = np.zeros(ng * ng * N); sigs[ng * N:(ng + 1) * N] = 0.02          # downscatter 0 -> 1 only
    for a in (1, 2, 3, 4, 5, 6):
        s.set_bc(a, 0)
    s.upload_xs(one, 0.05 * one, 0.02 * one, chi, sigs)
    del one, chi, sigs
    s.build()
    s.set_phi(np.random.default_rng(0).uniform(0.5, 2.0, (ng, N * s.n_loc)))
    s.set_linear_solver(6)
    return s


def timed(s, call):
    st = C.c_void_p(s.L.nf_stream(s.h))
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    call(); call()
    ms = []
    for _ in range(REPS):
        hip.hipEventRecord(e0, st); call(); hip.hipEventRecord(e1, st); hip.hipEventSynchronize(e1)
        f = C.c_float(); hip.hipEventElapsedTime(C.byref(f), e0, e1); ms.append(f.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return float(np.median(ms)), float(min(ms))


def kernel_case(name, n, rt, ng, r, copy_gbps=None):
    c = make(n, rt, rt, ng)
    f = c.refine(*r)
    N, R, nloc = c.ne, r[0] * r[1] * r[2], c.n_loc
    zoom_bytes = 8 * N * ng * (nloc + 2) + 8 * N * R * ng * nloc
    zm, zb = timed(f, lambda: c.zoom_source(f, 0.9))
    buf = c.vector(N * R * ng)
    proj_bytes = 8 * N * ng * (nloc + R)
    pm, pb = timed(c, lambda: c._chk(c.L.nf_project_flux(c.h, r[0], r[1], r[2], 0, -1, buf.ptr)))
    if copy_gbps is None:
        copy_gbps = c.time_device_copy(1 << 30, 20)
    buf.free(); f.close(); c.close()
    row = lambda nbytes, med, best: dict(bytes=nbytes, ms_median=med, ms_min=best, gbps=nbytes / (med * 1e-3) / 1e9,
                                         frac_of_copy=nbytes / (med * 1e-3) / 1e9 / copy_gbps)
    return dict(case=name, cells=N, nloc=nloc, groups=ng, refine=list(r), zoom_source_call=row(zoom_bytes, zm, zb),
                project_flux_all_groups_call=row(proj_bytes, pm, pb)), copy_gbps


def whole(n, r):
    c = make(n, 0, 0, 2)
    c.set_tol(1e-5, 1e-4, 1e-4, 200, 1000)
    out = []
    for _ in range(2):                                            # the second call runs with a warm allocator and loaded code objects
        t0 = time.perf_counter()
        f, res = c.zoom_resolved(r, 0.9)
        dt = time.perf_counter() - t0
        f.close()
        out.append(dict(seconds=dt, **res))
    c.close()
    return dict(coarse=n, refine=list(r), tol=[1e-5, 1e-4, 1e-4, 200, 1000], calls=out)


ap = argparse.ArgumentParser()
ap.add_argument("--kernels-only", action="store_true", help="skip the whole nf_zoom_resolved (for a rocprofv3 --kernel-trace --stats run)")
ap.add_argument("--out", default=os.path.join("profiles", "zoom_resolved.json"))
a = ap.parse_args()
rows = []
r1, copy = kernel_case("128cube_rt0p0_refine2", 128, 0, 2, (2, 2, 2))
rows.append(r1)
rows.append(kernel_case("64cube_rt1p1_refine2", 64, 1, 2, (2, 2, 2), copy)[0])
doc = dict(copy_gbps=copy, kernels=rows)
if not a.kernels_only:
    doc["zoom_resolved_128cube_to_256cube"] = whole(128, (2, 2, 2))
with open(a.out, "w") as fh:
    json.dump(doc, fh, indent=1)
print(json.dumps(doc))
