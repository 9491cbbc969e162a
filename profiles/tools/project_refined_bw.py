"""Bandwidth of k_project_refined (nf_project_flux / nf_project_power), output on the device:
  256^3 RT0-P0 x 2 groups, refine (2, 2, 2): flux (one group per call) and power;
  128^3 RT2-P2 x 2 groups, refine (3, 3, 3): flux.
Each call is bracketed by HIP events on the handle's stream after two warm-up calls (the interval also holds the call's host-side
launch latency: an upper bound of the kernel time; `rocprofv3 --kernel-trace --stats` gives the kernel alone).  Algorithmic bytes:
flux 8 N (nloc + R) per group, power 8 N (ng (nloc + 1) + R), R = rx ry rz; reported against 8 TB/s and the copy yardstick
nf_time_device_copy of the same run.  Then the pybind project_flux / project_power end to end (device-to-host copy included).
Run from the repository root on an MI355X after build(); prints one JSON line."""
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
    s.upload_xs(one, 0.05 * one, 0.02 * one, chi, np.zeros(ng * ng * N))
    del one, chi
    s.build()
    s.set_phi(np.random.default_rng(0).uniform(0.5, 2.0, (ng, N * s.n_loc)))
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


def case(name, n, rt, p, ng, r, power, copy_gbps=None):
    s = make(n, rt, p, ng)
    N, R, nloc = s.ne, r[0] * r[1] * r[2], s.n_loc
    buf = s.vector(N * R)
    ksf = np.full(ng * N, 0.3)
    kp = ksf.ctypes.data_as(C.POINTER(C.c_double))
    if power:
        call = lambda: s._chk(s.L.nf_project_power(s.h, r[0], r[1], r[2], 0, kp, buf.ptr))
        nbytes = 8 * N * (ng * (nloc + 1) + R)
    else:
        call = lambda: s._chk(s.L.nf_project_flux(s.h, r[0], r[1], r[2], 0, 0, buf.ptr))
        nbytes = 8 * N * (nloc + R)
    med, best = timed(s, call)
    if copy_gbps is None:
        copy_gbps = s.time_device_copy(1 << 30, 20)
    buf.free(); s.close()
    gbps = nbytes / (med * 1e-3) / 1e9
    return dict(case=name, cells=N, nloc=nloc, groups=ng, refine=list(r), power=power, bytes=nbytes, ms_median=med, ms_min=best,
                gbps=gbps, frac_of_8tbs=gbps / 8000.0, frac_of_copy=gbps / copy_gbps), copy_gbps


def pybind_end_to_end(n, ng, r):
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as m
    b = np.linspace(0.0, float(n), n + 1)
    s = m.NeutFEM(0, 0, ng, b, b, b)
    s.set_verbosity(m.VerbosityLevel.SILENT)
    s.get_D()[...] = 1.0; s.get_SigR()[...] = 0.05; s.get_NSF()[...] = 0.02; s.get_KSF()[...] = 0.3
    s.BuildMatrices()
    out = {}
    for name, fn in (("project_flux", s.project_flux), ("project_power", s.project_power)):
        fn(list(r))
        t0 = time.perf_counter(); a = fn(list(r)); out[name + "_s"] = time.perf_counter() - t0
        out[name + "_shape"] = list(a.shape)
        del a
    return out


rows = []
r1, copy = case("256cube_rt0p0_flux", 256, 0, 0, 2, (2, 2, 2), False)
rows.append(r1)
rows.append(case("256cube_rt0p0_power", 256, 0, 0, 2, (2, 2, 2), True, copy)[0])
rows.append(case("128cube_rt2p2_flux", 128, 2, 2, 2, (3, 3, 3), False, copy)[0])
print(json.dumps(dict(copy_gbps=copy, kernels=rows, pybind_256cube_2groups_refine2=pybind_end_to_end(256, 2, (2, 2, 2)))))
