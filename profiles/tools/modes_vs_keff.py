"""IAEA-3D resampled 256^3, 2 groups: ms per block outer of nf_solve_modes (n_modes 2, n_guard 2) against 4 x the ms per outer of
nf_solve_keff on the same handle, the achieved bytes/s of the two block kernels against nf_time_device_copy, outers to converge and the
dominance ratio, at the drivers' tolerances.  Run from the repository root on an MI355X after build(); prints progress lines and, last,
one JSON line (profiles/modes_vs_keff_256cube.json)."""
import ctypes as C
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
from neutfem_amd import cases
from neutfem_amd.capi import HipSolver, _dp

NC = int(sys.argv[1]) if len(sys.argv) > 1 else 256
case = cases.iaea3d_resampled(NC)
s = HipSolver(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], 0)
s.set_linear_solver(6)
for a, t in case["bc"]:
    s.set_bc(a, t)
s.upload_xs(case["D"], case["SigR"], case["NSF"], case["Chi"], case["SigS"]); s.build()
sync = lambda: s._chk(s.L.nf_synchronize(s.h))
TOL = (1e-5, 1e-4, 1e-4, 200, 1000)
# SolveKeff: 2 warm-up outers, then exactly 10 timed outers (tol_keff = 0), CG tol 1e-4 / 1000 as bench.py
s.set_tol(0.0, 1e-4, 1e-4, 2, 1000); s.solve_keff()
s.set_tol(0.0, 1e-4, 1e-4, 10, 1000); sync(); t0 = time.perf_counter(); k, n = s.solve_keff(); sync(); dt_k = time.perf_counter() - t0
cg_k = int(s.history()["cg"].sum())
print(f"keff: {1e3 * dt_k / n:.1f} ms per outer, {cg_k / n:.1f} CG per outer", flush=True)
s.reset_flux(); s.set_warm_state(0, 1.0)
s.set_tol(*TOL); sync(); t0 = time.perf_counter(); kc, nk = s.solve_keff(); sync(); dt_kc = time.perf_counter() - t0
print(f"keff converged: k = {kc:.8f} in {nk} outers, {dt_kc:.1f} s", flush=True)
# the block iteration: a short run and a longer one from the same start; the difference is whole block outers (start block, the
# final application to the wanted columns and the extraction cancel)
runs = {}
for mo in (2, 12):
    s.set_tol(TOL[0], TOL[1], TOL[2], mo, TOL[4]); sync(); t0 = time.perf_counter(); r = s.solve_modes(2, n_guard=2); sync()
    runs[mo] = (time.perf_counter() - t0, r)
    print(f"modes max_outer {mo}: {runs[mo][0]:.2f} s, cg {r['cg_total']}", flush=True)
ms_block = 1e3 * (runs[12][0] - runs[2][0]) / 10
cg_block = (runs[12][1]["cg_total"] - runs[2][1]["cg_total"]) / 10
s.set_tol(*TOL); sync(); t0 = time.perf_counter(); r = s.solve_modes(2, n_guard=2); sync(); dt_m = time.perf_counter() - t0
print(f"modes: {r}, {dt_m:.1f} s", flush=True)
# the two block kernels alone, through the C ABI (the call includes the reduction of the partials and the read-back of the sums)
n = int(s.ng * s.n_phi)
copy_gbps = s.time_device_copy(1 << 30, 20)
kern = {}
rng = np.random.default_rng(0)
chunk = rng.standard_normal(1 << 22)
for b, m in ((4, 2), (8, 4)):
    q, z = s.vector(n * b), s.vector(n * b)
    for v in (q, z):
        for off in range(0, n * b, chunk.size):
            cnt = min(chunk.size, n * b - off)
            s._chk(s.L.nf_memcpy_h2d(s.h, C.c_void_p(v.ptr.value + 8 * off), chunk.ctypes.data_as(C.c_void_p), 8 * cnt))
    H, G, res2 = np.empty(b * b), np.empty(b * b), np.empty(m)
    Cm = np.linalg.qr(rng.standard_normal((b, b)))[0].ravel(); Hm = 0.1 * rng.standard_normal(m * m)
    tg, tr = [], []
    for rep in range(6):
        sync(); t0 = time.perf_counter(); s._chk(s.L.nf_block_gram(s.h, b, n, q.ptr, z.ptr, _dp(H), _dp(G))); tg.append(time.perf_counter() - t0)
        sync(); t0 = time.perf_counter(); s._chk(s.L.nf_block_rotate(s.h, b, m, n, q.ptr, z.ptr, _dp(Cm), _dp(Hm), _dp(res2))); tr.append(time.perf_counter() - t0)
    tg, tr = min(tg[1:]), min(tr[1:])
    nt = (b + 3) // 4
    tile_cols = sum(8 if ti == tj else (12 if ti < tj else 8) for ti in range(nt) for tj in range(nt))
    kern[f"b{b}"] = dict(gram_ms=1e3 * tg, gram_gbps_algorithmic=2 * b * n * 8 / tg / 1e9, gram_gbps_requested=tile_cols * n * 8 / tg / 1e9,
                         rotate_ms=1e3 * tr, rotate_gbps=3 * b * n * 8 / tr / 1e9, m=m)
    print(kern[f"b{b}"], flush=True)
    q.free(); z.free()
line = dict(case=f"iaea3d_resampled_{NC}cube", cells=int(s.ne), groups=int(s.ng), tol="set_tol(1e-5,1e-4,1e-4,200,1000)", n_modes=2, n_guard=2,
            keff_ms_per_outer=1e3 * dt_k / 10, keff_cg_per_outer=cg_k / 10, keff_converged=kc,
            keff_outers_to_converge=nk, keff_wall_s=dt_kc,
            modes_ms_per_block_outer=ms_block, modes_cg_per_block_outer=cg_block, four_keff_outers_ms=4e3 * dt_k / 10,
            modes_ms_per_block_outer_at_keff_cg_rate=ms_block * (4 * cg_k / 10) / cg_block,
            modes_k=r["k"], modes_residual=r["residual"], dominance_ratio=r["dominance_ratio"], modes_outers=r["n_outer"],
            modes_converged=r["converged"], modes_cg_total=r["cg_total"], modes_wall_s=dt_m,
            block_bytes=2 * 4 * n * 8, copy_gbps=copy_gbps, kernels=kern)
print(json.dumps(line))
s.close()
