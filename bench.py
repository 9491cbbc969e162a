#!/usr/bin/env python3
"""bench.py -- outer power-iterations per second of the multigroup k-eigenvalue solve (BASELINE.json metric).

Workload (config.workload): IAEA-3D core resampled on a uniform n^3 mesh (default 256^3 = BASELINE configs[3] /
SURVEY C4; fits one MI355X), 2 groups, RT0-P0, six Dirichlet sides, FULL Schur path exactly as the reference
drivers run it (unpreconditioned CG to 1e-4 per group, Chebyshev-accelerated power iteration).
A "step" is one outer power iteration (fission source, ng group solves, k update, normalise, Chebyshev).
Inputs are uploaded and the line systems factored before the timed region; the timed region is K outer
iterations bracketed by barrier + device synchronize; value = K / max-over-ranks time.

A plain run sets up, warms up, times the K steps, writes --dump-outputs if given and prints the JSON line.  The
extras below take runs of their own and come with --full only (--no-converge / --no-parity / --no-small / --no-c5 /
--cpu-sample-iters 0 switch single ones off again):
  roofline      dominant kernel of the hot path (slowest Schur-apply direction pass): algorithmic bytes per
                launch / mean launch duration measured with HIP events on the solver's stream inside the timed
                region (DESIGN.md "Algorithmic bytes"); peak 8.0 TB/s.
  cpu_baseline  the CPU oracle (oracle/nf_oracle.c, 1 core, kind "port") timed on a bounded sample of the same
                workload: a fixed number of CG iterations on the same n^3 operator, extrapolated with the CG
                counts of the timed GPU steps.  Rank 0, N=1 only.
  converged     untimed converged solve with the drivers' settings (k-eff, pcm); other_configs, higher_order, parity,
                parity_at_bench_size, c5_single_gpu: the small BASELINE configs, an RT1-P1 throughput figure, parity probes
                against the oracle and BASELINE config 4 on this one GPU.

--dump-outputs DIR writes what the timed path computed in its last step, for two builds to be compared output by output:
  keff.npy      (1,) float64, k-eff after the timed steps
  phi.npy       (ng, M) float64, the scalar flux of every group at M cells: all cells (z-major, then y, then x) when they fit
                in DUMP_BYTES, else a sorted sample drawn with the fixed seed DUMP_SEED, the same on every run with the same --n
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
DUMP_BYTES = 16 << 20            # --dump-outputs: size cap of phi.npy
DUMP_SEED = 20261016             # --dump-outputs: seed of the cell sample


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=int(os.environ.get("NEUTFEM_BENCH_N", "256")),
                    help="cells per axis of the resampled IAEA-3D mesh (env NEUTFEM_BENCH_N: torch.distributed.run's own parser chokes on --n)")
    ap.add_argument("--case", default="iaea3d", choices=["iaea3d", "checker"])
    ap.add_argument("--groups", type=int, default=8, help="groups of the synthetic checkerboard case")
    ap.add_argument("--cpu-sample-iters", type=int, default=12, help="CG iterations timed on the CPU oracle (0 = skip)")
    ap.add_argument("--no-converge", action="store_true", help="skip the untimed converged solve (k-eff, pcm)")
    ap.add_argument("--no-parity", action="store_true", help="skip the small-mesh GPU-vs-oracle parity probe")
    ap.add_argument("--no-small", action="store_true", help="skip the small BASELINE configs (0-2)")
    ap.add_argument("--no-c5", action="store_true", help="skip the extra line for BASELINE config 4 (synthetic 512^3 x 8 groups on this one GPU)")
    ap.add_argument("--cg-tol", type=float, default=1e-4, help="relative CG tolerance of the timed steps (the drivers' 1e-4 is the headline; tighter values are a "
                    "diagnostic: at 1e-4 one more or fewer CG iteration of a solve at the stopping threshold moves k by ~1e-9)")
    ap.add_argument("--loopback-slabs", type=int, default=1, help="z-slabs per process (>1: exercise the slab path on one GPU)")
    ap.add_argument("--full", action="store_true", help="also measure the extras (roofline, converged solve, small configs, higher orders, CPU baseline, "
                    "parity probes, C5); off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write k-eff and the flux (a fixed sample of it on big meshes) after the timed steps as DIR/<name>.npy")
    ap.add_argument("--watchdog-s", type=float, default=float(os.environ.get("NEUTFEM_WATCHDOG_S", "300")),
                    help="multi-rank runs: exit non-zero when no outer iteration completes within this many seconds (a peer is gone or stuck)")
    return ap.parse_args()


class Watchdog:
    """Per-rank guard of a multi-rank run: a daemon thread polls nf_progress (outer iterations completed by the running solve) and ends
    THIS process with exit code 3 -- a fresh exit, never a re-exec of a process that has touched the GPU -- when the count has not
    moved for `limit` seconds while a solve is armed.  torchrun then tears the other ranks down; with the library's own collective
    timeout (NEUTFEM_COMM_TIMEOUT_S) no rank can sit in a collective for ever because one peer died."""

    def __init__(self, solver, limit, rank):
        import threading
        self.s, self.limit, self.rank, self.armed, self.stop = solver, limit, rank, False, False
        self.t = threading.Thread(target=self.run, daemon=True); self.t.start()

    def arm(self, on):
        self.last, self.t0, self.armed = -1, time.monotonic(), on

    def run(self):
        while not self.stop:
            time.sleep(min(2.0, max(0.05, self.limit / 10.0)))
            if not self.armed:
                continue
            try:
                n = self.s.progress()
            except Exception:
                continue
            if n != self.last:
                self.last, self.t0 = n, time.monotonic()
            elif time.monotonic() - self.t0 > self.limit:
                print(f"[bench watchdog] rank {self.rank}: no outer iteration completed for {self.limit:.0f} s (stuck at {n}): exiting", file=sys.stderr, flush=True)
                os._exit(3)


def dump_outputs(d, s, k, N, nxy, k0, ng, dist):
    """--dump-outputs: keff.npy and phi.npy (see the module docstring).  Every rank takes its own planes' share of the cell sample, the
    shares meet in a sum over ranks (each entry has one owner, the others add zero) and rank 0 writes."""
    per_group = DUMP_BYTES // (8 * ng)
    idx = np.arange(N) if N <= per_group else np.sort(np.random.default_rng(DUMP_SEED).choice(N, per_group, replace=False))
    phi = (s.get_phi_local() if hasattr(s, "get_phi_local") else s.get_phi()).reshape(ng, -1)
    off = k0 * nxy                                              # global index of this rank's first cell
    mine = (idx >= off) & (idx < off + phi.shape[1])
    part = np.zeros((ng, idx.size))
    part[:, mine] = phi[:, idx[mine] - off]
    if dist is not None:
        import torch
        t = torch.from_numpy(part); dist.all_reduce(t, op=dist.ReduceOp.SUM); part = t.numpy()
    if int(os.environ.get("RANK", "0")) == 0:
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "keff.npy"), np.array([k], dtype=np.float64))
        np.save(os.path.join(d, "phi.npy"), part)


def make_solver(case, device):
    from neutfem_amd.capi import HipSolver
    s = HipSolver(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"], device)
    s.set_linear_solver(6)                                      # BICGSTAB, as every reference driver
    for a, t in case["bc"]:
        s.set_bc(a, t)
    s.upload_xs(case["D"], case["SigR"], case["NSF"], case["Chi"], case["SigS"])
    s.build()
    return s


def make_oracle(case):
    from oracle.oracle import OracleNeutFEM
    o = OracleNeutFEM(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], case["z_breaks"])
    o.set_linear_solver(6)
    for a, t in case["bc"]:
        o.set_bc(a, t, 0.0)
    o.get_D()[...] = case["D"]; o.get_SigR()[...] = case["SigR"]; o.get_NSF()[...] = case["NSF"]
    o.get_Chi()[...] = case["Chi"]; o.get_SigS()[...] = case["SigS"]
    o.BuildMatrices()
    return o


def algorithmic_bytes(dim, N, nJd):
    """one Schur apply = 24 N + 40 n_J bytes; a direction pass gets its faces' 40 n_J,d plus an
    equal share of the 24 N (x read, y write, C diagonal)."""
    return 24.0 * N / dim + 40.0 * nJd


def small_configs(device):
    """BASELINE configs 0-2 as the reference drivers run them (tests/<case>/<case>.py: set_tol(1e-5,1e-4,1e-4,200,1000),
    coarse init): whole SolveKeff wall time -> outer iterations/s, k-eff, and the pcm distance to the CPU oracle on the same
    input (inputs: tests/golden/inputs_*.npz, captured from the drivers)."""
    import numpy as _np
    from neutfem_amd.capi import HipSolver
    from oracle.oracle import OracleNeutFEM
    res = []
    gold = os.path.join(ROOT, "tests", "golden")
    for label, name, rt, coarse, diag in [("config0 IAEA-2D 38x38 2g RT0-P0 (full Schur path)", "iaea2d", 0, True, False),
                                          ("config1 IAEA-3D 38x38x19 2g RT0-P0 (full Schur path, as the driver runs it)", "iaea3d", 0, True, False),
                                          ("config1 IAEA-3D 38x38x19 2g RT0-P0 (diagonal-Schur fast path)", "iaea3d", 0, False, True),
                                          ("config2 KOEBERG-2D 34x34 4g RT1-P1", "koeberg2d", 1, True, False)]:
        z = _np.load(os.path.join(gold, f"inputs_{name}.npz"))
        ng = int(z["ng"]); f = [int(v) for v in z["coarse_factors"]]
        def setup(obj, hip):
            obj.set_linear_solver(6)
            for at, ty in zip(z["bc_attr"], z["bc_type"]):
                obj.set_bc(int(at), int(ty)) if hip else obj.set_bc(int(at), int(ty), 0.0)
        s = HipSolver(rt, rt, ng, z["x_breaks"], z["y_breaks"], z["z_breaks"], device)
        setup(s, True); s.upload_xs(z["D"], z["SigR"], z["NSF"], z["Chi"], z["SigS"]); s.build()
        s.set_tol(1e-5, 1e-4, 1e-4, 200, 1000)
        s.solve_keff(coarse, f, diag)                              # warm-up (clocks, allocations)
        best = 1e9
        for _ in range(3):
            s.reset_flux(); t0 = time.perf_counter(); k, n = s.solve_keff(coarse, f, diag); best = min(best, time.perf_counter() - t0)
        h = s.history()
        path = {0: "host-driven outer loop", 1: "diagonal device loop", 2: "resident one-workgroup kernel", 3: "one-XCD kernel"}.get(int(s.info("last_path")), "?")
        o = OracleNeutFEM(rt, rt, ng, z["x_breaks"], z["y_breaks"], z["z_breaks"]); setup(o, False)
        o.get_D()[...] = z["D"]; o.get_SigR()[...] = z["SigR"]; o.get_NSF()[...] = z["NSF"]; o.get_Chi()[...] = z["Chi"]; o.get_SigS()[...] = z["SigS"]
        o.BuildMatrices(); o.set_tol(1e-5, 1e-4, 1e-4, 200, 1000)
        tcpu = 1e9
        for _ in range(2):
            o.reset_flux(); t0 = time.perf_counter(); ko = o.SolveKeff(coarse, f if coarse else [], diag); tcpu = min(tcpu, time.perf_counter() - t0)
        pg, po = s.get_phi().ravel(), o.phi_dofs().ravel()
        ho = o.history()
        res.append(dict(config=label, cells=int(s.ne), path=path, outers=int(n), coarse_outers=int(h["coarse_outer"]), cg_iterations=int(h["cg"].sum()),
                        outers_oracle=int(ho["n_outer"]), cg_iterations_oracle=int(ho["cg"].sum()),
                        flux_rel_l2_vs_oracle=float(_np.linalg.norm(pg - po) / _np.linalg.norm(po)),
                        solve_ms=round(best * 1e3, 2), outer_iters_per_s=round(n / best, 1), keff=k, keff_oracle=ko,
                        pcm_vs_oracle=round(1e5 * abs(k - ko) / ko, 4), pcm_vs_literature=round(1e5 * (1 / float(z["kref"]) - 1 / k), 1),
                        cpu_oracle_ms=round(tcpu * 1e3, 1)))
        s.close()
    return res


def higher_order_throughput(device, n=128, rt=1):
    """A throughput number for the higher orders at a size where the chip is busy (KOEBERG's 1 156 cells only show
    latency): one Schur apply y = S_0 x of IAEA-3D resampled to n^3 with RT1-P1, timed back to back with HIP events (nf_time_schur_apply),
    in algorithmic bytes by SURVEY 8(d)'s rule for RT1+ / P1+: 24 n_phi + 40 n_J with the bubble DOFs in n_J (3D RT1: 4 DOFs per face,
    4 interior per cell and direction; P1: 8 moments per cell) -- 1 148 B per cell.  What the kernels really move is less: the line
    factors are shared by the transverse modes and the bubbles are condensed per cell, so this figure can exceed what
    the same bytes would give on a kernel that stored a factor per face DOF."""
    from neutfem_amd import cases
    from neutfem_amd.capi import HipSolver
    c = cases.iaea3d_resampled(n)
    s = HipSolver(rt, rt, c["ng"], c["x_breaks"], c["y_breaks"], c["z_breaks"], device)
    s.set_linear_solver(6)
    for at, ty in c["bc"]:
        s.set_bc(at, ty)
    s.upload_xs(c["D"], c["SigR"], c["NSF"], c["Chi"], c["SigS"]); s.build()
    ms = s.time_schur_apply(0, 20)
    per_dir = {}
    for nm in ("schur_x", "schur_y", "schur_z"):
        cnt, tot = s.profile(nm)
        if cnt:
            per_dir[nm] = round(tot / cnt, 4)
    alg = 24.0 * s.n_phi + 40.0 * s.n_J
    res = dict(workload=f"IAEA-3D resampled {n}^3 RT{rt}-P{rt}, one Schur apply of group 0", cells=int(s.ne), n_phi=int(s.n_phi), n_J=int(s.n_J),
               apply_ms=round(ms, 4), pass_ms=per_dir, alg_bytes=alg, alg_bytes_per_cell=round(alg / s.ne, 1), achieved_GBps=round(alg / (ms * 1e-3) / 1e9, 1),
               frac_of_8TBps=round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
    s.close()
    return res


def split_planes(nz, parts):
    """contiguous z-plane ranges, as even as possible"""
    cuts = [round(i * nz / parts) for i in range(parts + 1)]
    return [(cuts[i], cuts[i + 1]) for i in range(parts)]


def note(msg):
    """progress line on stderr (long set-ups must not look hung)"""
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def launch_ranks(a):
    """`python bench.py --gpus N` (N > 1) outside a launcher: start N fresh ranks the way the driver does (python -m torch.distributed.run,
    one process per GPU) and hand back their exit code.  This parent never touches the GPU -- no HIP call, no library load --: it relays
    the children's output (rank 0's one JSON line on stdout) and exits with their code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    argv, skip = [], False
    for tok in sys.argv[1:]:                                     # torch.distributed.run's own parser takes `--n` for `--nnodes`: the mesh size travels in the environment
        if skip:
            skip = False
        elif tok == "--n":
            skip = True
        elif not tok.startswith("--n="):
            argv.append(tok)
    env = dict(os.environ, NEUTFEM_BENCH_N=str(a.n))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    print(f"[bench] --gpus {a.gpus} without a launcher environment: starting {a.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def main():
    a = parse()
    # the rank count is what --gpus says, and the launcher must agree: a run that quietly used another number of ranks would print a
    # well-formed line for the wrong N
    if a.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        raise SystemExit(launch_ranks(a))
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        print(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks: refusing to run (start it as `python bench.py --gpus {a.gpus}` "
              f"or `python -m torch.distributed.run --nproc-per-node {a.gpus} bench.py --gpus {a.gpus}`)", file=sys.stderr, flush=True)
        raise SystemExit(2)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    local = int(os.environ.get("NEUTFEM_FORCE_DEVICE", local))   # tests: several ranks on the one GPU of the box (tests/test_gpu_multiproc.py)
    from neutfem_amd import capi, cases                       # loads libneutfem_hip.so (and with it the ROCm HIP runtime) first
    if capi.device_count() <= 0:
        raise SystemExit("bench.py: no HIP device visible -- the hot path has no CPU fallback")
    dist = None
    if world > 1:
        # torch.distributed is plumbing only: rendezvous, barrier and the max-over-ranks of the timing (gloo, CPU).
        # The data path (interface planes, dot products) goes over RCCL inside libneutfem_hip.so.
        import torch
        import torch.distributed as dist_mod
        dist_mod.init_process_group("gloo")
        dist = dist_mod
    nz = a.n
    slabs_total = world * a.loopback_slabs
    if slabs_total > 1:
        # every rank builds only its own z-planes of the XS
        allp = split_planes(nz, slabs_total)
        mine = allp[rank * a.loopback_slabs:(rank + 1) * a.loopback_slabs]
        k0, k1 = mine[0][0], mine[-1][1]
        if a.case == "iaea3d":
            case = cases.iaea3d_resampled(a.n, z_range=(k0, k1)); zb_full = np.linspace(0.0, 380.0, nz + 1)
        else:
            case = cases.synthetic_checkerboard(a.n, a.groups, z_range=(k0, k1)); zb_full = case["z_breaks"]
        s = capi.HipTeam(0, 0, case["ng"], case["x_breaks"], case["y_breaks"], zb_full, mine, device=local,
                         below=rank > 0, above=rank < world - 1)
        s.set_linear_solver(6)
        for at, ty in case["bc"]:
            s.set_bc(at, ty)
        s.upload_xs_global(case["D"], case["SigR"], case["NSF"], case["Chi"], case["SigS"], k_offset=k0)
        s.build()
        if world > 1:
            import torch
            idt = torch.zeros(128, dtype=torch.uint8)
            if rank == 0:
                idt = torch.frombuffer(bytearray(capi.HipTeam.unique_id()), dtype=torch.uint8).clone()
            dist.broadcast(idt, 0)
            s.comm_init(bytes(idt.numpy().tobytes()), world, rank)
        comm_ranks, transport = s.comm_info()
        if world > 1 and comm_ranks not in (world, -1):
            raise SystemExit(f"bench.py: rank {rank}: the communicator counts {comm_ranks} ranks, the launcher {world}")
        head = s.head
        N_local = sum(x.ne for x in s.slabs); ng, dim = head.ng, head.dim
        N = a.n * a.n * nz
        nxy = head.nx * head.ny
    else:
        note(f"building case {a.case} n={a.n}")
        case = cases.iaea3d_resampled(a.n) if a.case == "iaea3d" else cases.synthetic_checkerboard(a.n, a.groups)
        note("uploading + BuildMatrices")
        s = make_solver(case, local)
        note("built")
        head = s
        comm_ranks, transport = 0, ""
        N, ng, dim = s.ne, s.ng, s.dim
        k0, nxy = 0, s.nx * s.ny
    TOL_FLUX, MAX_INNER = a.cg_tol, (1000 if a.cg_tol >= 1e-4 else 20000)   # drivers: set_tol(1e-5,1e-4,1e-4,200,1000)
    if a.case == "checker":                                     # fixed work, exactly 50 CG iterations per group solve
        TOL_FLUX, MAX_INNER = 0.0, 50

    def barrier():
        if dist is not None:
            dist.barrier()
        head._chk(head.L.nf_synchronize(head.h))               # stream + device synchronize

    dog = Watchdog(head, a.watchdog_s, rank) if world > 1 else None
    if dog:
        dog.arm(True)

    # warm-up: W untimed outer iterations (also warms caches / clocks); state carries over like the reference
    if a.warmup > 0:
        s.set_tol(0.0, TOL_FLUX, 1e-4, a.warmup, MAX_INNER)
        s.solve_keff()
    s.set_tol(0.0, TOL_FLUX, 1e-4, a.steps, MAX_INNER)          # tol_keff = 0 -> exactly K outers
    s.profile_reset()
    note("timed steps")
    # profiled on every run, not only --full's: the event timing of every 8th apply is part of the timed path the headline has always measured
    barrier(); t0 = time.perf_counter()
    k_timed, n_out = s.solve_keff(profile=True)
    barrier(); dt = time.perf_counter() - t0
    assert n_out == a.steps
    if dist is not None:
        import torch
        t = torch.tensor([dt], dtype=torch.float64); dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
    hist = s.history()
    cg_per_outer = float(hist["cg"].sum()) / a.steps
    if a.dump_outputs:
        note(f"writing outputs to {a.dump_outputs}")
        dump_outputs(a.dump_outputs, s, k_timed, N, nxy, k0, ng, dist)

    roofline = None
    if a.full:
        # roofline of the dominant kernel (slowest direction pass of the Schur apply)
        # per-launch figures refer to what ONE rank's launches process (its own planes)
        if slabs_total > 1:
            nzl = max(x.nz for x in s.slabs); nxl, nyl = head.nx, head.ny
            Nl = nxl * nyl * nzl
        else:
            nzl, nxl, nyl, Nl = s.nz, s.nx, s.ny, N
        nJd = {0: (nxl + 1) * nyl * nzl, 1: nxl * (nyl + 1) * nzl, 2: nxl * nyl * (nzl + 1)}
        kern = {0: "k_schur_x<2,NCH,VEC>", 1: "k_schur_s<SEG,1> / k_schur_c<1> (y lines)", 2: "k_schur_s<SEG,2> / k_schur_c<2> (z lines)"}
        passes = []
        # fused CG (undivided RT0-P0 mesh): the x pass also carries x_sol += alpha p and p = r + beta p of the previous
        # iteration (read r, x_sol; write p, x_sol = 32 B/cell on top of the apply; p itself is read once for both jobs) on every
        # CG iteration but the first of a group solve
        n_solves = hist["cg"].size
        fused_bytes = 32.0 * Nl * (1.0 - n_solves / max(float(hist["cg"].sum()), 1.0)) if slabs_total == 1 else 0.0
        for d, nm in enumerate(["schur_x", "schur_y", "schur_z"][:dim]):
            c, ms = s.profile(nm)
            if c:
                per = a.loopback_slabs                                  # launches per timed pass (one per local slab)
                passes.append(dict(name=nm, kernel=kern[d], launches=c * per, avg_ms=ms / c / per,
                                   alg_bytes=algorithmic_bytes(dim, Nl, nJd[d]) + (fused_bytes if d == 0 else 0.0)))
        if not passes:
            # small / medium meshes run the three passes of an apply as ONE launch (k_apply3): no per-direction timing exists; the
            # dominant kernel is that launch, charged with the whole apply (+ the fused CG vector updates)
            c, ms = s.profile("schur_apply")
            passes.append(dict(name="schur_apply", kernel="k_apply3 (x, y, z passes of one Schur apply in one launch)", launches=max(c, 1), avg_ms=ms / max(c, 1),
                               alg_bytes=24.0 * Nl + 40.0 * sum(nJd[d] for d in range(dim)) + fused_bytes))
        dom = max(passes, key=lambda p: p["avg_ms"])
        # HBM traffic of that kernel from the PMC counters.  Counters cannot be read inside this process: the figure comes from separate
        # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command (profiles/collect.sh; gfx950 x2 read correction), stored per
        # cell in a committed profile; `traffic_source` says which one, so a stale profile is visible.  null when no profile matches the run.
        traffic, traffic_source = None, None
        try:
            import re
            def _tag(fn):                                               # r02_a_... -> (2, 1, "a"); r03_zz_... -> (3, 2, "zz"); r01_... -> (1, 0, "")
                m = re.match(r"r(\d+)_(?:([a-z]+)_)?", fn)
                return (int(m.group(1)), len(m.group(2) or ""), m.group(2) or "") if m else (0, 0, "")
            sys.path.insert(0, os.path.join(ROOT, "profiles"))
            from summarize import kernel_source_hash
            cur = kernel_source_hash()
            cands = sorted((f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc_traffic_256cube.json")), key=_tag)
            def _load(fn):
                with open(os.path.join(ROOT, "profiles", fn)) as f:
                    return json.load(f)
            fresh_ones = [f for f in cands if _load(f).get("kernel_source_sha256") == cur]     # the profile of THESE kernels if there is one, else the latest
            prof = fresh_ones[-1] if fresh_ones else cands[-1]
            pj = _load(prof)
            pmc = pj["kernels"]
            pat = {"schur_x": r"k_schur_x<", "schur_y": r"k_schur_[sc]<(\d+, )?1,", "schur_z": r"k_schur_[sc]<(\d+, )?2,", "schur_apply": r"k_apply3<"}[dom["name"]]
            hits = [k for k in pmc if re.match(pat, k)]
            key = max(hits, key=lambda k: pmc[k].get("dispatches", 0)) if hits else None
            fresh = pj.get("kernel_source_sha256") == cur
            if os.environ.get("NEUTFEM_OPTS"):
                traffic_source = dict(file="profiles/" + prof, stale=True, why="NEUTFEM_OPTS overrides launch parameters: this is not the run that was profiled: traffic = null")
            elif a.n == 256 and a.case == "iaea3d" and slabs_total == 1 and key in pmc and not fresh:
                # the newest committed profile was taken with other kernel sources: no figure rather than a stale one
                traffic_source = dict(file="profiles/" + prof, stale=True, why="the kernels or their launch logic changed since this profile was collected (sha256 of nf_kernels.h + nf_assembly.h + neutfem_hip.hip differs): traffic = null")
            elif a.n == 256 and a.case == "iaea3d" and slabs_total == 1 and key in pmc:
                traffic = round(pmc[key]["hbm_bytes_per_cell"] * N)
                traffic_source = dict(file="profiles/" + prof, kernel=key, measured_in_this_run=False, kernel_sources_match=True,
                                      how="separate rocprofv3 --pmc passes (FETCH_SIZE x2 gfx950 correction, WRITE_SIZE) of `python bench.py`; bytes per cell x cells of this run",
                                      tag=pj.get("tag"), commit=pj.get("commit"))
        except Exception:
            traffic, traffic_source = None, None
        ach = dom["alg_bytes"] / (dom["avg_ms"] * 1e-3) / 1e9
        ca, cms = s.profile("schur_apply")
        apply_bytes = (24.0 * Nl + 40.0 * sum(nJd[d] for d in range(dim))) * a.loopback_slabs + fused_bytes
        roofline = dict(bound="hbm", kernel=dom["kernel"], achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=round(ach / HBM_PEAK_GBS, 4), traffic=traffic, traffic_source=traffic_source, launches=dom["launches"], avg_ms=round(dom["avg_ms"], 4),
                        event_sampling="HIP events bracket every 8th Schur apply of the timed steps (nf_set_option prof_every): an event record keeps "
                                       "neighbouring launches from going out back to back, 8 records per apply cost 6 % of a CG iteration at 256^3",
                        alg_bytes_per_launch=dom["alg_bytes"], fused_cg_vector_bytes_in_x_pass=fused_bytes,
                        schur_apply=dict(avg_ms=round(cms / max(ca, 1), 4), alg_bytes=apply_bytes,
                                         achieved=round(apply_bytes / (cms / max(ca, 1) * 1e-3) / 1e9, 1),
                                         frac=round(apply_bytes / (cms / max(ca, 1) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)),
                        passes=[dict(name=p["name"], avg_ms=round(p["avg_ms"], 4),
                                     achieved=round(p["alg_bytes"] / (p["avg_ms"] * 1e-3) / 1e9, 1)) for p in passes])
        # the same fraction against what a plain streaming copy reaches on this very GPU ("of spec" and "of measured copy")
        copy_gbs = head.time_device_copy(1 << 30, 20)
        roofline["measured_copy"] = dict(GBps=round(copy_gbs, 1), frac_of_copy=round(ach / copy_gbs, 4),
                                         schur_apply_frac_of_copy=round(roofline["schur_apply"]["achieved"] / copy_gbs, 4),
                                         note="best of plain / nontemporal copy kernels and hipMemcpyDtoD, 1 GiB, read + write counted; "
                                              "fractions use ALGORITHMIC bytes, which exceed the HBM traffic (PMC) of these kernels")
        if traffic:
            tg = traffic / (dom["avg_ms"] * 1e-3) / 1e9
            roofline["measured_copy"].update(hbm_traffic_GBps=round(tg, 1), hbm_traffic_frac_of_copy=round(tg / copy_gbs, 4))

    out = dict(metric="outer power-iters/sec (IAEA-3D RT0-P0 k-eigenvalue solve)" if a.case == "iaea3d" else "outer power-iters/sec (synthetic checkerboard RT0-P0 k-eigenvalue solve, fixed work)", value=round(a.steps / dt, 4), unit="outer-iters/s",
               n_gpus=world, rccl_ranks=(comm_ranks if world > 1 else 1), transport=(transport if world > 1 else "none (one rank: no collective on the data path)"),
               steps=a.steps, warmup=a.warmup, ms_per_step=round(dt / a.steps * 1e3, 3), higher_is_better=True,
               scaling="strong", vs_baseline=None, dtype="f64", data="synthetic",
               config=dict(workload=(f"IAEA-3D resampled {a.n}x{a.n}x{nz} RT0-P0 2g" if a.case == "iaea3d" else case["name"]) +
                           (f", full Schur path, CG tol {a.cg_tol:g}, Chebyshev" if a.case == "iaea3d" else ", full Schur path, exactly 50 CG iterations per group solve, Chebyshev"),
                           cells=int(N), groups=int(ng),
                           cg_iters_per_outer=round(cg_per_outer, 1),
                           parallelism=f"{world} process(es) x {a.loopback_slabs} z-slab(s) each; RCCL: interface planes + scalar all-reduces"),
               keff_after_timed_steps=k_timed)
    if roofline is not None:
        out["roofline"] = roofline

    # ---- untimed: converged k-eff at full size with the drivers' settings (coarse-mesh start included), on every N: the
    # pcm half of BASELINE's metric.  Collective on a decomposed run (all ranks solve, rank 0 reports).
    if a.full and not a.no_converge and a.case == "iaea3d":
        note("converged solve (untimed)")
        s.reset_flux()
        s.set_tol(1e-5, 1e-4, 1e-4, 200, 1000)
        t1 = time.perf_counter(); kc, nc = s.solve_keff(True, case["coarse_factors"]); tcv = time.perf_counter() - t1
        out["converged"] = dict(keff=kc, outers=nc, seconds=round(tcv, 2), kref_literature=1.029096,
                                pcm_vs_kref=round(1e5 * (1 / 1.029096 - 1 / kc), 2),
                                note="reference driver settings: set_tol(1e-5,1e-4,1e-4,200,1000), coarse init; the resampled 1.48 cm mesh does not "
                                     "align with the 20 cm assemblies, hence the offset from the literature value (physics sanity only)")
        # k of the undivided (one-GPU) solve of the same workload, for the decomposed runs to be compared with: taken from a
        # previous N = 1 line of this script -- the one this box wrote (gpurun_out/bench_keff_n1.json) or, failing that, the newest
        # committed profiles/r*_bench_256cube.json.  Never a literal in the source; at N = 1 nothing is compared (it would be a self-comparison).
        wl = out["config"]["workload"]
        n1_file = os.path.join(ROOT, "gpurun_out", "bench_keff_n1.json")
        if rank == 0 and slabs_total == 1:
            try:
                os.makedirs(os.path.dirname(n1_file), exist_ok=True)
                with open(n1_file, "w") as f:
                    json.dump(dict(workload=wl, keff=kc, outers=nc), f)
            except OSError:
                pass
        elif rank == 0:
            ref = None
            try:
                with open(n1_file) as f:
                    j = json.load(f)
                if j["workload"] == wl:
                    ref = (j["keff"], "gpurun_out/bench_keff_n1.json (N=1 run on this box)")
            except (OSError, ValueError, KeyError):
                pass
            if ref is None:
                for fn in sorted((f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_bench_256cube.json")), reverse=True):
                    try:
                        with open(os.path.join(ROOT, "profiles", fn)) as f:
                            j = json.loads(f.read().strip().splitlines()[-1])
                        if j["n_gpus"] == 1 and j["config"]["workload"] == wl and "converged" in j:
                            ref = (j["converged"]["keff"], "profiles/" + fn); break
                    except (OSError, ValueError, KeyError):
                        continue
            if ref is not None:
                out["converged"].update(keff_one_gpu=ref[0], keff_one_gpu_source=ref[1], pcm_vs_one_gpu=round(1e5 * abs(kc - ref[0]) / ref[0], 4))
    # ---- the other BASELINE configs (small, latency bound): timed with the reference drivers' own settings; before the big CPU
    # baseline, whose 10 GB of host arrays leave the allocator in a state that distorts millisecond-scale CPU timings
    if a.full and rank == 0 and slabs_total == 1 and not a.no_small:
        note("small BASELINE configs")
        out["other_configs"] = small_configs(local)
    if a.full and rank == 0 and slabs_total == 1 and not a.no_small and a.case == "iaea3d":
        note("higher-order throughput (RT1-P1 Schur apply at 128^3)")
        try:
            out["higher_order"] = higher_order_throughput(local)
        except Exception as e:                                       # an extra must never cost the headline line
            out["higher_order"] = dict(error=str(e)[:300])
    if a.full and rank == 0 and slabs_total == 1:
        # ---- CPU baseline: bounded sample of the same workload on the host (1 core) -------------------------------
        if a.cpu_sample_iters > 0:
            note("CPU baseline (oracle, 1 core)")
            o = make_oracle(case)
            rhs = np.abs(np.random.default_rng(0).standard_normal(o.n_phi))
            o.set_tol(0.0, 0.0, 1e-4, 1, a.cpu_sample_iters)    # CG tol 0 -> exactly cpu_sample_iters iterations
            # (i) CG iterations alone: Schur apply + the vector updates of src/solvers.cpp:577-636, no J back-solve
            t1 = time.perf_counter(); phi_c, _, its = o.solve_group(0, rhs, with_J=False); tc = time.perf_counter() - t1
            per_it = tc / max(its, 1)
            # (ii) what SchurSolver::Solve adds once per group solve: J = -A^-1 B^T phi (:227-228), and, in the reference as it is
            # written, SetMatrices -> SparseLU(A_g) again for every group of every outer (:163; here a banded LDL^T, cheaper)
            o.set_tol(0.0, 0.0, 1e-4, 1, 1)
            t1 = time.perf_counter(); o.solve_group(0, rhs, with_J=False); t_one = time.perf_counter() - t1
            t1 = time.perf_counter(); o.solve_group(0, rhs, with_J=True); t_J = max(time.perf_counter() - t1 - t_one, 0.0)
            o.set_refactor_each_solve(1)
            t1 = time.perf_counter(); o.solve_group(0, rhs, with_J=False); t_fac = max(time.perf_counter() - t1 - t_one, 0.0)
            o.set_refactor_each_solve(0)
            sane = per_it * cg_per_outer + ng * t_J              # factor once per BuildMatrices
            faithful = sane + ng * t_fac                         # re-factor A for every group and outer
            out["cpu_baseline"] = dict(value=round(1.0 / sane, 6), unit="outer-iters/s", cores=1, kind="port", mode="ref-sane",
                                       sample=f"{its} CG iterations (Schur apply + vector updates, no J back-solve) of group 0 on the same "
                                              f"{case['name']} operator = {tc:.1f} s on one host core; one J back-solve = {t_J:.2f} s and one "
                                              f"re-factorisation of A_g = {t_fac:.2f} s timed separately; an outer iteration = "
                                              f"{cg_per_outer:.0f} CG iterations (measured in the timed GPU steps) + {ng} J back-solves"
                                              f" (+ {ng} factorisations in ref-faithful mode)",
                                       sec_per_cg_iteration=round(per_it, 4), sec_per_J_backsolve=round(t_J, 3), sec_per_factorisation=round(t_fac, 3),
                                       ref_sane=dict(value=round(1.0 / sane, 6), sec_per_outer=round(sane, 1), what="A factored once per BuildMatrices"),
                                       ref_faithful=dict(value=round(1.0 / faithful, 6), sec_per_outer=round(faithful, 1),
                                                         what="A re-factored for every group of every outer as src/solvers.cpp:163 does "
                                                              "(banded LDL^T instead of Eigen's general SparseLU: favourable to the reference)"))
            # operator parity at the BENCHMARK size: one Schur apply of the GPU against the oracle on the same vector
            if a.case == "iaea3d" and not a.no_parity:
                xr = np.random.default_rng(1).standard_normal(o.n_phi)
                yo_, yg_ = o.schur_apply(0, xr), s.schur_apply(0, xr)
                out["parity_at_bench_size"] = dict(what="S_0 x on one random vector, GPU vs CPU oracle, full benchmark mesh", cells=int(N),
                                                   max_rel_err=float(np.abs(yg_ - yo_).max() / np.abs(yo_).max()))
            del o
        # ---- small-mesh parity probe against the oracle (same code path, tight tolerances) ---------------------
        if not a.no_parity and a.case == "iaea3d":
            small = cases.iaea3d_resampled(38, 19)
            sp, op = make_solver(small, local), make_oracle(small)
            tol = (1e-11, 1e-11, 1e-11, 2000, 2000)
            sp.set_tol(*tol); op.set_tol(*tol)
            kg, _ = sp.solve_keff(); ko = op.SolveKeff()
            pg, po = sp.get_phi().ravel(), op.phi_dofs().ravel()
            out["parity"] = dict(mesh="38x38x19", keff_gpu=kg, keff_oracle=ko, pcm=round(1e5 * abs(kg - ko) / ko, 6),
                                 flux_rel_l2=float(np.linalg.norm(pg - po) / np.linalg.norm(po)))
            sp.close()
    if dog:
        dog.arm(False); dog.stop = True
    s.close()
    # ---- BASELINE configs[4] (synthetic 512^3, 8 groups, fixed work of 50 CG iterations per group solve) on this ONE GPU,
    # so that the driver's run times it too.  Needs ~165 GB of HBM and ~75 GB of host memory for the case arrays: skipped when the
    # box has less.  The headline (`value`, `config.workload`) stays the IAEA-3D 256^3 case above.
    if a.full and rank == 0 and world == 1 and slabs_total == 1 and a.case == "iaea3d" and a.n == 256 and not a.no_c5:
        try:
            free_b, _tot = capi.mem_info(local)
            with open("/proc/meminfo") as f:
                avail_kb = next(int(l.split()[1]) for l in f if l.startswith("MemAvailable"))
            if free_b >= 180e9 and avail_kb * 1024 >= 110e9:
                note("C5: synthetic 512^3 x 8 groups (generation + upload + BuildMatrices take ~20 s)")
                c5 = cases.synthetic_checkerboard(512, 8)
                s5 = make_solver(c5, local)
                del c5["SigS"]
                s5.set_tol(0.0, 0.0, 1e-4, 1, 50); s5.solve_keff()                      # warm-up outer
                s5.set_tol(0.0, 0.0, 1e-4, 2, 50); s5.profile_reset()
                s5._chk(s5.L.nf_synchronize(s5.h)); t1 = time.perf_counter()
                k5, n5 = s5.solve_keff(profile=True)
                s5._chk(s5.L.nf_synchronize(s5.h)); t5 = time.perf_counter() - t1
                N5 = s5.ne; nJ5 = {0: 513 * 512 * 512, 1: 512 * 513 * 512, 2: 512 * 512 * 513}
                ps = []
                for d, nm in enumerate(["schur_x", "schur_y", "schur_z"]):
                    c, ms = s5.profile(nm)
                    if c:
                        fb = 32.0 * N5 * (1.0 - 1.0 / 50.0) if d == 0 else 0.0
                        ps.append(dict(name=nm, avg_ms=round(ms / c, 4), achieved=round((algorithmic_bytes(3, N5, nJ5[d]) + fb) / (ms / c * 1e-3) / 1e9, 1)))
                out["c5_single_gpu"] = dict(workload=c5["name"] + ", full Schur path, exactly 50 CG iterations per group solve", cells=int(N5), groups=8,
                                            steps=int(n5), value=round(n5 / t5, 4), unit="outer-iters/s", ms_per_step=round(t5 / n5 * 1e3, 1),
                                            keff_after_steps=k5, passes=ps, peak_GBps=HBM_PEAK_GBS)
                # no number without a check: (i) size-independent properties of S_g at the full 512^3 (linear, symmetric, positive) on the very
                # kernels that were timed; (ii) S_g x against the CPU oracle for all 8 groups on a 32 x 32 x 512 column of the same generator
                # (512-cell z lines: the same long-line kernel, the same segment / chunk structure along z)
                note("C5 self-check")
                rng5 = np.random.default_rng(5)
                xa, xb = rng5.standard_normal(N5), rng5.standard_normal(N5)
                par = dict(groups_checked=[0, 7])
                lin, sym, pos = 0.0, 0.0, True
                for g5 in (0, 7):
                    Sa, Sb = s5.schur_apply(g5, xa), s5.schur_apply(g5, xb)
                    Sab = s5.schur_apply(g5, 2.0 * xa - 3.0 * xb)
                    lin = max(lin, float(np.linalg.norm(Sab - (2.0 * Sa - 3.0 * Sb)) / np.linalg.norm(Sab)))
                    sym = max(sym, float(abs(xb @ Sa - xa @ Sb) / abs(xb @ Sa)))
                    pos = pos and bool(xa @ Sa > 0 and xb @ Sb > 0)
                    del Sa, Sb, Sab
                par.update(linearity_rel_l2=lin, symmetry_rel=sym, positive=pos)
                del xa, xb
                s5.close()
                col = cases.synthetic_checkerboard(512, 8, nxy=32)
                sc_, oc_ = make_solver(col, local), make_oracle(col)
                xr = np.random.default_rng(6).standard_normal(oc_.n_phi)
                par["column_32x32x512_vs_oracle_max_rel_err"] = max(float(np.abs(sc_.schur_apply(g5, xr) - oc_.schur_apply(g5, xr)).max() / np.abs(oc_.schur_apply(g5, xr)).max())
                                                                 for g5 in range(8))
                sc_.close(); del oc_
                par["ok"] = bool(lin < 1e-12 and sym < 1e-10 and pos and par["column_32x32x512_vs_oracle_max_rel_err"] < 1e-12)
                out["c5_single_gpu"]["parity"] = par
            else:
                out["c5_single_gpu"] = dict(skipped=f"needs >= 180 GB free HBM and >= 110 GB free host memory (have {free_b / 1e9:.0f} / {avail_kb * 1024 / 1e9:.0f})")
        except Exception as e:                                                          # never lose the headline line to the extra one
            out["c5_single_gpu"] = dict(error=str(e)[:300])
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
