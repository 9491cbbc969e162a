#!/usr/bin/env python3
"""Throughput of nf_solve_keff_batch against the loop of nf_solve_keff calls.

Per case -- IAEA-2D RT0-P0, KOEBERG-2D RT1-P1 -- 2 x CUs handles are built whose cross sections differ by a seeded +-1 % per assembly;
for n in {1, 8, 64, CUs, 2 CUs} the first n of them are solved from reset_flux() once by one batch call and once by n nf_solve_keff calls,
three rounds in alternating order.  Wall time, the final nf_synchronize included; the median of the rounds is reported as cases per
second, with the ratio loop / batch.  The reference drivers' tolerances (1e-5, 1e-4, 1e-4, 200, 1000).

    python profiles/tools/batch_throughput.py            # every case, each in a child process under its own time limit
    python profiles/tools/batch_throughput.py --case iaea2d

The parent process never opens the GPU: each case is one child under `timeout`, the first failure ends the run.  The table goes to
profiles/batch_throughput.txt."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = {"iaea2d": ("iaea2d", 0), "koeberg2d-rt1": ("koeberg2d", 1)}
TOL = (1e-5, 1e-4, 1e-4, 200, 1000)
OUT = os.path.join(ROOT, "profiles", "batch_throughput.txt")


def perturbed(inp, seed, amp=0.01):
    import numpy as np
    rng = np.random.default_rng(seed)
    ny, nx = inp["D"].shape[-2:]
    b = 2 if ny % 2 == 0 and nx % 2 == 0 else 1
    out = dict(inp)
    for key in ("D", "SigR", "NSF", "SigS"):
        out[key] = inp[key] * np.kron(1.0 + amp * rng.uniform(-1.0, 1.0, (ny // b, nx // b)), np.ones((b, b)))
    return out


def worker(case):
    from helpers import load_inputs, make_hip
    from neutfem_amd import capi
    name, rt = CASES[case]
    base = load_inputs(name)
    t0 = time.perf_counter()
    first = make_hip(perturbed(base, 1000), rt, rt)
    cus = first.info("compute_units")
    hs = [first] + [make_hip(perturbed(base, 1000 + i), rt, rt) for i in range(1, 2 * cus)]
    first.L.nf_synchronize(first.h)
    t_build = time.perf_counter() - t0
    for s in hs:
        s.set_tol(*TOL)
    def say(line): print(line, flush=True)                       # row by row: a case cut off by its time limit keeps what it measured
    lines = [f"{case}: {hs[0].nx} x {hs[0].ny} cells, RT{rt}-P{rt}, {hs[0].n_phi} flux DOFs per group, {cus} compute units; "
             f"{len(hs)} handles created and built in {t_build:.2f} s ({1e3 * t_build / len(hs):.2f} ms each)",
             f"{'n':>5} {'route':>10} {'batch ms':>10} {'loop ms':>10} {'batch cases/s':>14} {'loop cases/s':>13} {'loop/batch':>10}"]

    def run_batch(sub):
        for s in sub:
            s.reset_flux()
        sub[0].L.nf_synchronize(sub[0].h)
        t = time.perf_counter()
        k, no, st, res = capi.solve_keff_batch(sub)
        sub[0].L.nf_synchronize(sub[0].h)
        dt = time.perf_counter() - t
        assert not st.any(), st
        return dt, k, res

    def run_loop(sub):
        for s in sub:
            s.reset_flux()
        sub[0].L.nf_synchronize(sub[0].h)
        t = time.perf_counter()
        k = [s.solve_keff()[0] for s in sub]
        sub[0].L.nf_synchronize(sub[0].h)
        return time.perf_counter() - t, k

    for l in lines:
        say(l)
    run_batch(hs[:2]); run_loop(hs[:2])                          # first launches of both kernels
    for n in (1, 8, 64, cus, 2 * cus):
        sub = hs[:n]
        tb, tl = [], []
        for r in range(3):
            if r % 2 == 0:
                b = run_batch(sub); l = run_loop(sub)
            else:
                l = run_loop(sub); b = run_batch(sub)
            assert list(b[1]) == list(l[1]), "batch and loop disagree"
            tb.append(b[0]); tl.append(l[0])
        mb, ml = statistics.median(tb), statistics.median(tl)
        route = "batched" if b[2]["n_batched"] == n else "sequential"
        say(f"{n:>5} {route:>10} {1e3 * mb:>10.2f} {1e3 * ml:>10.2f} {n / mb:>14.1f} {n / ml:>13.1f} {ml / mb:>10.2f}")
    for s in hs:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), action="append")
    ap.add_argument("--worker", choices=sorted(CASES))
    ap.add_argument("--limit-s", type=int, default=900, help="time limit of one case (KOEBERG-2D RT1-P1: 180 ms per single solve, about 7 minutes of loops)")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker); return 0
    out, rc = [], 0
    for case in a.case or list(CASES):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit_s), sys.executable, os.path.abspath(__file__), "--worker", case], capture_output=True, text=True)
        sys.stdout.write(r.stdout); sys.stderr.write(r.stderr)
        out.append(r.stdout)
        rc = r.returncode
        if rc != 0:
            out.append(f"{case}: exit status {rc} (124: the time limit of {a.limit_s} s); the rows above are what was measured; stopped here\n")
            print(out[-1], file=sys.stderr)
            break
    with open(OUT, "a" if a.case else "w") as f:
        f.write("# python profiles/tools/batch_throughput.py -- median of three alternating rounds, wall time with the final synchronise\n" + "".join(out))
    return rc


if __name__ == "__main__":
    sys.exit(main())
