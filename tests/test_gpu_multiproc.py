"""The REAL multi-process path on one GPU: several ranks (one process each, all on device 0) run the slab-decomposed
Schur apply and power iteration through nf_comm_init / ncclSend / ncclRecv / ncclAllReduce, with tests/fake_rccl (a
host-staged stand-in selected by NEUTFEM_RCCL_LIB) as the transport -- RCCL itself refuses two ranks on one device.  What
this covers that the loopback tests cannot: rank/peer arithmetic, the order of collective calls across processes, the
comm-stream overlap, the coarse team borrowing the communicator, and bench.py's --gpus N code path end to end."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from helpers import CG_FORMS, make_hip, make_oracle, rel_l2, synthetic_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _env():
    if not os.path.exists(FAKE):
        pytest.fail("tests/fake_rccl/libfake_rccl.so is missing: run __graft_entry__.build()")
    e = dict(os.environ); e["NEUTFEM_RCCL_LIB"] = FAKE; e["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return e


def _run_ranks(world, args, tmp_path, timeout=200, env=None, wait_all=False):
    """start `world` workers, fail fast (with every rank's output) if one exits non-zero or the run exceeds `timeout` s.
    wait_all: let every rank end by itself (no kill on the first failure) -- the point of the test is that they all do"""
    import time
    port = str(_free_port())
    logs = [open(str(tmp_path / f"rank{r}.log"), "w+") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multiproc_worker.py"), str(r), str(world), port] + [str(a) for a in args],
                              env=env or _env(), stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    t0 = time.time(); bad = None
    while any(p.poll() is None for p in procs):
        if not wait_all and any(p.poll() not in (None, 0) for p in procs): bad = "a rank failed"; break
        if time.time() - t0 > timeout: bad = f"timed out after {timeout} s"; break
        time.sleep(0.2)
    if bad is None and any(p.returncode != 0 for p in procs): bad = "a rank failed"
    for p in procs:
        if p.poll() is None: p.kill()
    out = []
    for r, f in enumerate(logs):
        f.seek(0); out.append(f"--- rank {r} (rc={procs[r].returncode}) ---\n" + f.read()[-3000:]); f.close()
    if bad is not None:                                             # pytest truncates long assertion messages: keep the ranks' output where gpurun collects it
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "multiproc_last_failure.log"), "w") as f:
                f.write(f"{bad}\nargs: {args}\n" + "\n".join(out))
        except OSError:
            pass
    return bad, "\n".join(out)


@pytest.mark.parametrize("world,per,use_diag,planes", [(2, 1, 0, 48), (3, 1, 0, 48), (2, 2, 0, 48), (3, 1, 1, 48), (4, 1, 0, 12), (3, 1, 2, 16)])
def test_ranks_on_one_gpu_match_the_undivided_solve(world, per, use_diag, planes, tmp_path):
    """planes = 48: coarse slabs of 24 planes need one separator sweep; planes = 12: the fine slabs themselves are thin"""
    out = str(tmp_path / "res.npz")
    NO = (4 if world == 4 else 8) if use_diag == 0 else 16         # fixed work: outers of the fine solve (the full path spends half as many on the coarse twin first; four ranks of thin slabs: 8 sweeps per apply)
    bad, logs = _run_ranks(world, [out, per, use_diag, planes, 0, 0, NO], tmp_path)
    assert bad is None, bad + "\n" + logs
    res = np.load(out)
    nz = planes * world * per
    inp = synthetic_inputs(10, 8, nz, 2, seed=9, dirichlet=(1, 2, 4, 5, 6))
    o = make_oracle(inp)
    assert rel_l2(res["y"].ravel(), o.schur_apply(1, res["x"].ravel())) < 1e-12
    assert np.ptp(res["k"]) == 0.0 and np.ptp(res["n"]) == 0          # every rank returns the same k and outer count
    # full Schur path: single-reduction CG -- ONE all-reduce per CG iteration (4 kernels + k_finalize per rank), also with several slabs per rank
    if use_diag == 0:
        assert (res["red"] == 1).all() and (res["vec"] == 0).all(), (res["red"], res["vec"])
    s = make_hip(inp); s.set_tol(1e-12, 1e-9, 1e-9, NO, 2000)       # the same fixed work, undivided
    ks, ns = (s.solve_keff(use_diag=True, use_cmfd=use_diag == 2)) if use_diag else s.solve_keff(True, [2, 1, 2])
    assert int(res["n"][0]) == ns == NO
    assert abs(res["k"][0] - ks) / ks < 1e-8
    assert rel_l2(res["phi"].ravel(), s.get_phi().ravel()) < 1e-6
    if not use_diag:                                              # currents: z faces through the partition method across ranks
        assert rel_l2(res["J"].ravel(), s.get_J().ravel()) < 1e-6
    s.close()


def test_reduction_routes_agree(tmp_path):
    """the same 3-rank solve through the three reduction routes of the CG on slab teams: single-reduction CG (default: one all-reduce of
    five doubles per iteration, interface planes on a communicator of their own here), and the reference recurrence with its two
    reductions per iteration as vectors of block partials or as scalars behind k_finalize: same outer count, k and flux to rounding"""
    outs = []
    for cg1, vec, xc in (("1", "1", "1"), ("0", "1", "0"), ("0", "0", "0")):
        e = _env(); e["NEUTFEM_TEST_CG1"] = cg1; e["NEUTFEM_TEST_VEC_REDUCE"] = vec; e["NEUTFEM_TEST_XCHG_COMM"] = xc
        out = str(tmp_path / f"res{cg1}{vec}.npz")
        bad, logs = _run_ranks(3, [out, 1, 0, 16, 0, 0, 4], tmp_path, env=e)   # 4 fine outers (2 coarse), thin slabs: one separator sweep per apply
        assert bad is None, bad + "\n" + logs
        outs.append(np.load(out))
    a, b, c = outs
    assert (a["red"] == 1).all() and (a["vec"] == 0).all() and (a["xc"] == 1).all()
    assert (b["red"] == 2).all() and (b["vec"] == 1).all() and (b["xc"] == 0).all() and (c["red"] == 2).all() and (c["vec"] == 0).all()
    for x, form in ((a, "team_sr"), (b, "team_vec"), (c, "team_lean")):   # every rank ran the same form of the CG iteration, the one asked for
        assert [CG_FORMS[f] for f in x["form"]] == [form] * 3, (form, x["form"])
    for x in (a, b):
        assert int(x["n"][0]) == int(c["n"][0]) and abs(x["k"][0] - c["k"][0]) / c["k"][0] < 1e-11
        assert rel_l2(x["phi"].ravel(), c["phi"].ravel()) < 1e-9


def test_two_ranks_rt1p1(tmp_path):
    """RT1-P1 across two real processes: four transverse modes per interface travel as one message"""
    out = str(tmp_path / "res.npz")
    bad, logs = _run_ranks(2, [out, 1, 0, 14, 0, 1], tmp_path)
    assert bad is None, bad + "\n" + logs
    res = np.load(out)
    inp = synthetic_inputs(10, 8, 28, 2, seed=9, dirichlet=(1, 2, 4, 5, 6))
    s = make_hip(inp, 1, 1); s.set_tol(1e-12, 1e-9, 1e-9, 16, 2000)
    ks, ns = s.solve_keff(True, [2, 1, 2])
    assert int(res["n"][0]) == ns == 16 and abs(res["k"][0] - ks) / ks < 1e-8
    assert rel_l2(res["phi"].ravel(), s.get_phi().ravel()) < 1e-6
    s.close()


def test_thin_slab_is_refused_by_every_rank(tmp_path):
    """a middle slab of 3 planes: the refusal is taken on the all-reduced maximum, so all three ranks raise the same error at
    the same point instead of one raising and two blocking in the next collective"""
    bad, logs = _run_ranks(3, [str(tmp_path / "none.npz"), 1, 0, 3], tmp_path, timeout=120)
    assert bad == "a rank failed", (bad, logs)
    assert logs.count("too thin") >= 3, logs


def test_indivisible_coarse_factors_are_refused_by_every_rank(tmp_path):
    """100 planes on 3 ranks = 33 / 34 / 33 with coarse factor 2 in z: only the outer ranks cannot coarsen, but the verdict
    is all-reduced, so all three raise instead of the middle one blocking in the coarse solve's first collective"""
    bad, logs = _run_ranks(3, [str(tmp_path / "none.npz"), 1, 0, 0, 100], tmp_path, timeout=120)
    assert bad == "a rank failed", (bad, logs)
    assert logs.count("do not divide") >= 3, logs


@pytest.mark.parametrize("route,inject,extra,env_extra", [
    ("single-reduction CG (RT0-P0 teams' default: one 5-double all-reduce per iteration)", "1:40", [], {}),
    ("vector reduce (two reductions per iteration, one slab per rank)", "1:40", [], {"NEUTFEM_TEST_CG1": "0"}),
    ("scalar reduce (k_finalize + 2-double all-reduce)", "1:40", [], {"NEUTFEM_TEST_CG1": "0", "NEUTFEM_TEST_VEC_REDUCE": "0"}),
    ("RT1-P1 team (k_finalize + k_cg_logic, no lean CG)", "1:25:4", [0, 1], {})])
def test_failing_rank_stops_every_rank_instead_of_hanging_them(tmp_path, route, inject, extra, env_extra):
    """a rank-local error inside a solve used to return on that rank only -- the others then waited in
    ncclAllReduce until somebody killed the job.  NEUTFEM_INJECT_FAIL=1:40 makes rank 1 of 3 fail (as a refused launch would) at its
    41st CG iteration.  Expected: rank 1 raises its error flag in the all-reduces that exist anyway, keeps the collective schedule
    going, and ALL THREE ranks leave the solve at the same iteration -- rank 1 with its own error, ranks 0 and 2 with NF_ERR_REMOTE --
    within seconds, by themselves."""
    import time
    e = _env(); e["NEUTFEM_INJECT_FAIL"] = inject; e["NEUTFEM_COMM_TIMEOUT_S"] = "60"; e.update(env_extra)
    t0 = time.time()
    bad, logs = _run_ranks(3, [str(tmp_path / "none.npz"), 1, 0, 16] + extra, tmp_path, timeout=150, env=e, wait_all=True)
    assert bad == "a rank failed", (bad, logs)                     # i.e. not "timed out": every rank ended by itself
    assert time.time() - t0 < 120, logs
    per = logs.split("--- rank ")[1:]
    assert len(per) == 3 and all("(rc=0)" not in p.splitlines()[0] for p in per), logs      # nobody pretends to have succeeded
    assert "injected failure on rank 1" in per[1], logs
    assert "another rank of the team reported an error" in per[0] and "another rank of the team reported an error" in per[2], logs
    its = [int(p.split("every rank stopped at iteration ")[1].split()[0].rstrip(".,;)")) for p in (per[0], per[2])]
    assert its[0] == its[1], logs                                 # the same iteration on both healthy ranks


@pytest.mark.parametrize("where,inject,use_diag,expect", [
    ("start of outer 3 of the fine solve's coarse twin (the next CG solve ends everybody at its first reduction)", "1:o3", 0, "every rank stopped at iteration 0"),
    ("end of outer 2, after the group solves (the per-outer reduction carries the flags to the hosts)", "1:e2", 0, "during outer iteration 2; every rank stopped there"),
    ("diagonal path, start of outer 5 (no CG: the per-outer reduction is the only collective)", "1:o5", 1, "during outer iteration 5; every rank stopped there"),
    ("before the partition-method solve of nf_get_J (an exchange-only collective: verdicts are all-reduced first)", "1:a", 0, "no rank started it")])
def test_failure_outside_the_cg_loop_stops_every_rank(tmp_path, where, inject, use_diag, expect):
    """a rank that fails BETWEEN two collectives of the outer iteration (an allocation, a refused launch) or on its way
    into an exchange-only collective used to return alone; its peers then sat in the next collective until NEUTFEM_COMM_TIMEOUT_S.  Now
    the rank's flag rides in the reductions that exist anyway (first reduction of the next CG solve, per-outer reduction) and exchange-only
    collectives all-reduce a verdict before the first plane is posted: all three ranks end within seconds, rank 1 with its own error,
    ranks 0 and 2 with NF_ERR_REMOTE at the same point."""
    import time
    e = _env(); e["NEUTFEM_INJECT_FAIL"] = inject; e["NEUTFEM_COMM_TIMEOUT_S"] = "60"
    t0 = time.time()
    bad, logs = _run_ranks(3, [str(tmp_path / "none.npz"), 1, use_diag, 16, 0, 0, 8], tmp_path, timeout=100, env=e, wait_all=True)   # 8 fine outers (4 coarse)
    assert bad == "a rank failed", (bad, logs)                     # not "timed out": every rank ended by itself
    assert time.time() - t0 < 60, logs                             # and long before the collective timeout
    per = logs.split("--- rank ")[1:]
    assert len(per) == 3 and all("(rc=0)" not in p.splitlines()[0] for p in per), logs
    assert "injected failure on rank 1" in per[1], logs
    for p in (per[0], per[2]):
        assert "another rank of the team reported an error" in p and expect in p, logs


def test_a_lost_peer_times_out_and_the_solver_can_be_closed(tmp_path):
    """after NF_ERR_COMM the streams hold collectives whose peer is gone; nf_destroy used to synchronise them (and the coarse
    twin kept the aborted communicator), so closing the solver could block for ever.  Rank 1 of 2 exits before the solve: rank 0's
    first collective times out (NEUTFEM_COMM_TIMEOUT_S = 5), the team is marked dead, a second solve is refused at once and close()
    returns without waiting for the device."""
    import time
    e = _env(); e["NEUTFEM_WORKER_LOSE_RANK"] = "1"; e["NEUTFEM_COMM_TIMEOUT_S"] = "5"
    t0 = time.time()
    bad, logs = _run_ranks(2, [str(tmp_path / "none.npz"), 1, 0, 16], tmp_path, timeout=90, env=e, wait_all=True)
    assert bad == "a rank failed" and time.time() - t0 < 60, (bad, logs)
    r0 = logs.split("--- rank ")[1]
    assert "(rc=5)" in r0.splitlines()[0], logs
    assert "did not complete within 5 s" in r0 and "second solve refused" in r0 and "is unusable" in r0, logs
    assert float(r0.split("closed in ")[1].split()[0]) < 2.0, logs


@pytest.mark.parametrize("cg1", ["1", "0"])
def test_every_rank_issues_the_same_sequence_of_collectives(tmp_path, cg1):
    """What the stand-in transport cannot show and RCCL punishes with a hang: ranks that issue their collectives in different orders.  With
    NEUTFEM_TRACE_COMM=1 every rank prints one line per collective it enqueues (plane exchanges, all-reduces, verdicts); the three ranks of a solve
    -- coarse twin, thin slabs with separator sweeps, currents at the end -- must print the SAME sequence of (kind, element count), whatever their
    position in the stack (the bottom and top ranks have one neighbour, the middle one two: same calls, other peers).  Both CG routes."""
    e = _env(); e["NEUTFEM_TRACE_COMM"] = "1"; e["NEUTFEM_TEST_CG1"] = cg1; e["FAKE_RCCL_REPORT"] = "1"
    e["NEUTFEM_TEST_VEC_REDUCE"] = "0"                              # the reference recurrence through k_finalize + scalar all-reduces (the vector all-reduce is not traced)
    out = str(tmp_path / "res.npz")
    bad, logs = _run_ranks(3, [out, 1, 0, 16, 0, 0, 4], tmp_path, env=e)
    assert bad is None, bad + "\n" + logs[-3000:]
    seqs = []
    for r in range(3):
        with open(str(tmp_path / f"rank{r}.log")) as f:
            seq = []
            for ln in f:
                if not ln.startswith("[comm] rank"):
                    continue
                body = ln.split(None, 3)[3] if len(ln.split(None, 3)) > 3 else ""      # after "[comm] rank <r>"
                body = body.lstrip(": ")
                if body.startswith("exchange"):
                    seq.append(("exchange", body.split("which=")[1].split()[0], body.split("count=")[1].split()[0]))
                elif body.startswith("allreduce"):
                    kind = body.split()[1]
                    cnt = body.split("count=")[1].split()[0] if "count=" in body else "1"
                    seq.append(("allreduce", kind, cnt))
                else:
                    seq.append(("other", body.split()[0], ""))
            seqs.append(seq)
    # the stand-in serializes the calls on one communicator like RCCL does (an all-reduce on the solver's stream waits for the exchange issued before it on
    # the comm stream, and the other way round): the run above went through that chain -- thousands of cross-stream waits per rank -- without hanging
    import re
    logs_all = "".join(open(str(tmp_path / f"rank{r}.log")).read() for r in range(3))
    waits = [int(m.group(1)) for m in re.finditer(r"fake_rccl: rank \d of 3: \d+ calls, (\d+) cross-stream waits", logs_all)]
    assert len(waits) >= 3 and min(waits) > 500, (waits, logs_all[-500:])
    assert len(seqs[0]) > 200, len(seqs[0])                        # exchanges and reductions of two group solves per outer, coarse and fine
    assert seqs[0] == seqs[1] == seqs[2], next((i, a, b, c) for i, (a, b, c) in enumerate(zip(*seqs)) if not (a == b == c)) if len(set(map(len, seqs))) == 1 else list(map(len, seqs))
    n_ar = sum(1 for t in seqs[0] if t[0] == "allreduce" and t[1] in ("single-reduction", "reduce")); n_x = sum(1 for t in seqs[0] if t[0] == "exchange" and t[1] == "0")
    # one all-reduce per apply on the single-reduction route (plus the verdicts and per-outer reductions), two on the reference recurrence
    assert (n_ar <= 1.2 * n_x) if cg1 == "1" else (n_ar >= 1.5 * n_x), (n_ar, n_x)   # measured 4658 vs 2831 on the reference recurrence (exchanges also serve applies outside the CG)


def test_bench_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` as a user (or the driver at N = 1's form) types it: bench.py itself starts the two ranks the way the
    driver does for N = 2 (python -m torch.distributed.run, gloo rendezvous, RCCL id broadcast, slab split, barrier + max-over-ranks
    timing, one JSON line from rank 0) -- both ranks forced onto device 0 -- and the line says how many ranks the live communicator
    counts and which library carried the data (--gpus used to be ignored)"""
    e = _env(); e["NEUTFEM_FORCE_DEVICE"] = "0"; e["NEUTFEM_BENCH_N"] = "64"
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"): e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"],
                       env=e, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "starting 2 ranks" in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                       # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["transport"].endswith("libfake_rccl.so"), (d["n_gpus"], d["rccl_ranks"], d["transport"])
    assert d["steps"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    # same workload on one rank: the power iteration is the same algorithm, k after the timed steps must agree
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--cpu-sample-iters", "0",
                         "--no-converge", "--no-parity", "--no-small"], env=e, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert r1.returncode == 0, r1.stderr[-2000:]
    d1 = json.loads([ln for ln in r1.stdout.splitlines() if ln.startswith("{")][0])
    assert d1["n_gpus"] == 1 and d1["rccl_ranks"] == 1
    # IAEA-3D at the drivers' CG tolerance (1e-4, cond(S) ~ 1e17): the ranks' single-reduction CG and the undivided mesh's reference recurrence end
    # their solves at different iterates within that tolerance, so k after two unconverged outers agrees to ~4e-6 (measured; two builds of the
    # ORACLE differ by 1e-6 ... 7e-6 on such runs, tests/golden/rounding_spread.json); the bar is north_star's 1 pcm.  Tight-tolerance agreement of
    # the same path: test_ranks_on_one_gpu_match_the_undivided_solve (k 1e-8 after 8 fixed outers), test_iaea3d_256cube_golden[c3_layout...] (2e-9).
    assert abs(d["keff_after_timed_steps"] - d1["keff_after_timed_steps"]) / d1["keff_after_timed_steps"] < 1e-5


def test_bench_json_contract_single_rank():
    """the one-line JSON of `python bench.py --full` (driver contract + the tier's roofline / cpu_baseline objects), on a small mesh"""
    e = dict(os.environ); e["NEUTFEM_BENCH_N"] = "48"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--cpu-sample-iters", "3", "--full"],
                       env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1                                       # ONE line on stdout; progress notes go to stderr
    d = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", float),
                     ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[key], typ), key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f64"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert "traffic" in rf and rf["measured_copy"]["GBps"] > 1000
    cb = d["cpu_baseline"]
    assert cb["cores"] == 1 and cb["kind"] == "port" and cb["value"] > 0 and isinstance(cb["sample"], str)
    assert d["parity"]["pcm"] < 1.0 and d["parity"]["flux_rel_l2"] < 1e-8
    assert len(d["other_configs"]) == 4 and all(c["pcm_vs_oracle"] < 1.0 for c in d["other_configs"])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """a plain `python bench.py` (no --full) prints the headline and nothing it has to measure apart; --steps sets the timed outers;
    --dump-outputs writes k and the flux of the last timed step, the same on two runs with the same arguments"""
    e = dict(os.environ); e["NEUTFEM_BENCH_N"] = "48"
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / run)],
                           env=e, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    assert not set(d) & {"roofline", "converged", "other_configs", "higher_order", "cpu_baseline", "parity", "parity_at_bench_size", "c5_single_gpu"}
    k = [np.load(str(tmp_path / run / "keff.npy")) for run in ("a", "b")]
    phi = [np.load(str(tmp_path / run / "phi.npy")) for run in ("a", "b")]
    assert k[0].dtype == np.float64 and k[0].shape == (1,) and k[0][0] == d["keff_after_timed_steps"]
    assert phi[0].dtype == np.float64 and phi[0].shape == (2, 48 ** 3) and np.all(np.isfinite(phi[0])) and phi[0].max() > 0
    assert abs(k[1][0] - k[0][0]) < 1e-12 * k[0][0] and rel_l2(phi[1].ravel(), phi[0].ravel()) < 1e-12


def test_two_ranks_over_the_real_rccl(tmp_path):
    """The same worker over the REAL librccl, one GPU per rank: needs a box with at least two GPUs (the one-GPU test boxes skip it;
    RCCL refuses two ranks on one device).  Exercises what the stand-in transport cannot: grouped ncclSend / ncclRecv on the comm stream
    next to ncclAllReduce on the solver's stream of ONE communicator, and the order of the collective calls across processes."""
    from neutfem_amd import capi
    if capi.device_count() < 2:
        pytest.skip("needs two GPUs: real RCCL has one rank per device")
    e = dict(os.environ); e.pop("NEUTFEM_RCCL_LIB", None); e["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"; e["NEUTFEM_WORKER_RANK_IS_DEVICE"] = "1"
    out = str(tmp_path / "res.npz")
    bad, logs = _run_ranks(2, [out, 1, 0, 48], tmp_path, timeout=300, env=e)
    assert bad is None, bad + "\n" + logs
    res = np.load(out)
    inp = synthetic_inputs(10, 8, 96, 2, seed=9, dirichlet=(1, 2, 4, 5, 6))
    o = make_oracle(inp)
    assert rel_l2(res["y"].ravel(), o.schur_apply(1, res["x"].ravel())) < 1e-12
    s = make_hip(inp); s.set_tol(1e-12, 1e-9, 1e-9, 16, 2000)
    ks, ns = s.solve_keff(True, [2, 1, 2])
    assert int(res["n"][0]) == ns == 16 and abs(res["k"][0] - ks) / ks < 1e-8
    assert rel_l2(res["phi"].ravel(), s.get_phi().ravel()) < 1e-6
    s.close()
