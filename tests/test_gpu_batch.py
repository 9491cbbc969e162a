"""nf_solve_keff_batch: n small meshes in one launch, one workgroup each.  The bar is bit equality with nf_solve_keff on
twin handles, one after another -- the same inlined kernel body, fixed-order sums, nothing shared between workgroups -- per kernel
instantiation, with per-handle options, with more workgroups than compute units, from a warm state; the oracle independently; the
sequential route; the refusals; the Python surfaces."""
import ctypes as C

import numpy as np
import pytest

from helpers import load_inputs, make_hip, make_oracle, rel_l2, synthetic_inputs

pytestmark = pytest.mark.gpu

TOL = (1e-9, 1e-9, 1e-10, 200, 2000)
RES = dict(resident=1, resident_max_dofs=100000)
UNTOUCHED = -(2 ** 31)
INFO = ("last_path", "last_resident_serial", "last_outer", "last_cg_total")


def _solvers(shape, rt, ng, n, opts=RES, seed0=100, tol=TOL):
    out = []
    for i in range(n):
        s = make_hip(synthetic_inputs(*shape, ng=ng, seed=seed0 + i), rt, rt); s.set_tol(*tol)
        for k, v in opts.items():
            s.set_option(k, v)
        out.append(s)
    return out


def _warm(s):
    v, k = C.c_int(), C.c_double()
    assert s.L.nf_get_warm_state(s.h, C.byref(v), C.byref(k)) == 0
    return v.value, k.value


def _state(s, with_J=True):
    """everything nf_solve_keff leaves on a handle that the C ABI shows"""
    h = s.history()
    d = dict(hk=h["k"].copy(), hdk=h["dk"].copy(), hdphi=h["dphi"].copy(), hcg=h["cg"].copy(), phi=s.get_phi().copy(), warm=_warm(s),
             progress=s.progress(), info=tuple(s.info(k) for k in INFO))
    if with_J:
        d["J"] = s.get_J().copy()
    return d


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def _one_by_one(twins, **kw):
    ks, ns = [], []
    for t in twins:
        k, n = t.solve_keff(**kw); ks.append(k); ns.append(n)
    return ks, ns


def _check_batch_equals_twins(batch, twins, res_expect=None, **kw):
    from neutfem_amd import capi
    k, no, st, res = capi.solve_keff_batch(batch, **kw)
    tk, tn = _one_by_one(twins, **kw)
    assert list(st) == [0] * len(batch), st
    for i, (b, t) in enumerate(zip(batch, twins)):
        assert k[i] == tk[i] and no[i] == tn[i], (i, k[i], tk[i], no[i], tn[i])
        _same(_state(b), _state(t), i)
    if res_expect:
        for key, v in res_expect.items():
            assert res[key] == v, (key, res)
    return k, no, res


def _close(*lists):
    for l in lists:
        for s in l:
            s.close()


# shape, order, groups, options on top of RES, last_resident_serial, nf_batch_result::variant
INSTANCES = [
    ("pitch1536", (12, 11, 10), 0, 2, {}, 1, 1),
    ("pitch2560", (47, 45, 1), 0, 2, {}, 1, 2),
    ("lines-of-4", (4, 8, 8), 0, 2, {}, 1, 1),
    ("1d", (250, 1, 1), 0, 2, {}, 1, 1),
    ("rt1-lanes", (6, 3, 2), 1, 2, {}, 1, 3),
    ("rt2-lanes", (21, 5, 1), 2, 1, {}, 1, 4),
    ("scan-vec", (12, 11, 10), 0, 2, dict(resident_serial=0), 0, 6),
    ("scan-novec", (9, 8, 3), 0, 2, dict(resident_serial=0), 0, 5),
    ("scan-rt1", (6, 5, 4), 1, 2, dict(resident_serial=0), 0, 8),
    ("scan-rt2", (10, 9, 1), 2, 1, dict(resident_serial=0), 0, 10),
    ("scan-rt1-novec", (5, 5, 4), 1, 2, dict(resident_serial=0), 0, 7),
    ("scan-rt2-novec", (9, 9, 1), 2, 1, dict(resident_serial=0), 0, 9),
]


@pytest.mark.parametrize("name,shape,rt,ng,extra,serial,variant", INSTANCES, ids=[c[0] for c in INSTANCES])
def test_batch_is_bitwise_the_sequential_solves(name, shape, rt, ng, extra, serial, variant):
    opts = dict(RES, **extra)
    batch, twins = _solvers(shape, rt, ng, 5, opts), _solvers(shape, rt, ng, 5, opts)
    k, no, res = _check_batch_equals_twins(batch, twins, dict(n_batched=5, n_sequential=0, n_launches=1, variant=variant))
    for b in batch:
        assert b.info("last_path") == 2 and b.info("last_resident_serial") == serial
    assert batch[0].info("batch_launches") == 1 and batch[1].info("batch_launches") == 0 and twins[0].info("batch_launches") == 0
    assert len(set(no)) > 1 or len({b.info("last_cg_total") for b in batch}) > 1      # the workgroups did different amounts of work
    _close(batch, twins)


def test_per_handle_options():
    """n_opts = n: tolerances and max_outer differ per handle; tol_keff = 0 with max_outer = 6 gives exactly 6 outers next to neighbours
    that stop earlier and later"""
    from neutfem_amd import capi
    tols = [(1e-5, 1e-4, 1e-4, 200, 1000), (0.0, 1e-9, 1e-10, 6, 2000), TOL, (1e-7, 1e-7, 1e-8, 3, 500)]
    batch, twins = _solvers((12, 11, 10), 0, 2, 4), _solvers((12, 11, 10), 0, 2, 4)
    for l in (batch, twins):
        for s, t in zip(l, tols):
            s.set_tol(*t)
    k, no, res = _check_batch_equals_twins(batch, twins, dict(n_batched=4, n_launches=1))
    assert no[1] == 6 and no[3] == 3 and no[0] != 6 and no[2] > 6 and no[0] < no[2], no
    # the raw call with one option set for all: every handle runs under handle 1's options
    L = batch[0].L
    for s in batch + twins:
        s.reset_flux(); s.set_tol(*tols[1])
    hs = (C.c_void_p * 4)(*[s.h for s in batch]); o = batch[1].opts()
    kk, nn, st = np.zeros(4), np.zeros(4, dtype=np.int32), np.full(4, UNTOUCHED, dtype=np.int32)
    rb = capi.BatchResult()
    assert L.nf_solve_keff_batch(hs, 4, C.byref(o), 1, kk.ctypes.data_as(C.POINTER(C.c_double)), nn.ctypes.data_as(C.POINTER(C.c_int)),
                                 st.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rb)) == 0
    tk, tn = _one_by_one(twins)
    assert list(nn) == [6] * 4 == tn and list(kk) == tk and list(st) == [0] * 4 and rb.n_batched == 4
    for b, t in zip(batch, twins):
        _same(_state(b), _state(t))
    # keff, n_outer, status and res may each be NULL
    for s in batch + twins:
        s.reset_flux()
    assert L.nf_solve_keff_batch(hs, 4, C.byref(o), 1, None, None, None, None) == 0
    _one_by_one(twins)
    for b, t in zip(batch, twins):
        _same(_state(b), _state(t))
    _close(batch, twins)


def test_more_workgroups_than_compute_units():
    """compute units + 4 workgroups: the grid runs in turns.  The count is the device's multiProcessorCount, which is also what
    torch.cuda.get_device_properties(0).multi_processor_count reports; it is read through the library (nf_info "compute_units") because
    torch cannot initialise its own HIP runtime in a process in which the library has already opened the device"""
    from neutfem_amd import capi
    probe = _solvers((4, 8, 8), 0, 2, 1)
    n = probe[0].info("compute_units") + 4
    _close(probe)
    assert n >= 12
    batch, twins = _solvers((4, 8, 8), 0, 2, n), _solvers((4, 8, 8), 0, 2, n)
    _check_batch_equals_twins(batch, twins, dict(n_batched=n, n_sequential=0, n_launches=1, variant=1))
    assert batch[0].info("batch_capacity") == n and batch[0].info("batch_launches") == 1
    _check_batch_equals_twins(batch, twins, dict(n_batched=n, n_launches=1))          # from the warm state; the array of structs is reused
    assert batch[0].info("batch_capacity") == n and batch[0].info("batch_launches") == 2
    k, no, st, res = capi.solve_keff_batch(batch[:7])                                 # a smaller batch grows nothing either
    assert batch[0].info("batch_capacity") == n and res["n_batched"] == 7
    _close(batch, twins)


def test_warm_start_and_state():
    from neutfem_amd import capi
    batch, twins = _solvers((9, 8, 3), 0, 2, 4), _solvers((9, 8, 3), 0, 2, 4)
    outside, outside_twin = _solvers((9, 8, 3), 0, 2, 2, seed0=300), _solvers((9, 8, 3), 0, 2, 2, seed0=300)
    outside[1].solve_keff(); outside_twin[1].solve_keff()                            # one bystander solved, one fresh
    before = [_state(s, with_J=False) for s in outside]
    _check_batch_equals_twins(batch, twins, dict(n_batched=4))
    k2, no2, _ = _check_batch_equals_twins(batch, twins, dict(n_batched=4))          # second batch from the warm state
    assert all(_warm(b)[0] == 1 for b in batch) and all(n >= 1 for n in no2)
    # one handle solved alone between two batches behaves as between two nf_solve_keff calls
    assert batch[2].solve_keff() == twins[2].solve_keff()
    _same(_state(batch[2]), _state(twins[2]))
    _check_batch_equals_twins(batch, twins, dict(n_batched=4))
    # reset_flux: back to the cold start, on some handles only
    for l in (batch, twins):
        l[0].reset_flux(); l[3].reset_flux()
    assert _warm(batch[0])[0] == 0 and _warm(batch[1])[0] == 1
    k4, no4, _ = _check_batch_equals_twins(batch, twins, dict(n_batched=4))
    assert no4[0] > no4[1]                                                             # cold next to warm
    # handles that were not in the batches: flux, warm state, history as they were
    for s, b, t in zip(outside, before, outside_twin):
        _same(_state(s, with_J=False), b); _same(_state(s, with_J=False), _state(t, with_J=False))
    _close(batch, twins, outside, outside_twin)


def _perturbed(inp, seed, amp=0.01):
    """cross sections scaled by a seeded +-amp per assembly (blocks of 2 x 2 cells where the mesh allows)"""
    rng = np.random.default_rng(seed)
    ny, nx = inp["D"].shape[-2:]
    b = 2 if ny % 2 == 0 and nx % 2 == 0 else 1
    out = dict(inp)
    for key in ("D", "SigR", "NSF", "SigS"):
        f = np.kron(1.0 + amp * rng.uniform(-1.0, 1.0, (ny // b, nx // b)), np.ones((b, b)))
        out[key] = inp[key] * f
    return out


def test_batch_against_the_oracle():
    """independent of the sequential route: IAEA-2D RT0-P0, three perturbed cross-section sets in one batch, against the CPU oracle's own
    solves at the bars tests/test_gpu_paths.py holds this path to"""
    from neutfem_amd import capi
    base = load_inputs("iaea2d")
    inps = [_perturbed(base, 11 + i) for i in range(3)]
    batch = [make_hip(inp) for inp in inps]
    for s in batch:
        s.set_tol(*TOL)
    k, no, st, res = capi.solve_keff_batch(batch)
    assert list(st) == [0, 0, 0] and res["n_batched"] == 3 and res["n_launches"] == 1
    assert len(set(k)) == 3
    for i, inp in enumerate(inps):
        o = make_oracle(inp); o.set_tol(*TOL); ko = o.SolveKeff()
        assert abs(k[i] - ko) / ko < 1e-9, (i, k[i], ko)
        assert no[i] == o.info("last_outer"), (i, no[i], o.info("last_outer"))
        assert rel_l2(batch[i].get_phi().ravel(), o.phi_dofs().ravel()) < 1e-8, i
    _close(batch)


def _void_handle(seed):
    from neutfem_amd.capi import HipSolver
    inp = synthetic_inputs(9, 8, 3, ng=2, seed=seed)
    s = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"]); s.set_linear_solver(6)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        s.set_bc(int(a), int(t))
    mask = np.zeros((3, 8, 9), dtype=bool); mask[1, 2:4, 3:5] = True
    s.set_void(mask, 0.5)
    s.upload_xs(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); s.build(); s.set_tol(*TOL)
    for k, v in RES.items():
        s.set_option(k, v)
    return s


SEQUENTIAL = ["resident-off", "void-mask", "other-shape", "above-resident-max-dofs", "coarse-init", "diagonal-solver"]


@pytest.mark.parametrize("case", SEQUENTIAL)
def test_sequential_route(case):
    """a batch that the one launch cannot take still solves, handle by handle, with the results of nf_solve_keff"""
    kw = {}
    def three():
        l = _solvers((9, 8, 3), 0, 2, 3)
        if case == "resident-off":
            l[1].set_option("resident", 0)
        elif case == "void-mask":
            l[1].close(); l[1] = _void_handle(101)
        elif case == "other-shape":
            l[2].close(); l[2] = _solvers((9, 8, 4), 0, 2, 1, seed0=102)[0]
        elif case == "above-resident-max-dofs":
            l[0].set_option("resident_max_dofs", 100)
        return l
    if case == "coarse-init":
        base = load_inputs("iaea2d"); kw = dict(use_coarse=True, factors=[int(v) for v in base["coarse_factors"]])
        def three():
            l = [make_hip(_perturbed(base, 21 + i)) for i in range(2)]
            for s in l:
                s.set_tol(*TOL)
            return l
    elif case == "diagonal-solver":
        kw = dict(use_diag=True)
    batch, twins = three(), three()
    n = len(batch)
    _check_batch_equals_twins(batch, twins, dict(n_batched=0, n_sequential=n, n_launches=0, variant=0), **kw)
    assert batch[0].info("batch_launches") == 0
    paths = [b.info("last_path") for b in batch]
    if case in ("resident-off", "void-mask", "above-resident-max-dofs"):
        assert paths.count(2) == 2, paths                          # only the odd one leaves the resident kernel
    elif case == "diagonal-solver":
        assert paths == [1, 1, 1]
    _close(batch, twins)


def _raw(L, handles, n, opts, n_opts):
    from neutfem_amd import capi
    m = max(len(handles), 1)
    hs = (C.c_void_p * m)(*handles)
    st = np.full(m, UNTOUCHED, dtype=np.int32)
    os_ = (capi.KeffOpts * max(len(opts), 1))(*opts)
    rc = L.nf_solve_keff_batch(hs, n, os_, n_opts, None, None, st.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert np.all(st == UNTOUCHED)
    return rc, L.nf_last_error().decode()


def test_refusals_touch_nothing(monkeypatch):
    """every refusal of the contract, each before any launch: status untouched, flux, warm state and history of every handle as they
    were.  The different-devices case needs two visible devices and does not run on a one-GPU machine: there it is NOT covered."""
    from neutfem_amd import capi
    from neutfem_amd.capi import HipSolver, HipTeam
    ARG, UNSUPPORTED = -1, -4
    good = _solvers((9, 8, 3), 0, 2, 3)
    good[0].solve_keff()                                                # one of them with a history and a warm state
    before = [_state(s, with_J=False) for s in good]
    L = good[0].L; o = [s.opts() for s in good]; h = [s.h for s in good]
    assert _raw(L, h, 0, o, 1)[0] == ARG and _raw(L, h, -2, o, 1)[0] == ARG
    rc, msg = _raw(L, [h[0], None, h[2]], 3, o, 3); assert rc == ARG and "NULL" in msg
    rc, msg = _raw(L, [h[0], h[1], h[0]], 3, o, 3); assert rc == ARG and "twice" in msg
    assert _raw(L, h, 3, o[:2], 2)[0] == ARG and _raw(L, h, 3, o, 0)[0] == ARG
    inp = synthetic_inputs(9, 8, 3, ng=2, seed=5)
    if capi.device_count() > 1:
        other = make_hip(inp, device=1)
        rc, msg = _raw(L, [h[0], other.h], 2, o, 1); assert rc == ARG and "device" in msg
        other.close()
    slab = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], interface_above=True)
    rc, msg = _raw(L, [h[0], slab.h, h[1]], 3, o, 3); assert rc == UNSUPPORTED and "slab" in msg
    slab.close()
    inp6 = synthetic_inputs(9, 8, 6, ng=2, seed=5)                      # a slab needs three z-planes
    team = HipTeam(0, 0, 2, inp6["x_breaks"], inp6["y_breaks"], inp6["z_breaks"], [(0, 3), (3, 6)])
    rc, msg = _raw(L, [h[0], team.head.h], 2, o, 1); assert rc == UNSUPPORTED and "slab" in msg
    team.close()
    # a handle with a communicator: a one-rank RCCL communicator on an undivided, built handle (NEUTFEM_FORCE_RCCL keeps it at one rank)
    monkeypatch.setenv("NEUTFEM_FORCE_RCCL", "1")
    lone = HipTeam(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], [(0, 3)])
    lone.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); lone.build()
    lone.comm_init(HipTeam.unique_id(), 1, 0)
    monkeypatch.delenv("NEUTFEM_FORCE_RCCL")
    assert lone.head.info("n_local_slabs") == 1
    rc, msg = _raw(L, [h[0], lone.head.h, h[1]], 3, o, 3); assert rc == UNSUPPORTED and "communicator" in msg and "collectives" in msg
    rc, msg = _raw(L, [lone.head.h], 1, o, 1); assert rc == UNSUPPORTED and "communicator" in msg
    lone.close()
    fresh = HipSolver(0, 0, 2, inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])          # not built
    k, n = C.c_double(), C.c_int()
    alone = L.nf_solve_keff(fresh.h, C.byref(o[0]), C.byref(k), C.byref(n))
    rc, msg = _raw(L, [h[0], h[1], fresh.h], 3, o, 3); assert rc == alone != 0 and "nf_build" in msg
    fresh.close()
    with pytest.raises(RuntimeError, match="twice"):
        capi.solve_keff_batch([good[0], good[0]])
    for s, b in zip(good, before):
        _same(_state(s, with_J=False), b)
    assert good[0].info("batch_launches") == 0
    k, no, st, res = capi.solve_keff_batch(good)                         # and the same handles still batch
    assert list(st) == [0, 0, 0] and res["n_batched"] == 3
    _close(good)


def _pybind(inp, tol):
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    s = ns.NeutFEM(0, 0, int(inp["ng"]), inp["x_breaks"], inp["y_breaks"], inp["z_breaks"])
    s.set_verbosity(ns.VerbosityLevel.SILENT)
    for a, t in zip(inp["bc_attr"], inp["bc_type"]):
        s.set_bc(int(a), ns.BCType(int(t)), 0.0)
    s.get_D()[...] = inp["D"]; s.get_SigR()[...] = inp["SigR"]; s.get_NSF()[...] = inp["NSF"]; s.get_Chi()[...] = inp["Chi"]; s.get_SigS()[...] = inp["SigS"]
    s.set_linear_solver(ns.LinearSolverType.BICGSTAB)
    s.set_tol(*tol)
    s.BuildMatrices()
    return s


def test_python_surfaces():
    """capi.solve_keff_batch is the raw C call; SolveKeffBatch over pybind objects agrees with it and leaves every object as SolveKeff does"""
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as ns
    from neutfem_amd import capi
    shape = (12, 11, 10)                                                # RT0-P0, 1320 unknowns per group: the one-workgroup solve by default
    inps = [synthetic_inputs(*shape, ng=2, seed=100 + i) for i in range(3)]
    tols = [TOL, (1e-6, 1e-6, 1e-7, 200, 2000), TOL]
    a, b = [make_hip(i) for i in inps], [make_hip(i) for i in inps]
    for l in (a, b):
        for s, t in zip(l, tols):
            s.set_tol(*t)
    k, no, st, res = capi.solve_keff_batch(a)
    hs = (C.c_void_p * 3)(*[s.h for s in b]); os_ = (capi.KeffOpts * 3)(*[s.opts() for s in b])
    kk, nn, ss = np.zeros(3), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    rb = capi.BatchResult()
    assert b[0].L.nf_solve_keff_batch(hs, 3, os_, 3, kk.ctypes.data_as(C.POINTER(C.c_double)), nn.ctypes.data_as(C.POINTER(C.c_int)),
                                      ss.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rb)) == 0
    assert np.array_equal(k, kk) and np.array_equal(no, nn) and np.array_equal(st, ss) and res == rb.as_dict()
    assert res == dict(n_batched=3, n_sequential=0, n_launches=1, variant=1) and no[1] < no[0]
    for x, y in zip(a, b):
        _same(_state(x), _state(y))
    objs = [_pybind(i, t) for i, t in zip(inps, tols)]
    ks = ns.SolveKeffBatch(objs)
    assert ns.get_batch_info() == dict(n_batched=3, n_sequential=0, n_launches=1, variant=1)
    for i, (obj, s) in enumerate(zip(objs, a)):
        assert abs(ks[i] - k[i]) <= 1e-12 * abs(k[i]) and obj.GetLastKeff() == ks[i]
        assert rel_l2(obj.get_flux().reshape(2, -1), s.get_phi()) <= 1e-12
    single = _pybind(inps[1], tols[1])
    assert abs(single.SolveKeff() - ks[1]) <= 1e-12 * abs(ks[1]) and rel_l2(single.get_flux(), objs[1].get_flux()) <= 1e-12
    ks2 = ns.SolveKeffBatch(objs)                                       # warm: the objects' own last k and flux go in
    assert all(abs(x - y) <= 1e-8 * abs(y) for x, y in zip(ks2, ks))
    objs[0].reset_flux()
    assert (objs[0].get_flux() == 1.0).all()
    _close(a, b)
