"""Tables of distinct lines in the streaming Schur passes (LineDict in neutfem_amd/csrc/nf_kernels.h, option "line_dict").

The table path reads the same factor bits as the streaming path and runs the same arithmetic, so the bar between the two is
np.array_equal, not a tolerance.  Every case first asserts through the launch-plan report (HipSolver.apply_plan, "dict" per pass and
"line_dict" per direction) that the pass under test takes its table -- or does not, where the case says so -- and only then checks numbers:

  apply        max |y - y_oracle| <= 1e-12 max |y_oracle| on every group, and bit-equal to the same handle under line_dict = 0
  fixed work   solve_keff, tol (0, 1e-11, 1e-11, 6, 3000): k-history and flux bit-equal between line_dict 0 and 1; k-history 1e-9 and
               flux 1e-8 against the oracle

Inputs: block-structured cross-sections -- a palette of four materials drawn with a fixed seed, one material per block of cells, every
cross-section piecewise constant, mesh widths exactly uniform (1.25) unless the case says otherwise.  The expected number of distinct
lines is counted with numpy on the inputs (bit patterns of the D sequence of a line, its SigR sequence for x lines, and the transverse
widths), never taken from the code under test.  Shapes: the ones tests/test_gpu_variants.py established as engaging the variants."""
import functools

import numpy as np
import pytest

from helpers import make_hip, make_oracle, rel_l2, synthetic_inputs

pytestmark = pytest.mark.gpu

OPTS = dict(resident=0, cg_fuse3=0, cg_xcd=0, nt_min_cells=0, line_dict=1)   # the four-launch CG, streaming instantiations at any size
FIXED = (0.0, 1e-11, 1e-11, 6, 3000)
A, A_BLK = (130, 8, 16), (13, 4, 8)
# A_long: the chunked kernel on y and z, inside CG with the split dot product (which the lean CG of small meshes does not take); A_split: the
# one-chunk kernel's z.w instantiation -- the two non-lean forms the big meshes run
CASES = {"A": (A, A_BLK, {}), "A_long": (A, A_BLK, dict(s_long=1, cg_lean=0)), "A_split": (A, A_BLK, dict(cg_lean=0, split_dot=2)),
         "B": ((70, 24, 4), (10, 6, 2), {}), "C": ((64, 40, 40), (8, 8, 8), {})}
FAMILY = {"A": "s", "A_long": "c", "A_split": "s", "B": "s", "C": "s"}


def block_inputs(shape, block, seed=11, ng=2, y_random=False):
    """piecewise-constant cross-sections on blocks of `block` cells; removal of 1 - 5 per cm, so that the inner CG converges in a few dozen iterations
    and the oracle's fixed-work solve of the largest shape takes three seconds"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    npal = 4
    pal = dict(D=rng.uniform(0.3, 1.8, (ng, npal)), SigR=rng.uniform(1.0, 5.0, (ng, npal)), NSF=rng.uniform(0.0, 0.3, (ng, npal)),
               S=rng.uniform(0.005, 0.05, npal))
    nb = [-(-n // b) for n, b in zip((nz, ny, nx), block[::-1])]
    mat = rng.integers(0, npal, nb)
    for ax, b in enumerate(block[::-1]):
        mat = np.repeat(mat, b, axis=ax)
    mat = mat[:nz, :ny, :nx]
    D, SigR, NSF = (np.stack([pal[k][g][mat] for g in range(ng)]) for k in ("D", "SigR", "NSF"))
    Chi = np.zeros((ng,) + mat.shape); Chi[0] = 0.8; Chi[1] = 0.2
    SigS = np.zeros((ng, ng) + mat.shape); SigS[1, 0] = pal["S"][mat]
    brk = lambda n: 1.25 * np.arange(n + 1)
    yb = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.5, ny))]) if y_random else brk(ny)
    return dict(x_breaks=brk(nx), y_breaks=yb, z_breaks=brk(nz), D=D, SigR=SigR, NSF=NSF, Chi=Chi, SigS=SigS, bc_attr=np.arange(1, 7),
                bc_type=np.zeros(6, int), coarse_factors=np.array([1, 1, 1]), kref=1.0, ng=ng)


def distinct_lines(inp):
    """distinct lines per direction, the largest group's: bit patterns of what the factors of a line are made from"""
    hx, hy, hz = (np.diff(inp[k]) for k in ("x_breaks", "y_breaks", "z_breaks"))
    nz, ny, nx = inp["D"].shape[1:]
    HX, HY, HZ = np.broadcast_to(hx, (nz, ny, nx)), np.broadcast_to(hy[:, None], (nz, ny, nx)), np.broadcast_to(hz[:, None, None], (nz, ny, nx))
    out = {}
    for name, axis, fields in (("x", 2, ("D", "SigR")), ("y", 1, ("D",)), ("z", 0, ("D",))):
        best = 0
        for g in range(int(inp["ng"])):
            cols = [inp[f][g] for f in fields] + [HX, HY, HZ]      # widths along the line and across it, per cell
            a = np.concatenate([np.moveaxis(c, axis, -1).reshape(-1, c.shape[axis]) for c in cols], axis=1)
            best = max(best, len(np.unique(np.ascontiguousarray(a).view(np.uint64), axis=0)))
        out[name] = best
    return out


def _set(s, opts):
    for k, v in opts.items():
        s.set_option(k, v)


def _vectors(n_phi, ng):
    rng = np.random.default_rng(3)
    xs = []
    for g in range(ng):
        x = rng.standard_normal(n_phi); x[rng.random(n_phi) < 0.1] *= 1e-12
        x.setflags(write=False); xs.append(x)
    return xs


def _oracle_applies(inp):
    o = make_oracle(inp)
    xs = _vectors(o.n_phi, int(inp["ng"]))
    return xs, [o.schur_apply(g, x) for g, x in enumerate(xs)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs and oracle side of one shape: applies and the fixed-work solve, computed once"""
    shape, block, _ = CASES[name]
    if name.startswith("A_"):
        return _case("A")
    inp = block_inputs(shape, block)
    xs, ys = _oracle_applies(inp)
    o = make_oracle(inp); o.set_tol(*FIXED); o.SolveKeff(); h = o.history()
    assert h["n_outer"] == FIXED[3]
    return dict(inp=inp, x=xs, y=ys, hk=h["k"].copy(), phi=o.phi_dofs().copy(), n=distinct_lines(inp))


def _check_plan(s, want, counts=None, families=None):
    """every pass of the next apply, outside and inside CG, reports dict == want[dir]; the distinct-line counts where given"""
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        for d in "xyz":
            assert plan[d]["dict"] == want[d], (in_cg, d, plan[d], plan["line_dict"])
            assert plan[d]["nt"] == 1, (d, plan[d])
            if plan[d]["family"] == "s":                            # the one-chunk kernel names its instantiation: the table next to the streaming loads
                assert plan[d]["variant"] == "+".join(["nt"] + ["zw"] * plan[d]["zw"] + ["dict"] * want[d]), (in_cg, d, plan[d])
            assert (plan["line_dict"][d] > 0) == bool(want[d]), plan["line_dict"]
            if counts is not None and want[d]:
                assert plan["line_dict"][d] == counts[d], (d, plan["line_dict"], counts)
        if families is not None and in_cg:
            assert [plan[d]["family"] for d in "yz"] == list(families), plan
    return plan


def _applies(s, xs, ys, label):
    out = []
    for g, (x, yo) in enumerate(zip(xs, ys)):
        y = s.schur_apply(g, x)
        err = np.abs(y - yo).max() / np.abs(yo).max()
        print(f"apply {label} g={g}: max-abs error / max|y| = {err:.3e} (bar 1e-12)")
        assert np.isfinite(y).all() and err <= 1e-12, (label, g, err)
        out.append(y)
    return out


def _same_bits(a, b, label):
    for g, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (label, g, float(np.abs(u - v).max()))


ALL, NONE = dict(x=1, y=1, z=1), dict(x=0, y=0, z=0)


def _on_off(inp, xs, ys, label, opts=None, want=ALL, counts=None):
    """the applies with the tables as `want` says, against the oracle and bit-equal to the same handle under line_dict = 0; returns the handle"""
    s = make_hip(inp); _set(s, dict(OPTS, **(opts or {})))
    _check_plan(s, want, counts)
    on = _applies(s, xs, ys, label)
    keep = s.info("line_dict_bytes"), s.info("line_dict_rejected")
    s.set_option("line_dict", 0)
    _check_plan(s, NONE)
    assert s.info("line_dict_bytes") == 0
    _same_bits(on, _applies(s, xs, ys, label + " line_dict=0"), label)
    s.set_option("line_dict", 1)
    return s, keep


# ---- the four shapes: apply and fixed-work solve ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_apply_and_solve(name):
    ref = _case(name)
    s = make_hip(ref["inp"]); _set(s, dict(OPTS, **CASES[name][2])); s.set_tol(*FIXED)
    fam = FAMILY[name]
    plan = _check_plan(s, ALL, ref["n"], (fam, fam))
    assert plan["x"]["NCH"] == (2 if name.startswith("A") else 1)
    if name in ("A_long", "A_split"):                                  # inside CG: per-pass shares of p.q in the z.w form
        assert plan["lean"] == 0 and plan["split_dot"] == 1 and plan["y"]["zw"] == 1 and plan["z"]["zw"] == 1, plan
    if name == "A_split":
        assert plan["y"]["variant"] == "nt+zw+dict" and plan["z"]["variant"] == "nt+zw+dict", plan
    assert 0 < s.info("line_dict_bytes") and s.info("line_dict_rejected") == 0
    on = _applies(s, ref["x"], ref["y"], name)
    k1, n1 = s.solve_keff(); h1 = s.history(); hk1, cg1, phi1 = h1["k"].copy(), h1["cg"].copy(), s.get_phi().copy()
    assert n1 == FIXED[3] and s.info("last_path") == 0
    errs = np.abs(hk1 / ref["hk"] - 1).max(), rel_l2(phi1.ravel(), ref["phi"].ravel())
    print(f"fixed work {name}: k-history {errs[0]:.3e} (bar 1e-9), flux {errs[1]:.3e} (bar 1e-8)")
    np.testing.assert_allclose(hk1, ref["hk"], rtol=1e-9)
    assert errs[1] < 1e-8
    s.close()
    s = make_hip(ref["inp"]); _set(s, dict(OPTS, line_dict=0, **CASES[name][2])); s.set_tol(*FIXED)   # a fresh handle: no state of the first solve
    _check_plan(s, NONE)
    _same_bits(on, _applies(s, ref["x"], ref["y"], name + " line_dict=0"), name)
    k0, n0 = s.solve_keff(); h0 = s.history()
    assert k0 == k1 and n0 == n1 and np.array_equal(h0["k"], hk1) and np.array_equal(h0["cg"], cg1) and np.array_equal(s.get_phi(), phi1)
    s.close()


# ---- lines that differ in one cell --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_cell(where):
    """shape A with six cells given a D of their own (group 0), no two of them on a common x, y or z line, two each at the first / a middle /
    the last cell of their x, y and z line: every direction gains exactly six distinct lines"""
    nx, ny, nz = A
    base = _case("A")
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base["inp"].items()}
    pos = lambda n: {"first": 0, "middle": n // 2 - 1, "last": n - 1}[where]
    cells = [(3, 1, pos(nx)), (9, 6, pos(nx) + (1 if where != "last" else -1)),       # (iz, iy, ix): along x
             (5, pos(ny), 40), (12, pos(ny) + (1 if where != "last" else -1), 77),     # along y
             (pos(nz), 3, 101), (pos(nz) + (1 if where != "last" else -1), 4, 17)]     # along z
    for ax in range(3):
        pairs = {tuple(c[i] for i in range(3) if i != ax) for c in cells}
        assert len(pairs) == 6
    for i, c in enumerate(cells):
        inp["D"][(0,) + c] *= 1.01 + 0.01 * i
    n = distinct_lines(inp)
    assert all(n[d] == base["n"][d] + 6 for d in "xyz"), (n, base["n"])
    xs, ys = _oracle_applies(inp)
    return dict(inp=inp, x=xs, y=ys, n=n)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_cell_differences(where):
    ref = _one_cell(where)
    s, _ = _on_off(ref["inp"], ref["x"], ref["y"], "one cell " + where, counts=ref["n"])
    s.close()


def test_x_lines_equal_in_D_but_not_in_SigR():
    """the x table carries the C diagonal: two x lines with the D of their neighbours and a SigR of their own in one cell get ids of their own"""
    base = _case("A")
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base["inp"].items()}
    inp["SigR"][1, 2, 5, 64] *= 1.5; inp["SigR"][1, 11, 2, 129] *= 1.25
    n = distinct_lines(inp)
    assert n["x"] == base["n"]["x"] + 2 and n["y"] == base["n"]["y"] and n["z"] == base["n"]["z"], (n, base["n"])
    xs, ys = _oracle_applies(inp)
    s, _ = _on_off(inp, xs, ys, "SigR only", counts=n)
    s.close()


def test_nonuniform_transverse_widths():
    """random y widths: x and z lines with equal materials but another hy are different lines; y lines stay as few as before"""
    inp = block_inputs(A, A_BLK, y_random=True)
    n, nu = distinct_lines(inp), _case("A")["n"]
    assert n["x"] > nu["x"] and n["z"] > nu["z"] and n["y"] == nu["y"], (n, nu)
    xs, ys = _oracle_applies(inp)
    s, _ = _on_off(inp, xs, ys, "random hy", counts=n)
    s.close()


# ---- inputs and options under which a direction must keep streaming ------------------------------------------------------------------
def test_no_repeats():
    inp = synthetic_inputs(*A, 2, seed=5)
    xs, ys = _oracle_applies(inp)
    s, (nbytes, rejected) = _on_off(inp, xs, ys, "no repeats", want=NONE)
    nlines = A[1] * A[2] + A[0] * A[2] + A[0] * A[1]
    assert rejected == 0 and nbytes <= 4 * 2 * nlines, nbytes           # nothing beyond the ids
    s.close()


def test_groups_differ():
    """group 0 block-structured, group 1 random: one decision per direction for all groups -- no table"""
    base = _case("A")
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base["inp"].items()}
    inp["D"][1] = np.random.default_rng(9).uniform(0.3, 1.8, inp["D"][1].shape)
    xs, ys = _oracle_applies(inp)
    s, (nbytes, rejected) = _on_off(inp, xs, ys, "groups differ", want=NONE)
    assert rejected == 0
    s.close()


def test_cap():
    """line_dict_max_bytes below the x table (rows x 144 doubles x 3 arrays) and above the y and z tables (rows x 16 or 32 doubles x 2)"""
    ref = _case("A")
    n = ref["n"]
    tx, ty, tz = n["x"] * 144 * 24, n["y"] * 16 * 16, n["z"] * 16 * 16
    assert max(ty, tz) < tx
    s, _ = _on_off(ref["inp"], ref["x"], ref["y"], "cap", opts=dict(line_dict_max_bytes=tx - 8), want=dict(x=0, y=1, z=1), counts=n)
    s.set_option("line_dict_max_bytes", tx)
    _check_plan(s, ALL, n)
    s.close()


@pytest.mark.parametrize("dirs", [1, 2, 4])
def test_single_direction(dirs):
    ref = _case("A")
    s, _ = _on_off(ref["inp"], ref["x"], ref["y"], "dirs=%d" % dirs, opts=dict(line_dict_dirs=dirs),
                   want=dict(x=dirs & 1, y=(dirs >> 1) & 1, z=(dirs >> 2) & 1), counts=ref["n"])
    s.close()


@pytest.mark.parametrize("long_lines", [0, 1])
def test_collisions_are_refused(long_lines):
    """two bits of fingerprint: different lines fall into one group, the bit-for-bit verification refuses the direction -- no wrong answer, no error"""
    ref = _one_cell("first")
    assert min(ref["n"].values()) > 4                                   # more distinct lines in every direction than two bits can tell apart
    s, (nbytes, rejected) = _on_off(ref["inp"], ref["x"], ref["y"], "fp_bits=2", opts=dict(line_dict_fp_bits=2, s_long=long_lines), want=NONE)
    assert rejected == 7 and nbytes == 0, (rejected, nbytes)
    s.set_option("line_dict_fp_bits", 128)
    _check_plan(s, ALL, ref["n"])
    assert s.info("line_dict_rejected") == 0
    s.close()


def test_rebuild_drops_the_tables():
    """another block pattern, then another boundary condition, into the same handle: the results follow the new input"""
    ref = _case("A")
    s = make_hip(ref["inp"]); _set(s, OPTS)
    _check_plan(s, ALL, ref["n"])
    _applies(s, ref["x"], ref["y"], "first pattern")
    inp2 = block_inputs(A, (10, 2, 4), seed=23)
    s.upload_xs(inp2["D"], inp2["SigR"], inp2["NSF"], inp2["Chi"], inp2["SigS"])
    assert s.info("line_dict_bytes") == 0
    s.build()
    xs, ys = _oracle_applies(inp2)
    n2 = distinct_lines(inp2)
    assert n2 != ref["n"]
    _check_plan(s, ALL, n2)
    _applies(s, xs, ys, "second pattern")
    # the upper x side from Dirichlet to the natural condition: the last factor of every x line changes
    inp3 = dict(inp2, bc_attr=np.array([1, 2, 3, 5, 6]), bc_type=np.zeros(5, int))
    s.set_bc(4, 1)
    assert s.info("line_dict_bytes") == 0
    s.build()
    o = make_oracle(inp3)
    ys3 = [o.schur_apply(g, x) for g, x in enumerate(xs)]
    assert not np.array_equal(ys3[0], ys[0])
    _check_plan(s, ALL, n2)
    _applies(s, xs, ys3, "natural condition on one x side")
    s.close()


def test_automatic_mode_stays_out_of_small_meshes():
    ref = _case("A")
    s = make_hip(ref["inp"]); _set(s, dict(resident=0, cg_fuse3=0, cg_xcd=0))
    for in_cg in (False, True):
        plan = s.apply_plan(in_cg)
        assert all(plan[d]["dict"] == 0 and plan[d]["nt"] == 0 for d in "xyz") and plan["line_dict"] == dict(x=0, y=0, z=0), plan
    _applies(s, ref["x"], ref["y"], "defaults")
    assert s.info("line_dict_bytes") == 0
    s.close()


def test_benchmark_mesh_engages_the_tables():
    """IAEA-3D at 256^3 with the options bench.py runs: the passes that ship enabled take their tables (12 / 12 / 3 distinct D sequences,
    18 x lines once SigR counts), built by the first solve or plan -- the golden run of tests/test_gpu_parity.py goes through them"""
    from bench import make_solver
    from neutfem_amd import cases
    s = make_solver(cases.iaea3d_resampled(256), 0)
    plan = s.apply_plan(True)
    print("256^3 plan:", plan["line_dict"], {d: (plan[d]["family"], plan[d]["dict"]) for d in "xyz"}, "bytes", s.info("line_dict_bytes"))
    assert s.info("line_dict_rejected") == 0
    assert plan["line_dict"] == dict(x=18, y=12, z=3), plan            # automatic mode ships all three directions
    assert [(plan[d]["family"], plan[d]["dict"], plan[d]["nt"]) for d in "xyz"] == [("x", 1, 1), ("c", 1, 1), ("s", 1, 1)], plan
    s.close()


@pytest.mark.parametrize("entry", ["apply", "solve_group"])
def test_first_apply_or_solve_builds_the_tables(entry):
    """no plan report beforehand: the first apply, or the first group solve, builds the tables itself"""
    ref = _case("A")
    s = make_hip(ref["inp"]); _set(s, OPTS)
    assert s.info("line_dict_bytes") == 0
    if entry == "apply":
        y = s.schur_apply(0, ref["x"][0])
    else:
        s.solve_group(0, np.abs(ref["x"][0]), 1e-8, 500)
    assert s.info("line_dict_bytes") > 0 and s.info("line_dict_rejected") == 0
    _check_plan(s, ALL, ref["n"])
    if entry == "apply":
        err = np.abs(y - ref["y"][0]).max() / np.abs(ref["y"][0]).max()
        assert err <= 1e-12, err
    s.close()
