"""The Schur apply per component at the benchmark's contrast: every launch variant against tests/apply_exact.py.

The other operator-level tests hold max |y - y_oracle| <= 1e-12 max |y_oracle|.  With IAEA-3D's filler (D = 1e-3, Sigma_R = 1e15) in a third of
the mesh, max |y| is 1e19 and 70 % of the cells lie below that bar whatever a kernel writes there (tests/test_apply_exact.py pins this).
Here the yardstick is the extended-precision apply and the metric is per component,

    rho = max_i |y_i - y_exact,i| / s_i,     s_i = |C_i x_i| + sum_d beta (|u_d,i| + |u_d,i+1|)

on f6_block_inputs (block-structured cross-sections with the filler as one of four materials, 28 - 30 % of the cells) and on the committed
benchmark inputs, with the input vector of the other files (normal, 10 % of the entries x 1e-12).  Every case first asserts through the
launch-plan report (HipSolver.apply_plan) that the variant under test is what the next apply launches, then checks rho on both groups.
Variants that are bit-equal on the synthetic inputs of the other files are asserted bit-equal here too.

Inside CG the passes are other instantiations (fused p.q partials, split dot product, lean, k_apply3, one-XCD kernel) that cannot be applied
alone: they are reached with solve_group(g, b, tol = 0, maxit = 2), b = |normal| on the cells that are not filler and 0 on the filler.  Two
CG steps from x = 0 give x2 = c b - a0 a1 S b with c = a0 + a1 (1 + b0); the reference is the same two steps in extended precision
(apply_exact.exact_cg2) and the scale is |c| b_i + a0 a1 s_i(b).  |x2| runs from 1e-18 in the filler to 0.8 in the fuel.
The resident one-workgroup kernel is launched by solve_keff only, never by solve_group: it is reached with ONE outer iteration from the
flat flux, tol (0, 0, 0, 1, 2) -- two CG steps per group on b_0 = chi_0 F and b_1 = chi_1 F + Sigma_s(0 -> 1) V x2_0, F = sum_g nuSigma_f,g V,
which vanish on the filler like the b above.  The kernel returns the normalised iterate; the one scalar is fitted on group 0
(phi_0 . x2_0 / x2_0 . x2_0, in extended precision) and both groups are then judged per component with that scalar.

Slab teams: HipTeam.schur_apply (the chain-solve endpoint pass, with and without separator sweeps) under endpoint_weights 0 and 1 -- the
weights are measured at build time through that chain solve, at this contrast; the weighted pass itself (k_endpoint_w) runs inside the
single-reduction CG only and is asserted in the in-CG plan.

Higher orders (RT1-P1, RT2-P2): the scale |C| |x| + |B| |u|, u = A^-1 B^T x, comes from the scipy twin's matrices.  Two checks (see
test_higher_orders for what the first run found): against the double oracle, four times the oracle's own error measured in the test on the same
case and group -- its rho against the twin or against the twin's operator with exact local tables (apply_exact.ExactTwin), whichever is
larger; and against that exact operator, rho <= K_HIGHER x 2^-53.

Bars: rho <= K x 2^-53, K_APPLY for the applies and K_SOLVE for the two-step solves (tests/apply_exact.py), and never more than 100 x the
oracle's own rho on the same input (a condition, not a measurement).  K = the next power of two at or above 4 x the largest rho x 2^53 measured on an MI355X:

  largest rho x 2^53 over the groups (and over the twins of a case)                          gpu   oracle
  apply  default plan: A / B / C / iaea3d / iaea3d_1x1 / iaea2d        4.6 3.8 3.5 4.7 3.9 3.4   8.8 10.9 8.2 10.8 7.4 5.5
  apply  streaming, nt_loads 1 and 0 (bit-equal): A / B / C                      4.6 3.8 3.5   8.8 10.9 8.2
  apply  xcd 0 and 7 (bit-equal): A / C                                              4.6 3.5   8.8 8.2
  apply  chunked, s_long_dirs 1 / 2 / 3, s_tx 0 / 16 / 64, c_early 0 / 1 / 2 (A)          4.6   8.8
  apply  line_dict 1 and 0 (bit-equal): A, A_long, A_split / B / D               4.6 3.8 4.3   8.8 10.9 14.1
  apply  slab teams 2 x 48 / 3 x 32 / thin, endpoint_weights 0 and 1 (T)         4.4 3.4 4.4   10.9
  apply  tests/test_gpu_parity.py::_apply_case, 21 inputs (largest of each side)          8.4   29.1
  cg2    four-launch lean 1 / 0, x_two_phase 1 / 0 (retired key: bit-equal), line_dict 1 / 0 (A)    1237.7   3178.2
  cg2    split_dot 2, chunked kernel in CG, A_long, A_split (A)                        1241.1   3178.2
  cg2    k_apply3 (A)                                                                  1240.0   3178.2
  cg2    line_dict 1 and 0 (bit-equal): B / D                                     184.9 610.3   1301.7 2348.5
  cg2    one-XCD kernel / k_apply3 (W)                                              39.8 40.5   187.1
  cg2    resident kernel, one outer: line-per-lane / scans / one-sided / no LDS (R)       7.9   66.1
  cg2    k_keff_xcd, one outer (W)                                                       6.5   490.9
  K_APPLY = 64 (4 x 8.4 = 34), K_SOLVE = 8192 (4 x 1241 = 4964).  No case is above its oracle: the scan-based line solves lose nothing to
  the band LDL^T at a 1/D contrast of 2000.  The two-step solves sit at 1e3 x 2^-53 on either side because alpha_1 = |r1|^2 / p1.S p1 is
  dominated by the filler cells (C = 2e15 against p1 = -a0 (S b)_i) and inherits the error of (S b)_i where the face terms cancel.
  higher orders, against the twin's operator with exact tables: gpu 34.7 / 25.0 (RT1-P1), 30.3 / 26.5 (RT2-P2); oracle 247 / 222, 281 / 454;
  twin 97 / 145, 271 / 436; gpu versus oracle 228 / 230, 289 / 427; oracle versus twin 237 / 267, 89 / 93.  K_HIGHER = 256 (4 x 34.7 = 139).
"""
import functools

import numpy as np
import pytest

from apply_exact import EPS, K_APPLY, K_HIGHER, K_SOLVE, LD, ExactApply, ExactTwin, exact_cg2, f6_block_inputs, f6_mask, input_vector, rho
from helpers import load_inputs, make_hip, make_oracle
from neutfem_amd.capi import HipTeam
from test_gpu_line_dict import distinct_lines

pytestmark = pytest.mark.gpu

F6 = {"A": ((130, 8, 16), (13, 4, 8)), "B": ((70, 24, 4), (10, 6, 2)), "C": ((130, 9, 7), (13, 3, 7)),
      "D": ((64, 40, 40), (8, 8, 8)),                             # shape C of tests/test_gpu_line_dict.py
      "W": ((30, 28, 9), (10, 7, 3)),                             # inside the one-XCD window (tests/test_gpu_variants.py section f)
      "T": ((16, 8, 96), (4, 4, 8)),                              # slab teams
      "R": ((12, 11, 10), (4, 4, 5))}                             # the resident kernel's shape in tests/test_gpu_variants.py and tests/test_gpu_paths.py
STREAM = dict(resident=0, cg_fuse3=0, cg_xcd=0, nt_min_cells=0, line_dict=0)   # the four-launch CG, streaming instantiations at any size, no tables
TABLES = dict(STREAM, line_dict=1)


def _set(s, opts):
    for k, v in opts.items():
        s.set_option(k, v)


# ---- references: computed once per input, shared, never modified -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name):
    return f6_block_inputs(*F6[name]) if name in F6 else load_inputs(name)


@functools.lru_cache(maxsize=None)
def _ref(name, groups=None):
    """per group: input vector, exact apply, scale, and the oracle's own rho"""
    inp = _inputs(name)
    o = make_oracle(inp)
    out = dict(inp=inp, groups=tuple(range(int(inp["ng"]))) if groups is None else groups, x={}, y={}, s={}, rho_o={})
    for g in out["groups"]:
        x = input_vector(o.n_phi, g)
        y, s = ExactApply(inp, g).apply(x)
        out["x"][g], out["y"][g], out["s"][g], out["rho_o"][g] = x, y, s, rho(o.schur_apply(g, x), y, s)
    return out


@functools.lru_cache(maxsize=None)
def _ref_cg(name):
    """per group: right-hand side, the exact two CG steps, their scale, and the oracle's own rho"""
    inp = _inputs(name)
    o = make_oracle(inp); o.set_tol(1e-5, 0.0, 0.0, 200, 2)
    out = dict(inp=inp, groups=tuple(range(int(inp["ng"]))), x={}, y={}, s={}, rho_o={})
    for g in out["groups"]:
        b = np.abs(np.asarray(input_vector(o.n_phi, g))) * ~f6_mask(inp, g)
        b.setflags(write=False)
        x2, sc = exact_cg2(inp, g, b)
        xo, _, its = o.solve_group(g, b, with_J=False)
        assert its == 2
        out["x"][g], out["y"][g], out["s"][g], out["rho_o"][g] = b, x2, sc, rho(xo, x2, sc)
    return out


def _judge(kind, label, g, got, ref):
    r, ro = rho(got, ref["y"][g], ref["s"][g]), ref["rho_o"][g]
    K = K_APPLY if kind == "apply" else K_SOLVE
    print(f"RHO {kind} {label} g={g}: gpu {r:.2e} = {r / EPS:.1f} x 2^-53 (bar {K}), oracle {ro:.2e} = {ro / EPS:.1f} x 2^-53, gpu / oracle {r / ro:.1f}")
    assert np.isfinite(got).all(), (label, g)
    assert r <= K * EPS, (kind, label, g, r / EPS)
    assert r <= 100 * max(ro, EPS), (kind, label, g, r, ro)        # beyond that it is a finding, not a rounding order (an oracle that is exact on a tiny input sets no bar)


def _applies(s, ref, label, team_shape=None):
    """the apply on every group of the reference against the exact one; returns the outputs"""
    out = []
    for g in ref["groups"]:
        if team_shape is None: y = s.schur_apply(g, ref["x"][g])
        else: y = s.schur_apply(g, np.asarray(ref["x"][g]).reshape(team_shape)).ravel()
        _judge("apply", label, g, y, ref)
        out.append(y)
    return out


def _solves(s, ref, label):
    """two CG steps on every group against the exact ones; returns the iterates"""
    out = []
    for g in ref["groups"]:
        x, its, _ = s.solve_group(g, ref["x"][g], 0.0, 2)
        assert its == 2, (label, g, its)
        _judge("cg2", label, g, x, ref)
        out.append(x)
    return out


def _same_bits(a, b, label):
    for g, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (label, g, float(np.abs(u - v).max()))


# ---- default plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "iaea3d", "iaea3d_1x1", "iaea2d"])
def test_default_plan(name):
    ref = _ref(name)
    s = make_hip(ref["inp"])
    plan = s.apply_plan()
    dirs = "xyz"[:s.info("dim")]
    assert plan["in_cg"] == 0 and plan["slab"] == 0 and [p["dir"] for p in plan["passes"]] == list(dirs), plan
    for d in dirs:                                                 # small meshes: plain loads, no tables, one-chunk y / z passes
        assert plan[d]["family"] == ("x" if d == "x" else "s") and plan[d]["nt"] == 0 and plan[d]["dict"] == 0, (d, plan[d])
    assert plan["line_dict"] == dict(x=0, y=0, z=0)
    _applies(s, ref, "default " + name)
    s.close()


# ---- four-launch streaming passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_streaming_and_plain_loads(name):
    """nt_loads 1 / 0: the same arithmetic under other load instructions -- bit-equal"""
    ref = _ref(name)
    s = make_hip(ref["inp"]); _set(s, STREAM)
    res = {}
    for nt in (1, 0):
        s.set_option("nt_loads", nt)
        for in_cg in (False, True):
            plan = s.apply_plan(in_cg)
            for d in "xyz":
                want = nt if (d != "x" or F6[name][0][0] % 2 == 0) else 0      # the streaming x pass reads pairs: even nx
                assert plan[d]["family"] == ("x" if d == "x" else "s") and plan[d]["nt"] == want and plan[d]["dict"] == 0, (nt, d, plan[d])
        res[nt] = _applies(s, ref, f"{name} nt_loads={nt}")
    _same_bits(res[1], res[0], "nt_loads")
    s.close()


GRIDS = {"A": dict(x=[32, 1, 1], y=[3, 16, 1], z=[3, 8, 1]), "C": dict(x=[16, 1, 1], y=[3, 7, 1], z=[3, 9, 1])}


@pytest.mark.parametrize("name,moves", [("A", "xyz"), ("C", "x")])
def test_xcd_tile_order(name, moves):
    """xcd = 7 on A: the tiles of all three passes move; on C no y / z tile count is a multiple of 8 -- requested, and falls back to the natural
    order.  Partials are stored by position: bit-equal to xcd = 0"""
    ref = _ref(name)
    s = make_hip(ref["inp"]); _set(s, dict(STREAM, xcd=0))
    assert all(s.apply_plan()[d]["xcd_order"] == 0 for d in "xyz")
    base = _applies(s, ref, f"{name} xcd=0")
    s.set_option("xcd", 7)
    plan = s.apply_plan()
    for d in "xyz":
        assert plan[d]["grid"] == GRIDS[name][d] and plan[d]["nt"] == 1 and plan[d]["xcd_order"] == 1, (d, plan[d])
    assert "".join(d for d in "xyz" if plan[d]["xcd_permutes"]) == moves, plan["passes"]
    _same_bits(_applies(s, ref, f"{name} xcd=7"), base, "xcd=7")
    s.close()


# ---- chunked kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dirs", [1, 2, 3])
def test_chunked_kernel(dirs):
    """s_long = 1 on y, z or both, tile widths 32 (default) / 16 / 64, on its tables with early loads of level 0 / 1 / 2 (which move loads
    only: bit-equal across the levels)"""
    ref = _ref("A")
    nx = F6["A"][0][0]
    s = make_hip(ref["inp"]); _set(s, dict(TABLES, s_long=1, s_long_dirs=dirs))
    fam = dict(y="c" if dirs & 1 else "s", z="c" if dirs & 2 else "s")
    counts = distinct_lines(ref["inp"])
    for tx in (0, 16, 64):
        s.set_option("s_tx", tx)
        res = {}
        for early in (0, 1, 2):
            s.set_option("c_early", early)
            plan = s.apply_plan()
            for d in "yz":
                p = plan[d]
                assert p["family"] == fam[d] and p["nt"] == 1 and p["dict"] == 1 and plan["line_dict"][d] == counts[d], (d, p, plan["line_dict"])
                if fam[d] == "c":
                    assert p["NCH"] == 2 and p["TX"] == (tx or 32) and p["grid"][0] == -(-nx // (tx or 32)) and p["early"] == early, p
                else:
                    assert p["early"] == 0 and p["TX"] == (tx or 64), p
            res[early] = _applies(s, ref, f"A s_long_dirs={dirs} s_tx={tx} c_early={early}")
        _same_bits(res[1], res[0], "c_early=1"); _same_bits(res[2], res[0], "c_early=2")
    s.close()


# ---- tables of distinct lines ----------------------------------------------------------------------------------------------------
LINE_CASES = {"A": ("A", {}), "A_long": ("A", dict(s_long=1, cg_lean=0)), "A_split": ("A", dict(cg_lean=0, split_dot=2)), "B": ("B", {}), "D": ("D", {})}
FAMILY = {"A": "s", "A_long": "c", "A_split": "s", "B": "s", "D": "s"}


@pytest.mark.parametrize("case", list(LINE_CASES))
def test_line_tables(case):
    """line_dict 1 against 0 on the cases of tests/test_gpu_line_dict.py rebuilt with the filler palette: the distinct-line count is the one
    numpy counts on the inputs, both sides hold the bar, and they are bit-equal -- outside CG and in the two CG steps"""
    name, extra = LINE_CASES[case]
    ref, cg = _ref(name), _ref_cg(name)
    counts = distinct_lines(ref["inp"])
    s = make_hip(ref["inp"]); _set(s, dict(TABLES, **extra))
    res = {}
    for on in (1, 0):
        s.set_option("line_dict", on)
        for in_cg in (False, True):
            plan = s.apply_plan(in_cg)
            for d in "xyz":
                assert plan[d]["dict"] == on and plan[d]["nt"] == 1 and plan["line_dict"][d] == (counts[d] if on else 0), (on, in_cg, d, plan[d], plan["line_dict"], counts)
            if in_cg:
                assert [plan[d]["family"] for d in "yz"] == [FAMILY[case]] * 2, plan["passes"]
                if "cg_lean" in extra:
                    assert plan["lean"] == 0 and plan["split_dot"] == 1 and plan["y"]["zw"] == 1 and plan["z"]["zw"] == 1, plan
        assert (s.info("line_dict_bytes") > 0) == bool(on) and s.info("line_dict_rejected") == 0
        res[on] = (_applies(s, ref, f"{case} line_dict={on}"), _solves(s, cg, f"{case} line_dict={on}"))
    _same_bits(res[1][0], res[0][0], "apply line_dict"); _same_bits(res[1][1], res[0][1], "cg2 line_dict")
    s.close()


# ---- inside CG -------------------------------------------------------------------------------------------------------------------
def _plan_lean(plan, lean):
    assert plan["in_cg"] == 1 and plan["fused"] == 1 and plan["lean"] == lean and plan["split_dot"] == 0, plan
    assert all(plan[d]["family"] == ("x" if d == "x" else "s") and plan[d]["nt"] == 1 for d in "xyz"), plan["passes"]
    assert plan["z"]["zw"] == 0, plan["z"]                         # the whole p.q in the last pass


@pytest.mark.parametrize("lean", [1, 0])
def test_cg_four_launch(lean):
    ref = _ref_cg("A")
    s = make_hip(ref["inp"]); _set(s, dict(STREAM, cg_lean=lean))
    _plan_lean(s.apply_plan(True), lean)
    _solves(s, ref, f"A four-launch cg_lean={lean}")
    assert s.info("last_xcd") == 0
    s.close()


def test_cg_split_dot():
    """per-pass shares of p.q, the y / z passes in the z.w form (what the big meshes run)"""
    ref = _ref_cg("A")
    s = make_hip(ref["inp"]); _set(s, dict(STREAM, cg_lean=0, split_dot=2))
    plan = s.apply_plan(True)
    assert plan["lean"] == 0 and plan["split_dot"] == 1 and plan["y"]["zw"] == 1 and plan["z"]["zw"] == 1, plan
    assert all(plan[d]["family"] == "s" and plan[d]["nt"] == 1 for d in "yz")
    _solves(s, ref, "A split_dot=2")
    s.close()


def test_cg_chunked_kernel():
    ref = _ref_cg("A")
    s = make_hip(ref["inp"]); _set(s, dict(STREAM, s_long=1, cg_lean=0, split_dot=1))
    plan = s.apply_plan(True)
    assert plan["lean"] == 0 and plan["split_dot"] == 1, plan
    for d in "yz":
        assert plan[d]["family"] == "c" and plan[d]["NCH"] == 2 and plan[d]["zw"] == 1 and plan[d]["nt"] == 1, (d, plan[d])
    _solves(s, ref, "A chunked in CG")
    s.close()


def test_cg_x_pass_two_load_phases():
    """the two-phase x pass is retired (docs/HISTORY.md): the key is still accepted, the plan no longer reports "p2", and it changes no bit"""
    ref = _ref_cg("A")
    res = {}
    for p2 in (1, 0):
        s = make_hip(ref["inp"]); _set(s, dict(STREAM, x_two_phase=p2, cg_fuse=1))
        plan = s.apply_plan(True)
        assert plan["fused"] == 1 and plan["x"]["NCH"] == 2 and plan["x"]["nt"] == 1 and "p2" not in plan["x"], plan["x"]
        assert "p2" not in s.apply_plan(False)["x"]
        res[p2] = _solves(s, ref, f"A x_two_phase={p2}")
        s.close()
    _same_bits(res[1], res[0], "x_two_phase")


def test_cg_fused_directions():
    """k_apply3 (cg_fuse3 = 1, the default of meshes up to 400 k cells): two launches per iteration.  The report has no entry for it; that it
    ran shows in the bits, which differ from the four-launch CG's (another summation order of p.q), while rho holds"""
    ref = _ref_cg("A")
    s = make_hip(ref["inp"]); _set(s, dict(resident=0, cg_fuse3=1, cg_xcd=0))
    assert s.apply_plan(True)["lean"] == 1                         # k_apply3 rides on the lean CG
    x3 = _solves(s, ref, "A cg_fuse3=1")
    assert s.info("last_xcd") == 0
    s.set_option("cg_fuse3", 0)
    x4 = _solves(s, ref, "A cg_fuse3=0 plain loads")
    assert any(not np.array_equal(u, v) for u, v in zip(x3, x4))
    s.close()


def test_cg_one_xcd():
    """k_cg_xcd: the whole solve as one launch on one XCD (default inside its window of 2 000 ... 28 000 unknowns, x lines up to 128 cells)"""
    ref = _ref_cg("W")
    s = make_hip(ref["inp"]); _set(s, dict(resident=0, cg_xcd=1))
    _solves(s, ref, "W one-XCD")
    assert s.info("last_xcd") == 1 and s.info("xcd_solves") == len(ref["groups"]) and s.info("xcd_refused") == 0
    s.set_option("cg_xcd", 0)
    _solves(s, ref, "W cg_xcd=0 (k_apply3)")
    assert s.info("last_xcd") == 0 and s.info("xcd_solves") == len(ref["groups"])
    s.close()


# ---- resident kernel -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_outer(name):
    """one outer iteration from the flat flux with two CG steps per group, in extended precision; the oracle's own rho under the same scalar fit"""
    inp = _inputs(name)
    ng, cells = int(inp["ng"]), inp["D"][0].size
    assert ng == 2
    V = np.einsum("k,j,i->kji", *(np.diff(inp[k]) for k in ("z_breaks", "y_breaks", "x_breaks"))).ravel()
    F = (inp["NSF"].reshape(ng, cells) * V).sum(axis=0)           # fission source of phi = 1
    out = dict(inp=inp, groups=(0, 1), y={}, s={}, rho_o={})
    b0 = inp["Chi"].reshape(ng, cells)[0] * F
    out["y"][0], out["s"][0] = exact_cg2(inp, 0, b0)
    b1 = inp["Chi"].reshape(ng, cells)[1] * F + inp["SigS"].reshape(ng, ng, cells)[1, 0] * V * np.asarray(out["y"][0], dtype=np.float64)
    out["y"][1], out["s"][1] = exact_cg2(inp, 1, b1)
    assert not b0[f6_mask(inp)].any() and not b1[f6_mask(inp)].any() and b0.max() > 0 and b1.max() > 0
    o = make_oracle(inp); o.set_tol(0.0, 0.0, 0.0, 1, 2); o.SolveKeff()
    assert o.history()["n_outer"] == 1 and (o.history()["cg"] == 2).all()
    for g, r in enumerate(_outer_rho(o.phi_dofs(), out)):
        out["rho_o"][g] = r
    return out


def _outer_rho(phi, ref):
    phi = np.asarray(phi).reshape(2, -1).astype(LD)
    c = (phi[0] * ref["y"][0]).sum() / (ref["y"][0] * ref["y"][0]).sum()
    return [rho(phi[g] / c, ref["y"][g], ref["s"][g]) for g in (0, 1)]


RESIDENT = {"line-per-lane": ({}, 1), "scans": (dict(resident_serial=0), 0), "one-sided": (dict(resident_two_sided=0), 1), "no-lds": (dict(resident_lds=0), 0)}


@pytest.mark.parametrize("variant", list(RESIDENT))
def test_resident_kernel(variant):
    ref = _ref_outer("R")
    opts, serial = RESIDENT[variant]
    s = make_hip(ref["inp"]); _set(s, dict(resident=1, resident_max_dofs=100000, **opts)); s.set_tol(0.0, 0.0, 0.0, 1, 2)
    k, n = s.solve_keff()
    assert n == 1 and s.info("last_path") == 2 and s.info("last_resident_serial") == serial and (s.history()["cg"] == 2).all(), (n, s.info("last_path"), s.history()["cg"])
    phi = s.get_phi()
    assert np.isfinite(phi).all()
    for g, r in enumerate(_outer_rho(phi, ref)):
        ro = ref["rho_o"][g]
        print(f"RHO cg2 R resident {variant} g={g}: gpu {r:.2e} = {r / EPS:.1f} x 2^-53 (bar {K_SOLVE}), oracle {ro:.2e} = {ro / EPS:.1f} x 2^-53, gpu / oracle {r / ro:.1f}")
        assert r <= K_SOLVE * EPS and r <= 100 * ro, (variant, g, r / EPS, ro / EPS)
    s.close()


def test_keff_one_xcd():
    """k_keff_xcd: the whole power iteration as one launch on one XCD (last_path 3), one outer iteration on W like the resident kernel on R;
    also held to 4 x the oracle's own rho, the bar of tests/test_gpu_orders_exact.py"""
    ref = _ref_outer("W")
    s = make_hip(ref["inp"]); _set(s, dict(resident=0, keff_xcd=1, cg_xcd=1)); s.set_tol(0.0, 0.0, 0.0, 1, 2)
    assert s.apply_plan(True)["form"] == "xcd"
    k, n = s.solve_keff()
    assert n == 1 and s.info("last_path") == 3 and s.info("xcd_refused") == 0 and (s.history()["cg"] == 2).all(), (n, s.info("last_path"), s.history()["cg"])
    phi = s.get_phi()
    assert np.isfinite(phi).all()
    for g, r in enumerate(_outer_rho(phi, ref)):
        ro = ref["rho_o"][g]
        print(f"RHO cg2 W k_keff_xcd g={g}: gpu {r:.2e} = {r / EPS:.1f} x 2^-53 (bar {K_SOLVE}), oracle {ro:.2e} = {ro / EPS:.1f} x 2^-53, gpu / oracle {r / ro:.1f}")
        assert r <= K_SOLVE * EPS and r <= 4 * ro, (g, r / EPS, ro / EPS)
    s.close()


# ---- slab teams ------------------------------------------------------------------------------------------------------------------
SPLITS = {"2x48": [(0, 48), (48, 96)], "3x32": [(0, 32), (32, 64), (64, 96)], "thin": [(0, 10), (10, 22), (22, 40), (40, 96)]}


@pytest.mark.parametrize("weights", [0, 1])
@pytest.mark.parametrize("split", list(SPLITS))
def test_slab_teams(split, weights):
    ref = _ref("T")
    inp = ref["inp"]
    nx, ny, nz = F6["T"][0]
    t = HipTeam(0, 0, int(inp["ng"]), inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], SPLITS[split])
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"]); t.build()
    _set(t.head, dict(cg_single_reduce=1, endpoint_weights=weights))
    _applies(t, ref, f"T {split} endpoint_weights={weights}", team_shape=(nz, ny, nx))   # prepares the team: the report needs its sweeps and weights
    print(f"team {split}: separator sweeps {t.head.timers()['separator_sweeps']}")
    for x in t.slabs:
        plan = x.apply_plan(False)
        assert plan["slab"] == 1 and plan["z1"]["family"] == "s" and plan["z2"]["family"] == "s", plan["passes"]   # outside CG: the chain solve
        cgp = x.apply_plan(True)
        assert cgp["single_reduce"] == 1 and cgp["z1"]["family"] == ("endpoint_w" if weights else "s"), cgp["passes"]
    t.close()


# ---- higher orders ---------------------------------------------------------------------------------------------------------------
HIGHER = {"rt1": ((70, 8, 8), (10, 4, 4), 1), "rt2": ((12, 6, 5), (4, 3, 5), 2)}
HO_GRIDS = {"rt1": dict(x=[16, 4, 1], y=[2, 8, 4], z=[2, 8, 4])}      # four transverse modes in gridDim.z (tests/test_gpu_variants.py, shape R)


@functools.lru_cache(maxsize=None)
def _ref_higher(name):
    """per group: the double oracle's apply, the twin's operator with exact tables in extended precision (apply and the scale |C| |x| + |B| |u|),
    and the rho of the oracle against the twin and of both against the exact operator"""
    from subcrit_exact import ref_from_inputs
    shape, block, rt = HIGHER[name]
    inp = f6_block_inputs(shape, block)
    o, r = make_oracle(inp, rt, rt), ref_from_inputs(inp, rt, rt)
    ex = ExactTwin(r)
    out = dict(inp=inp, rt=rt, x=[], yo=[], y=[], s=[], rho_ot=[], rho_o=[], rho_t=[])
    for g in range(int(inp["ng"])):
        x = input_vector(o.n_phi, g)
        y, s, du = ex.apply(g, x)
        assert du <= 1e-18, du                                        # the refinement has converged
        yo, yt = o.schur_apply(g, x).copy(), r.schur_apply(g, np.asarray(x))
        out["x"].append(x); out["yo"].append(yo); out["y"].append(y); out["s"].append(s)
        out["rho_ot"].append(rho(yo, yt.astype(LD), s)); out["rho_o"].append(rho(yo, y, s)); out["rho_t"].append(rho(yt, y, s))
    return out


@pytest.mark.parametrize("name", list(HIGHER))
def test_higher_orders(name):
    """Found by this test: with the bar first set for it, gpu-versus-oracle <= 4 x the oracle-versus-twin rho, RT2-P2 missed (289 and 427 x 2^-53
    against 89 and 93; RT1-P1 held, 228 / 230 against 237 / 267).  The cause is not the kernel: the oracle and the twin share the reference's
    Gauss table, tabulated to 15 digits, so their mutual distance leaves out the error both carry -- against the operator with exact tables
    they sit at 221 ... 454 x 2^-53, the kernels (closed forms of the condensed line blocks) at 25 ... 35.  Hence the two checks below."""
    ref = _ref_higher(name)
    rt = ref["rt"]
    for label, opts in (("default", {}), ("streaming", dict(resident=0, cg_fuse3=0, cg_xcd=0, nt_min_cells=0))):
        s = make_hip(ref["inp"], rt, rt); _set(s, opts)
        plan = s.apply_plan()
        assert s.info("rt_order") == rt and s.info("p_order") == rt
        for d in "xyz":
            assert plan[d]["family"] == ("x" if d == "x" else "s") and plan[d]["nt"] == 0 and plan[d]["dict"] == 0, (d, plan[d])   # streaming loads: RT0-P0 only
            if name in HO_GRIDS:
                assert plan[d]["grid"] == HO_GRIDS[name][d], (d, plan[d])
        for g in range(len(ref["x"])):
            y = s.schur_apply(g, ref["x"][g])
            r, rgo = rho(y, ref["y"][g], ref["s"][g]), rho(y, ref["yo"][g].astype(LD), ref["s"][g])
            ro, rt_, rot = ref["rho_o"][g], ref["rho_t"][g], ref["rho_ot"][g]
            print(f"RHO higher {name} {label} g={g}: against the exact operator x 2^-53: gpu {r / EPS:.1f} (bar {K_HIGHER}), oracle {ro / EPS:.1f}, twin {rt_ / EPS:.1f}; "
                  f"gpu vs oracle {rgo / EPS:.1f}, oracle vs twin {rot / EPS:.1f}")
            assert np.isfinite(y).all()
            assert r <= K_HIGHER * EPS and r <= 100 * ro, (name, label, g, r / EPS, ro / EPS)
            # against the double oracle: four times the reference's own error -- its distance from the twin or from the exact operator, whichever is larger
            assert rgo <= 4 * max(rot, ro), (name, label, g, rgo / EPS, rot / EPS, ro / EPS)
        s.close()
