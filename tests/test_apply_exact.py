"""tests/apply_exact.py pinned on the CPU: the extended-precision apply against the oracle and the scipy twin, and what its per-component
metric rho = max_i |y_i - y_exact,i| / s_i sees that the normwise metric of the other operator-level tests cannot.

Bars.  The oracle (band LDL^T of the face matrix in double) and the twin (SuperLU of an independently assembled matrix) are two more
evaluation orders of the same sum, so both sit at a few units of 2^-53 of the scale:
  oracle  rho <= 64 x 2^-53 (7.1e-15) on every case and group; measured here 0.4e-15 ... 4.0e-15
  twin    measured 0.5e-15 ... 3.1e-15 on the five small cases; the same bar of 64 x 2^-53 holds it with the same margin
Sensitivity: one entry of the oracle's own output times 1 + 1e-9, in a cell that is not filler, moves rho to |y_i| / s_i x 1e-9 and the
normwise metric by |y_i| / max |y| x 1e-9 = 1e-24 or so.  The cell is the first one of its kind (line end / block seam / interior, in
cell order) whose |y_i| >= 0.2 s_i, so that rho > 1e-10 follows from the arithmetic and not from luck."""
import functools

import numpy as np
import pytest

from apply_exact import (CURRENT_FAMILIES, EPS, LD, ORDER_BAR, ORDER_CASES, P0_CASES, ExactApply, ExactTwin, current_classes, currents_bar, currents_cg_oracle,
                         currents_outer_oracle, exact_cg2, exact_cg2_op, exact_outer_p0, f6_block_inputs, f6_mask, gauss_legendre_ld, input_vector,
                         normwise, order_case, order_ref_cg, order_ref_outer, order_start_flux, p0_case, rho, rough_start)
from helpers import load_inputs, make_oracle, rel_l2, synthetic_inputs

BAR = 64 * EPS
F6_SHAPES = {"A": ((130, 8, 16), (13, 4, 8)), "B": ((70, 24, 4), (10, 6, 2)), "C": ((130, 9, 7), (13, 3, 7))}

CASES = {
    "1d": lambda: synthetic_inputs(9, 1, 1, 2, seed=21),
    "2d": lambda: synthetic_inputs(12, 7, 1, 2, seed=22),
    "2d-mixed": lambda: synthetic_inputs(12, 7, 1, 2, seed=22, dirichlet=(2, 3)),
    "3d": lambda: synthetic_inputs(8, 6, 5, 2, seed=23),
    "3d-mixed": lambda: synthetic_inputs(8, 6, 5, 2, seed=23, dirichlet=(1, 4, 5)),
    "mixed-bc-3d": lambda: synthetic_inputs(20, 18, 10, 1, seed=5, dirichlet=(1, 4, 5)),      # tests/test_gpu_parity.py::test_schur_apply_mixed_bc
    "mixed-bc-2d": lambda: synthetic_inputs(24, 12, 1, 1, seed=6, dirichlet=(2, 3)),
    "nonuniform": lambda: synthetic_inputs(33, 17, 21, 2, seed=33 + 7 * 17 + 13 * 21),
    "f6-A": lambda: f6_block_inputs(*F6_SHAPES["A"]),
    "f6-B": lambda: f6_block_inputs(*F6_SHAPES["B"]),
    "f6-C": lambda: f6_block_inputs(*F6_SHAPES["C"]),
    "iaea3d": lambda: load_inputs("iaea3d"),
}
TWIN = ["1d", "2d", "2d-mixed", "3d", "3d-mixed"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs, input vectors, oracle outputs and the exact (y, s) per group -- computed once"""
    inp = CASES[name]()
    o = make_oracle(inp)
    ng = int(inp["ng"])
    xs = [input_vector(o.n_phi, g) for g in range(ng)]
    yo = [o.schur_apply(g, x).copy() for g, x in enumerate(xs)]
    ex = [ExactApply(inp, g).apply(x) for g, x in enumerate(xs)]
    return dict(inp=inp, x=xs, yo=yo, ex=ex, ng=ng)


def test_longdouble_is_extended():
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("name", list(CASES))
def test_exact_apply_agrees_with_the_oracle(name):
    c = _case(name)
    for g in range(c["ng"]):
        y, s = c["ex"][g]
        r = rho(c["yo"][g], y, s)
        print(f"{name} g={g}: oracle rho = {r:.2e} = {r / EPS:.1f} x 2^-53 (bar 64), normwise {normwise(c['yo'][g], y.astype(np.float64)):.2e}")
        assert np.isfinite(np.asarray(y, dtype=np.float64)).all() and (s > 0).all()
        assert r <= BAR, (name, g, r)


@pytest.mark.parametrize("name", TWIN)
def test_exact_apply_agrees_with_the_scipy_twin(name):
    from subcrit_exact import ref_from_inputs
    c = _case(name)
    r = ref_from_inputs(c["inp"])
    for g in range(c["ng"]):
        y, s = c["ex"][g]
        e = rho(r.schur_apply(g, np.asarray(c["x"][g])), y, s)
        print(f"{name} g={g}: twin rho = {e:.2e} = {e / EPS:.1f} x 2^-53 (bar 64)")
        assert e <= BAR, (name, g, e)


def test_scale_bounds_the_result():
    """|C_i x_i| <= s_i and |y_i| <= s_i (the triangle inequality)"""
    c = _case("f6-A")
    for g in range(c["ng"]):
        y, s = c["ex"][g]
        assert (np.abs(y) <= s * (1 + LD(2) ** -60)).all()
        cx = np.abs(np.asarray(c["inp"]["SigR"][g]).ravel().astype(LD) * LD(1.25) ** 3 * np.asarray(c["x"][g]).astype(LD))
        assert (cx <= s * (1 + LD(2) ** -60)).all()


def _pick(inp, g, y, s):
    """three cells that are not filler: at a line end (the first or last cell of its x, y or z line), at a block seam (its upper x
    neighbour is another material) and in the interior (the six neighbours are its own material) -- the first of each kind, in cell order, with |y_i| >= 0.2 s_i"""
    D = np.asarray(inp["D"])[g]
    nz, ny, nx = D.shape
    ok = (~f6_mask(inp, g).reshape(D.shape)) & (np.abs(y) >= LD(0.2) * s).reshape(D.shape)
    end = ok.copy(); end[1:-1, 1:-1, 1:-1] = False
    seam = ok.copy(); seam[:, :, -1] = False; seam[:, :, :-1] &= D[:, :, :-1] != D[:, :, 1:]; seam[:, :, 0] = False
    same = np.ones(D.shape, bool)
    for ax in range(3):
        a = np.moveaxis(D, ax, 0); m = np.moveaxis(same, ax, 0)
        m[0] = False; m[-1] = False
        m[1:-1] &= (a[1:-1] == a[:-2]) & (a[1:-1] == a[2:])
    inner = ok & same
    out = {}
    for kind, m in (("line end", end), ("block seam", seam), ("interior", inner)):
        idx = np.flatnonzero(m.ravel())
        assert idx.size, kind
        out[kind] = int(idx[0])
    return out


@pytest.mark.parametrize("name", ["f6-A", "f6-B", "f6-C", "iaea3d"])
def test_metric_sees_what_the_normwise_bar_cannot(name):
    c = _case(name)
    for g in range(c["ng"]):
        y, s = c["ex"][g]
        yo = c["yo"][g]
        below = float((np.abs(yo) < 1e-12 * np.abs(yo).max()).mean())
        print(f"{name} g={g}: {100 * below:.0f} % of the cells below 1e-12 max|y|, filler {100 * f6_mask(c['inp'], g).mean():.0f} %")
        assert below > 0.6
        for kind, i in _pick(c["inp"], g, y, s).items():
            bad = yo.copy(); bad[i] *= 1.0 + 1e-9
            new, old = rho(bad, y, s), normwise(bad, yo)
            print(f"  {kind}: cell {i}, |y_i| = {abs(yo[i]):.3e}: rho {new:.2e} (clean {rho(yo, y, s):.1e}), normwise {old:.2e}")
            assert new > 1e-10 and old < 1e-12, (name, g, kind, new, old)


def test_f6_block_inputs_are_what_they_say():
    for shape, block in list(F6_SHAPES.values()) + [((20, 18), (4, 3)), ((21, 20), (3, 4))]:
        inp = f6_block_inputs(shape, block)
        f6 = f6_mask(inp).reshape(shape[::-1])
        assert 0.2 < f6.mean() < 0.4, f6.mean()
        assert np.array_equal(f6, f6_mask(inp, 1).reshape(f6.shape))
        for k in ("x_breaks", "y_breaks", "z_breaks"):
            assert np.array_equal(np.diff(inp[k]), np.full(len(inp[k]) - 1, 1.25))
        if len(shape) == 2:                                        # the 2D form: (ng, ny, nx), no z breaks, the four attributes of a 2D mesh
            assert inp["D"].shape == (2,) + shape[::-1] and inp["SigS"].shape == (2, 2) + shape[::-1] and np.array_equal(inp["z_breaks"], [0.0])
            assert list(inp["bc_attr"]) == [1, 2, 3, 4] and not inp["bc_type"].any() and len(inp["x_breaks"]) == shape[0] + 1 and len(inp["y_breaks"]) == shape[1] + 1
            shape, block = shape + (1,), block + (1,)
        else:
            assert list(inp["bc_attr"]) == [1, 2, 3, 4, 5, 6] and not inp["bc_type"].any()
        assert (inp["D"][:, f6] == 1e-3).all() and (inp["SigR"][:, f6] == 1e15).all()
        assert not inp["NSF"][:, f6].any() and not inp["Chi"][:, f6].any() and not inp["SigS"][:, :, f6].any()
        assert (inp["SigR"][:, ~f6] >= 0.01).all() and (inp["SigR"][:, ~f6] <= 0.13).all()
        # piecewise constant on the blocks
        bx, by, bz = block
        D = inp["D"][0].reshape(shape[::-1])
        for iz in range(0, shape[2], bz):
            for iy in range(0, shape[1], by):
                for ix in range(0, shape[0], bx):
                    blk = D[iz:iz + bz, iy:iy + by, ix:ix + bx]
                    assert (blk == blk.flat[0]).all()


def test_two_step_cg_reference():
    """exact_cg2: x2 = c b - a0 a1 S b is two steps of the oracle's own CG; per component the oracle sits at a few 1e-13 of |x2|, with |x2|
    running over eighteen decades"""
    c = _case("f6-A")
    inp = c["inp"]
    o = make_oracle(inp)
    o.set_tol(1e-5, 0.0, 0.0, 200, 2)
    for g in range(c["ng"]):
        b = np.abs(np.asarray(c["x"][g])) * ~f6_mask(inp, g)
        x2, sc = exact_cg2(inp, g, b)
        xo, _, its = o.solve_group(g, b, with_J=False)
        assert its == 2
        r = rho(xo, x2, sc)
        rel = float((np.abs(xo.astype(LD) - x2) / np.abs(x2)).max())
        print(f"two CG steps g={g}: oracle rho = {r:.2e} = {r / EPS:.1f} x 2^-53, per component against |x2| {rel:.2e}, |x2| from {float(np.abs(x2).min()):.1e} to {float(np.abs(x2).max()):.1e}")
        f6 = f6_mask(inp, g)
        assert not b[f6].any() and float(np.abs(x2[f6]).max()) < 1e-9 * float(np.abs(x2).max())   # a normwise check of x2 sees the fuel only
        # alpha_1 = |r1|^2 / p1.S p1 is dominated by the filler cells (C = 2e15 against p1 = -a0 (S b)_i there), so it inherits the relative
        # error of (S b)_i in cells where the face terms cancel to a thousandth of their size: 1e-13, not 1e-16.  Measured: rho 4.7e-14 and
        # 3.5e-13, 2.9e-12 and 3.8e-13 of |x2| per component; the bar is a few times that -- this pins the reference, the GPU bar is in tests/test_gpu_apply_exact.py
        assert r <= 1e-11 and rel <= 1e-11


# ---- higher orders: the twin's operator with exact tables ---------------------------------------------------------------------------
def test_extended_gauss_rule():
    for n in (3, 5, 7):
        x, w = gauss_legendre_ld(n)
        for k in range(0, 2 * n, 2):                               # exact for every degree below 2 n: int x^k = 2 / (k + 1)
            assert abs((w * x ** k).sum() - LD(2) / (k + 1)) <= LD(2) ** -60, (n, k)
        assert abs((w * x ** (2 * n - 1)).sum()) <= LD(2) ** -60


@pytest.mark.parametrize("name", ["1d", "2d-mixed", "3d", "3d-mixed"])
def test_exact_twin_agrees_with_the_closed_forms(name):
    """RT0-P0: the two extended-precision references -- closed-form tridiagonals with a Thomas sweep, and the twin's matrices with exact
    tables under iterative refinement -- have nothing in common but the input dict.  The refinement stops at 1e-19 of max |u|, normwise, so
    per component they agree to a fraction of 2^-53 of the scale (measured 0.2 ... 0.6); the bar is 2^-51, far below what rests on either"""
    from subcrit_exact import ref_from_inputs
    c = _case(name)
    ex = ExactTwin(ref_from_inputs(c["inp"]))
    for g in range(c["ng"]):
        y, s = c["ex"][g]
        y2, s2, du = ex.apply(g, c["x"][g])
        r = rho(y2, y, s)
        print(f"{name} g={g}: exact twin against the closed forms rho = {r:.2e} = {r / EPS:.2f} x 2^-53, last correction {du:.1e}")
        assert du <= 1e-18 and r <= 4 * EPS
        assert (np.abs(s2 - s) <= 1e-15 * s).all()


@pytest.mark.parametrize("rt,shape,block", [(2, (6, 4, 3), (3, 2, 3)), (1, (9, 4, 4), (3, 2, 2))])
def test_oracle_and_twin_share_the_tabulated_gauss_rule(rt, shape, block):
    """RT1-P1 / RT2-P2 at the filler's contrast: oracle and twin against the operator with exact local tables.  Both keep the reference's
    15-digit Gauss table, whose weights are off by up to 1e-15 relative, so each sits at 40 ... 200 x 2^-53 of the scale (measured) -- a
    property of the reference, kept on purpose.  For RT2 the distance between the two (47 ... 80) is well below the distance of either
    from the operator: oracle-versus-twin does not measure the oracle's error.  Bar: 2^-40 of the scale, a sanity bound on both"""
    from subcrit_exact import ref_from_inputs
    inp = f6_block_inputs(shape, block)
    o, r = make_oracle(inp, rt, rt), ref_from_inputs(inp, rt, rt)
    ex = ExactTwin(r)
    for g in range(2):
        x = input_vector(o.n_phi, g)
        y, s, du = ex.apply(g, x)
        yo, yt = o.schur_apply(g, x), r.schur_apply(g, np.asarray(x))
        ro, rt_, rot = rho(yo, y, s), rho(yt, y, s), rho(yo, yt.astype(LD), s)
        print(f"RT{rt} {shape} g={g}: x 2^-53: oracle {ro / EPS:.1f}, twin {rt_ / EPS:.1f}, oracle vs twin {rot / EPS:.1f}; last correction {du:.1e}")
        assert du <= 1e-18 and max(ro, rt_) <= 2.0 ** -40
        if rt == 2:
            assert rot < min(ro, rt_)


# ---- two CG steps and one outer iteration on the twin: the references of tests/test_gpu_orders_exact.py ------------------------------
@pytest.mark.parametrize("name", ["1d", "2d-mixed", "3d", "3d-mixed"])
def test_two_cg_steps_on_the_twin_agree_with_the_closed_forms(name):
    """RT0-P0: exact_cg2_op on ExactTwin against exact_cg2 (the closed forms), b = |input vector| -- the bar of
    test_exact_twin_agrees_with_the_closed_forms, per component of the two-step scale"""
    from subcrit_exact import ref_from_inputs
    c = _case(name)
    ex = ExactTwin(ref_from_inputs(c["inp"]))
    for g in range(c["ng"]):
        b = np.abs(np.asarray(c["x"][g]))
        x2, sc = exact_cg2(c["inp"], g, b)
        dus = []
        x2t, sct = exact_cg2_op(ex.operator(g, dus), b)
        r = rho(x2t, x2, sc)
        print(f"{name} g={g}: two CG steps, twin against the closed forms rho = {r:.2e} = {r / EPS:.2f} x 2^-53, last corrections {max(dus):.1e}")
        assert len(dus) == 2 and max(dus) <= 1e-18 and r <= 4 * EPS
        assert (np.abs(sct - sc) <= 1e-15 * sc).all()


def test_one_outer_on_the_twin_agrees_with_the_closed_forms():
    """RT0-P0 at the filler's contrast (shape R of tests/test_gpu_apply_exact.py): ExactTwin.outer -- right-hand sides from the twin's
    diagonals -- against the same outer written with cell volumes and the closed-form apply"""
    from subcrit_exact import ref_from_inputs
    inp = f6_block_inputs((12, 11, 10), (4, 4, 5))
    cells = inp["D"][0].size
    out = ExactTwin(ref_from_inputs(inp)).outer()
    V = np.full(cells, LD(1.25) ** 3)
    F = (inp["NSF"].reshape(2, cells).astype(LD) * V).sum(axis=0)
    b0 = inp["Chi"].reshape(2, cells)[0].astype(LD) * F
    y0, s0 = exact_cg2(inp, 0, b0)
    b1 = inp["Chi"].reshape(2, cells)[1].astype(LD) * F + inp["SigS"].reshape(2, 2, cells)[1, 0].astype(LD) * V * y0
    y1, s1 = exact_cg2(inp, 1, b1)
    assert len(out["du"]) == 4 and max(out["du"]) <= 1e-18
    # b0 is the same arithmetic on either side; b1 carries the distance of the two y0 through the scattering block
    slack = (LD(2) ** -60 * np.abs(b0), LD(2) ** -60 * np.abs(b1) + 4 * EPS * inp["SigS"].reshape(2, 2, cells)[1, 0].astype(LD) * V * s0)
    for g, (b, y, s) in enumerate(((b0, y0, s0), (b1, y1, s1))):
        r = rho(out["y"][g], y, s)
        print(f"one outer g={g}: twin against the closed forms rho = {r:.2e} = {r / EPS:.2f} x 2^-53")
        assert (np.abs(out["b"][g] - b) <= slack[g]).all() and r <= 4 * EPS


def _lane_plans():
    """lane_plan (neutfem_amd/csrc/nf_resident_lanes.h) of every case, two-sided and one-sided, at the 160 KiB of LDS the library plans
    with (resident_lds_cap: bytes / 8 - 32 doubles)"""
    import os, shutil, subprocess, tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    args = []
    for rt, p, shape, _ in ORDER_CASES.values():
        dim = len(shape)
        args += [dim, *shape, *([1] * (3 - dim)), min(rt, p), (p + 1) ** dim, (p + 1) ** (dim - 1)]   # NB, moments per cell, transverse modes: as nf_create counts them
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "resident_lanes_cases")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(here, "host", "resident_lanes_cases_main.cpp")])
        lines = subprocess.run([exe, str(160 * 1024 // 8 - 32)] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split("\n")
    keys = ("fits", "tw0", "tw1", "tw2", "slots", "PC", "NPp", "need")
    rows = [dict(zip(keys, map(int, l.split()))) for l in lines if l]
    assert len(rows) == 2 * len(ORDER_CASES)
    return {name: (rows[2 * i], rows[2 * i + 1]) for i, name in enumerate(ORDER_CASES)}


def test_order_cases_cover_what_they_are_for():
    """by lane_plan's arithmetic every case fits a line-per-lane variant, two-sided and one-sided -- the bubble variant where the flux has
    bubble moments (NB = min(RT, P) > 0), the RT0-P0 one at its smaller pitch for the P0 cases; the set covers RT1 and RT2 in 2D and 3D with
    P = RT and P < RT, both parities of nx at NB = 1 and at NB = 2 (the scan variants' VEC), RT2-P0, and lines shorter than 4 cells in some
    directions beside two-sided ones"""
    plans = _lane_plans()
    for name, (two, one) in plans.items():
        rt, p, shape, _ = ORDER_CASES[name]
        print(name, ORDER_CASES[name], two, one)
        assert two["fits"] == 1 and one["fits"] == 1 and one["tw0"] + one["tw1"] + one["tw2"] == 0, (name, two, one)
        assert [two["tw0"], two["tw1"], two["tw2"]] == [int(n >= 4) for n in shape] + [0] * (3 - len(shape)), (name, two)
        if min(rt, p) > 0: assert 0 < two["NPp"] <= 5120 and (p + 1) ** (len(shape) - 1) <= 9 and (p + 1) ** len(shape) <= 27
        else: assert two["PC"] == 0 and (shape[0] | 1) * int(np.prod(shape[1:])) <= 1536      # nf_batch_result::variant 1
    have = {(rt, len(shape), p == rt) for rt, p, shape, _ in ORDER_CASES.values()}
    assert {(1, 2, True), (2, 2, True), (1, 3, True), (2, 3, True)} <= have and {rt for rt, _, eq in have if not eq} == {1, 2}
    assert {(min(rt, p), shape[0] % 2) for rt, p, shape, _ in ORDER_CASES.values()} >= {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert {(2, 0), (2, 1), (1, 0)} <= {(rt, p) for rt, p, _, _ in ORDER_CASES.values()}
    two = plans["h"][0]
    assert (two["tw0"], two["tw1"], two["tw2"]) == (1, 0, 0)


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_order_cases_meet_their_conditions(name):
    """what tests/test_gpu_orders_exact.py asserts of its references, with the oracle alone: the refinement has converged on every
    reference apply, the oracle takes exactly 2 CG steps, the filler covers 20 - 40 % of the cells, b vanishes on every filler DOF and is
    positive somewhere in each group -- for the two CG steps and for the one outer from either start flux.  Prints the bars' base: the
    double oracle's own rho x 2^53"""
    c = order_case(name)
    rt, p, shape, _ = ORDER_CASES[name]
    cg, ou, rough = order_ref_cg(name), order_ref_outer(name), order_ref_outer(name, "rough")
    fill = float(f6_mask(c["inp"]).mean())
    print(f"{name} RT{rt}-P{p} {shape}: {c['ex'].r.nPhi} unknowns per group, filler {100 * fill:.0f} %, oracle rho x 2^53: two CG steps "
          f"{cg['rho_o'][0] / EPS:.0f} / {cg['rho_o'][1] / EPS:.0f}, one outer {ou['rho_o'][0] / EPS:.0f} / {ou['rho_o'][1] / EPS:.0f}, "
          f"from the rough start {rough['rho_o'][0] / EPS:.0f} / {rough['rho_o'][1] / EPS:.0f}; last corrections up to {max(cg['du'] + ou['du'] + rough['du']):.1e}")
    assert 0.2 <= fill <= 0.4 and c["filler"].size == c["ex"].r.nPhi and c["filler"].sum() == c["nloc"] * f6_mask(c["inp"]).sum()
    phi0 = order_start_flux(name, "rough")
    assert order_start_flux(name, "flat") is None and phi0.shape == (2, c["ex"].r.nPhi) and phi0.min() >= 0.5 and phi0.max() <= 1.5
    for ref in (cg, ou, rough):
        assert len(ref["du"]) == 4 and max(ref["du"]) <= 1e-18
    for o_ in (ou, rough):
        assert o_["n_outer_o"] == 1 and (o_["cg_o"] == 2).all()
    for g in (0, 1):
        assert cg["its_o"][g] == 2
        for b in (cg["x"][g], ou["b"][g], rough["b"][g]):
            b = np.asarray(b)
            assert not b[c["filler"]].any() and b.max() > 0, (name, g)
        for r in (cg["rho_o"][g], ou["rho_o"][g], rough["rho_o"][g]):
            assert 0 < r <= 2.0 ** -36, (name, g, r / EPS)            # a sanity bound on the oracle (its largest, RT2-P1: 6069 x 2^-53)


# ---- the reconstructed currents J = -A^-1 B^T phi: the references of tests/test_gpu_currents_exact.py -----------------------------------
CURRENT_CASES = [("p0", n) for n in P0_CASES] + [("higher", n) for n in ORDER_CASES]
ZERO_SCALE = {"e": (1478, 2956), "f": (11390, 20502), "i": (18224, 20502)}      # P < RT: the RT modes that see no flux moment, of all current DOFs


def test_the_two_current_references_agree():
    """RT0-P0 on shape R: ExactApply.currents (closed-form tridiagonals, Thomas, M(A)^-1 for the scale) and ExactTwin.currents (the twin's
    triplets, iterative refinement, dense block inverses) are two restatements with nothing in common but the input dict.  On what they are
    used on -- a solver's returned flux, here the oracle's after one outer iteration from the rough start -- they agree to 1e-17 of the
    scale per component (measured 7.5e-18 and 7.3e-18: a fifteenth of 2^-53); the two scales are the same bound computed twice, one of
    them in double.  On the signed input vector of the apply tests (10 % of its entries x 1e-12) the distance is 1.10e-17 / 1.11e-17, the
    same with more refinement sweeps: it is the twin's local tables, summed from a 7-point rule, against the closed forms 2/3 and 1/3 --
    printed here, and the reason why the RT0-P0 tests judge with the closed forms"""
    from subcrit_exact import ref_from_inputs
    c = p0_case("R")
    ex = ExactTwin(ref_from_inputs(c["inp"], 0, 0))
    phi = currents_outer_oracle("p0", "R")["phi"]
    for g in (0, 1):
        x = input_vector(phi[g].size, g)
        print(f"R g={g}: on the signed input vector rho = {rho(ex.currents(g, x)[0], *c['ea'][g].currents(x)):.2e}")
        J, s = c["ea"][g].currents(phi[g])
        J2, s2, du = ex.currents(g, phi[g])
        r = rho(J2, J, s)
        print(f"R g={g}: the two references rho = {r:.2e}, last correction {du:.1e}, scales apart {float((np.abs(s2 - s) / s).max()):.1e}")
        assert J.shape == J2.shape == (ex.r.nJ,) and (s > 0).all()
        assert du <= 1e-18 and r <= 1e-17, (g, du, r)
        assert (np.abs(s2 - s) <= 1e-13 * s).all()
        assert (np.abs(J) <= s * (1 + LD(2) ** -60)).all()             # |u| = |A^-1 t| <= |A^-1| |t| <= s


@pytest.mark.parametrize("family,name", CURRENT_CASES)
def test_oracle_currents_per_component(family, name):
    """Fit-free: solve_group(g, b, with_J = True) with two CG steps returns phi and J of the same unnormalised field, so the oracle's J is
    judged against the reference applied to its own phi with no scalar in between -- which also pins the references' DOF order and sign.
    The cap of 64 x 2^-53 is a sanity bound on the yardstick (about 8 x the largest figure measured, 7.4): an oracle above it means the
    reference or its scale is broken.  Conditions: refinement du <= 1e-18, filler in 20 - 40 % of the cells, no zero-scale DOF at P = RT
    and exactly the modes without a flux moment at P < RT, where reference and oracle are exact zeros"""
    r = currents_cg_oracle(family, name)
    c = order_case(name) if family == "higher" else p0_case(name)
    fill = float(f6_mask(c["inp"]).mean())
    print(f"{family} {name}: oracle rho x 2^53 " + ", ".join(f"{k} {v[0] / EPS:.1f} / {v[1] / EPS:.1f}" for k, v in r["rho"].items()) + f"; filler {fill:.3f}")
    assert 0.2 <= fill <= 0.4
    for vs in r["rho"].values():
        for v in vs:
            assert np.isfinite(v) and v <= 64 * EPS, (family, name, r["rho"])
    if family == "higher":
        assert len(c["du_J"]) >= 2 and max(c["du_J"]) <= 1e-18, c["du_J"]
    for g, (J, s) in enumerate(r["ref"]):
        zero = s == 0
        want = ZERO_SCALE.get(name, (0, zero.size)) if family == "higher" else (0, zero.size)
        assert (int(zero.sum()), zero.size) == want, (name, g, int(zero.sum()), zero.size)
        assert not J[zero].any() and not r["J"][g][zero].any() and np.abs(J[~zero]).min() >= 0


@pytest.mark.parametrize("family,name", [(f, n) for f in CURRENT_FAMILIES for n in CURRENT_FAMILIES[f]])
def test_fitted_scalar_on_the_oracle(family, name):
    """The procedure of the GPU tests on the oracle: one outer iteration from the rough start, phi_dofs() and J_dofs(), one scalar fitted on
    the currents of group 0.  SolveKeff returns phi = raw / |raw| and builds J from raw; after ONE outer iteration no Chebyshev step has
    touched phi, so raw = c phi up to one rounding per entry, which moves the reference by at most 2^-53 s.  The fit adds at most
    kappa x the fit-free rho, kappa = sum s |J| / sum J^2 on group 0 (|dc / c| <= rho sum s |J| / sum J^2), hence the cap (64 (1 + kappa) + 1) x 2^-53 --
    a sanity bound again; the figures are 1 ... 14.  c agrees with the scalar of the flux against the exact outer to rounding (measured
    3e-15 at most); a wrong sign or global factor is O(1)"""
    r = currents_outer_oracle(family, name)
    worst = max(v for vs in r["rho"].values() for v in vs)
    print(f"{family} {name}: oracle rho x 2^53 " + ", ".join(f"{k} {v[0] / EPS:.1f} / {v[1] / EPS:.1f}" for k, v in r["rho"].items()) +
          f"; c c_flux - 1 = {float(r['c'] * r['c_flux'] - 1):.1e}, kappa {r['kappa']:.1f}")
    assert np.isfinite(worst) and worst <= (64 * (1 + r["kappa"]) + 1) * EPS, (family, name, worst / EPS)
    assert abs(float(r["c"] * r["c_flux"] - 1)) <= 1e-12
    if family == "higher":
        assert max(order_case(name)["du_J"]) <= 1e-18 and r["zero_scale"] == [ZERO_SCALE.get(name, (0, 0))[0]] * 2


def test_current_bars_are_pooled_over_their_family():
    for family in CURRENT_FAMILIES:
        bar, worst = currents_bar(family)
        print(f"{family}: the oracle's largest rho {worst / EPS:.1f} x 2^-53 over {CURRENT_FAMILIES[family]}, bar {bar / EPS:.1f}")
        assert bar == ORDER_BAR * max(worst, EPS) and EPS <= worst <= 64 * (1 + 64) * EPS


def test_exact_outer_p0_is_the_twins_outer():
    """the closed-form outer of the RT0-P0 cases against ExactTwin.outer from the same rough start (shape R)"""
    from subcrit_exact import ref_from_inputs
    c = p0_case("R")
    phi0 = rough_start(2, c["inp"]["D"][0].size)
    y = exact_outer_p0(c["inp"], phi0)
    out = ExactTwin(ref_from_inputs(c["inp"], 0, 0)).outer(phi0)
    for g in (0, 1):
        assert rho(out["y"][g], y[g], out["s"][g]) <= 4 * EPS


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_currents_metric_sees_what_the_normwise_bars_cannot(name):
    """the largest bubble current of the oracle's J times 1 + 1e-9 -- a wrong iM / eL / eR coefficient at that level: rel_l2 against the
    unperturbed J, the measure of every older current test (bars 1e-7 ... 1e-9), moves by 1e-10; rho goes from a few 2^-53 to 1e5 x 2^-53"""
    r = currents_cg_oracle("higher", name)
    bub = r["classes"]["bubbles"]
    for g, (Jr, s) in enumerate(r["ref"]):
        J = r["J"][g]
        i = bub[np.argmax(np.abs(J[bub]))]
        bad = J.copy(); bad[i] *= 1.0 + 1e-9
        new, clean, old = rho(bad[bub], Jr[bub], s[bub]), r["rho"]["bubbles"][g], rel_l2(bad, J)
        print(f"{name} g={g}: bubble DOF {i}: rho {clean / EPS:.1f} -> {new / EPS:.3g} x 2^-53, rel_l2 {old:.1e}")
        assert old < 1e-8 and new > 1e4 * EPS, (name, g, old, new / EPS)


def test_currents_metric_sees_a_misplaced_small_bubble(name="c"):
    """a bubble of one transverse mode stored in its neighbour's slot where both are small: the two bubble DOFs of neighbouring modes (slots
    l + k a and l + k (a + 1) of one cell and direction) with the smallest larger-of-the-two magnitude, swapped.  rel_l2 does not move
    (below 1e-8: on case c, whose filler blocks are 4 x 3 x 5 cells, they sit inside the filler at 1e-17 of the largest current -- asserted
    as a condition; on the synthetic inputs of the older tests no pair is small, and those tests do see a swap); rho says the DOFs are
    wrong by their own size"""
    r = currents_cg_oracle("higher", name)
    c = order_case(name)
    k, bub = c["rt"], r["classes"]["bubbles"]
    ni = k * (k + 1) ** (len(c["shape"]) - 1)
    for g, (Jr, s) in enumerate(r["ref"]):
        J = r["J"][g]
        slots = bub.reshape(-1, ni)[:, :ni - k]                      # every (cell, direction) block: slot and its neighbour in the next mode
        big = np.maximum(np.abs(J[slots]), np.abs(J[slots + k]))
        big[(J[slots] == J[slots + k])] = np.inf
        i = slots.ravel()[np.argmin(big)]
        assert big.min() <= 1e-10 * np.abs(J).max(), (name, g, big.min())
        bad = J.copy(); bad[i], bad[i + k] = J[i + k], J[i]
        new, old = rho(bad[bub], Jr[bub], s[bub]), rel_l2(bad, J)
        print(f"{name} g={g}: bubbles {i} and {i + k} ({J[i]:.2e}, {J[i + k]:.2e}) swapped: rho {new / EPS:.3g} x 2^-53, rel_l2 {old:.1e}")
        assert old < 1e-8 and new > 1e4 * EPS, (name, g, old, new / EPS)


def test_current_classes_partition_the_dofs():
    for dims, rt, cut in (((5, 4, 20), 2, (9,)), ((20, 18), 1, ()), ((12, 11, 10), 0, ())):
        classes, nJ = current_classes(dims, rt, cut)
        allidx = np.sort(np.concatenate(list(classes.values())))
        assert np.array_equal(allidx, np.arange(nJ))
        if cut: assert classes["z interface"].size == len(cut) * dims[0] * dims[1] * (rt + 1) ** 2
