"""The orders with bubble moments (NB = 1, 2) per component at the benchmark's contrast: the CG forms and every SolveKeff path against the
extended-precision twin (tests/apply_exact.py: ExactTwin, exact_cg2_op, ExactTwin.outer).

tests/test_gpu_apply_exact.py judges RT0-P0 this way through every launch variant; of the higher orders it reaches the plain apply at
P = RT only.  Here, on f6_block_inputs (IAEA-3D's filler, D = 1e-3, Sigma_R = 1e15, in 25 - 34 % of the cells; ng = 2, all-Dirichlet) at
the smallest shapes at which these kernels engage (apply_exact.ORDER_CASES: RT1-P1, RT2-P2, RT1-P0, RT2-P1, RT2-P0 in 2D and 3D, both
parities of nx at either NB, one case whose y and z lines are shorter than 4 cells):

  two CG steps   solve_group(g, b, 0, 2), b = |input vector| off the filler and 0 on every flux DOF of a filler cell, against exact_cg2_op on
                 the twin with the scale |c| |b| + a0 a1 s(b): the four-launch CG lean and not lean (fused p.q partials at NB > 0), k_apply3,
                 k_cg_xcd (SEG = 4 bubble tiles) -- each named by the plan before the solve and by nf_info "cg_form" after it
  one outer      set_tol(0, 0, 0, 1, 2), solve_keff() against ExactTwin.outer, one scalar fitted on group 0 -- from SolveKeff's own flat
                 start flux and from a rough one (apply_exact.order_start_flux: after the flat start the right-hand sides are equal in
                 moments of equal mass, and an apply that confuses two of them shows only in the scalar a1 of the second CG step): the
                 host-driven loop (k_group_rhs's P >= 1 form), k_keff_xcd, the resident line-per-lane variants two-sided and one-sided
                 (k_resident_keff<false, 1|2, -1>: nf_batch_result::variant 3, 4), the resident scans with and without LDS
                 (k_resident_keff<VEC, 1|2, 0>: variants 7 - 10).  The instantiation is named by solve_keff_batch on a twin handle with n = 1,
                 which must also leave the same bits.

Metric: rho of tests/apply_exact.py, per component.  Bar: ORDER_BAR = 4 times the double oracle's own rho on the same case, group and
quantity (its solve_group with two iterations, or its one-outer SolveKeff under the same scalar fit), computed here on the CPU -- the margin
test_higher_orders grants; the oracle runs the same algorithm in double and differs in summation order and in its band LDL^T.  The bar is
never derived from the GPU's numbers.  Conditions (asserted, also without a GPU in tests/test_apply_exact.py): refinement du <= 1e-18 on
every reference apply, the oracle takes exactly 2 CG steps, the filler covers 20 - 40 % of the cells, b vanishes on every filler DOF and
is positive somewhere in each group.

Measured on an MI355X, rho x 2^53 as g0 / g1 (oracle: the bar is 4 x that); no figure is above its oracle's:

  two CG steps        unknowns   oracle      four-launch lean   four-launch   k_apply3   k_cg_xcd
  a RT1-P1 20x18      1440       319/293     75/64              75/64         75/65      76/64
  b RT2-P2 21x20      3780       478/452     99/90              99/90         98/90      98/93
  c RT1-P1 8x6x5      1920       303/570     20/49              20/49         20/50      20/49
  d RT2-P2 5x5x4      2700       763/267     78/31              78/31         78/31      78/32
  e RT1-P0 20x18      360        110/105     4/5                4/5           4/10       6/8
  f RT2-P1 8x6x5      1920       6069/2046   131/77             131/77        127/77     131/77
  g RT2-P2 4x5x5      2700       518/610     82/20              82/20         82/19      81/20
  h RT1-P1 9x3x2      432        152/133     5/7                5/7           5/5        6/4
  i RT2-P0 8x6x5      240        1278/695    22/7               22/7          20/6       20/7
  one outer           variants   oracle      host loop   k_keff_xcd   lanes   lanes one-sided   scans   scans no LDS
  a RT1-P1 20x18      3, 8       359/363     55/44       56/50        55/34   56/36             54/50   54/50
  b RT2-P2 21x20      4, 9       106/261     11/16       11/17        13/12   13/12             13/18   13/18
  c RT1-P1 8x6x5      3, 8       262/162     17/22       13/18        15/18   15/18             13/16   13/16
  d RT2-P2 5x5x4      4, 9       189/315     65/64       65/64        63/63   63/64             64/63   64/63
  e RT1-P0 20x18      1, 6       54/47       6/6         6/6          7/6     7/7               4/7     4/7
  f RT2-P1 8x6x5      3, 8       259/368     8/15        7/11         7/8     6/8               6/12    6/12
  g RT2-P2 4x5x5      4, 10      204/181     62/62       62/66        60/62   62/64             66/66   66/66
  h RT1-P1 9x3x2      3, 7       204/192     13/7        8/7          9/13    8/13              13/10   13/10
  i RT2-P0 8x6x5      1, 6       309/269     5/9         6/11         6/9     6/10              9/10    9/10
  one outer, rough start         oracle      host loop   k_keff_xcd   lanes   lanes one-sided   scans   scans no LDS
  a RT1-P1 20x18                 280/444     19/36       18/44        22/53   18/52             21/44   21/44
  b RT2-P2 21x20                 373/272     38/62       38/61        58/24   27/61             38/60   38/60
  c RT1-P1 8x6x5                 276/282     10/12       11/10        14/13   12/16             12/12   12/12
  d RT2-P2 5x5x4                 158/210     80/80       82/79        78/71   75/73             79/78   79/78
  e RT1-P0 20x18                 64/63       6/7         6/7          4/4     4/4               6/7     6/7
  f RT2-P1 8x6x5                 323/318     11/13       9/15         8/16    13/12             8/12    8/12
  g RT2-P2 4x5x5                 191/178     84/89       85/87        91/90   91/92             86/84   86/84
  h RT1-P1 9x3x2                 208/208     9/9         9/8          9/6     8/6               10/7    10/7
  i RT2-P0 8x6x5                 301/295     8/10        8/10         9/6     9/6               8/8     8/8
  The largest gpu / oracle ratio: 0.24 (two CG steps), 0.37 (one outer), 0.52 (rough start; g, lanes one-sided).
  (variants: nf_batch_result::variant of the lanes, of the scans.)  RT0-P0, shape W of tests/test_gpu_apply_exact.py, k_keff_xcd: 5.3 / 6.5,
  oracle 39 / 491.

Sensitivity, tried on a scratch build and not kept.  (A) The bubble diagonal factor diagc of resident_choose times 1 + 1e-10 at P = RT:
the lanes and one-sided lanes of a, b, c, d, g and h fail from either start (rho 1.4e5 ... 2.8e5 x 2^-53 against bars of 424 ... 1492),
everything else here passes, and so do tests/test_gpu_orders.py, tests/test_gpu_batch.py and tests/test_gpu_paths.py.  (B) mom[2][1][1] and
mom[2][2][1] swapped at P < RT in 3D: f's lanes pass from the flat start at 8.3 / 8.1, the figures of the correct build, and fail from the
rough one at 6.7e11 / 4.7e11 -- which is why the rough start is here; tests/test_gpu_paths.py notices it in its converged RT2-P1 solve.
"""
import numpy as np
import pytest

from apply_exact import EPS, ORDER_BAR, ORDER_CASES, f6_mask, order_case, order_ref_cg, order_ref_outer, order_start_flux, outer_rho, rho
from helpers import CG_FORMS, make_hip

pytestmark = pytest.mark.gpu


def _set(s, opts):
    for k, v in opts.items():
        s.set_option(k, v)


def _conditions(name, cg=None, ou=None):
    c = order_case(name)
    fill = float(f6_mask(c["inp"]).mean())
    assert 0.2 <= fill <= 0.4, (name, fill)
    for ref, bs in ((cg, cg and [cg["x"][g] for g in (0, 1)]), (ou, ou and ou["b"])):
        if ref is None: continue
        assert len(ref["du"]) == 4 and max(ref["du"]) <= 1e-18, (name, ref["du"])      # two reference applies per group, all converged
        for g, b in enumerate(bs):
            b = np.asarray(b)
            assert not b[c["filler"]].any() and b.max() > 0, (name, g)
    if cg is not None: assert all(cg["its_o"][g] == 2 for g in (0, 1)), cg["its_o"]
    if ou is not None: assert ou["n_outer_o"] == 1 and (ou["cg_o"] == 2).all(), (ou["n_outer_o"], ou["cg_o"])
    return c


def _judge(kind, name, label, rhos, rhos_o):
    """prints every group's figure, then asserts the bar"""
    rt, p, shape, _ = ORDER_CASES[name]
    for g, (r, ro) in enumerate(zip(rhos, rhos_o)):
        print(f"RHO {kind} {name} RT{rt}-P{p} {'x'.join(map(str, shape))} {label} g={g}: gpu {r / EPS:.1f} x 2^-53, oracle {ro / EPS:.1f} (bar {ORDER_BAR} x oracle = {ORDER_BAR * ro / EPS:.0f}), gpu / oracle {r / ro:.2f}")
    for g, (r, ro) in enumerate(zip(rhos, rhos_o)):
        assert r <= ORDER_BAR * ro, (kind, name, label, g, r / EPS, ro / EPS)


# ---- two CG steps ----------------------------------------------------------------------------------------------------------------
LAUNCHES = dict(resident=0, cg_fuse3=0, cg_xcd=0)
CG = {"four-launch lean": (dict(LAUNCHES, cg_lean=1), "lean"), "four-launch": (dict(LAUNCHES, cg_lean=0), "fused"),
      "k_apply3": (dict(resident=0, cg_fuse3=1, cg_xcd=0), "fuse3"), "k_cg_xcd": (dict(resident=0, cg_fuse3=1, cg_xcd=1, cg_xcd_min_cells=0), "xcd")}


def _solves(s, ref, name, label):
    out = []
    for g in ref["groups"]:
        x, its, _ = s.solve_group(g, ref["x"][g], 0.0, 2)
        assert its == 2 and np.isfinite(x).all(), (name, label, g, its)
        out.append(x)
    _judge("cg2", name, label, [rho(x, ref["y"][g], ref["s"][g]) for g, x in enumerate(out)], [ref["rho_o"][g] for g in ref["groups"]])
    return out


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_cg_forms(name):
    """every case is inside what xcd_eligible takes once cg_xcd_min_cells is out of the way (SEG = 4 tiles, at most 9 modes, x lines of at
    most 128 cells, under 28 000 unknowns): the plan must say "xcd", no case is left to another form"""
    ref = order_ref_cg(name)
    c = _conditions(name, cg=ref)
    got = {}
    for label, (opts, form) in CG.items():
        s = make_hip(c["inp"], c["rt"], c["p"]); _set(s, opts)
        assert s.info("rt_order") == c["rt"] and s.info("p_order") == c["p"] and s.n_loc == c["nloc"] and s.n_phi == ref["x"][0].size
        plan = s.apply_plan(True)
        assert plan["in_cg"] == 1 and plan["form"] == form and plan["fused"] == 1 and plan["lean"] == int(form != "fused"), (label, plan)
        assert all(plan[d]["family"] == ("x" if d == "x" else "s") for d in "xyz"[:s.info("dim")]), plan["passes"]
        got[label] = _solves(s, ref, name, label)
        assert CG_FORMS[s.info("cg_form")] == form and s.info("last_xcd") == int(form == "xcd") and s.info("xcd_refused") == 0, (label, CG_FORMS[s.info("cg_form")])
        if form == "xcd": assert s.info("xcd_solves") == len(ref["groups"])
        s.close()
    # k_apply3 sums p.q in another order than the four-launch CG: that it ran shows in the bits
    assert any(not np.array_equal(u, v) for u, v in zip(got["k_apply3"], got["four-launch lean"])), name


# ---- one outer iteration ---------------------------------------------------------------------------------------------------------
RES = dict(resident=1, resident_max_dofs=100000)
# options, last_path, last_resident_serial, nf_batch_result::variant as a function of (NB, nx) -- NB = min(RT, P), the bubble moments the flux
# carries; the P0 cases take the RT0-P0 instantiations (1: lanes at pitch 1536, 5 / 6: scans) with their own line factors.  None = not a resident path
OUTER = {
    "host loop": (dict(resident=0, keff_xcd=0), 0, None, None),
    "k_keff_xcd": (dict(resident=0, keff_xcd=1, cg_xcd=1, cg_xcd_min_cells=0), 3, None, None),
    "lanes": (dict(resident=1), 2, 1, lambda nb, nx: 2 + nb if nb else 1),
    "lanes one-sided": (dict(resident=1, resident_two_sided=0), 2, 1, lambda nb, nx: 2 + nb if nb else 1),
    "scans": (dict(RES, resident_serial=0), 2, 0, lambda nb, nx: 5 + 2 * nb + (nx % 2 == 0)),
    "scans no LDS": (dict(RES, resident_lds=0), 2, 0, lambda nb, nx: 5 + 2 * nb + (nx % 2 == 0)),
}
REACHED = {}                                                      # variant -> cases, filled as the tests run (printed for the record)


def _outer_solver(c, opts, phi0):
    s = make_hip(c["inp"], c["rt"], c["p"]); _set(s, opts); s.set_tol(0.0, 0.0, 0.0, 1, 2)
    if phi0 is not None: s.set_phi(phi0)
    return s


@pytest.mark.parametrize("start", ["flat", "rough"])
@pytest.mark.parametrize("label", list(OUTER))
@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_one_outer(name, label, start):
    """start = "rough" is what a wrong moment index needs to show per component (apply_exact.order_start_flux): found with two entries of
    ResidentArgs::mom swapped at RT2-P1, which the flat start let pass"""
    from neutfem_amd import capi
    ref, phi0 = order_ref_outer(name, start), order_start_flux(name, start)
    c = _conditions(name, ou=ref)
    opts, path, serial, variant = OUTER[label]
    s = _outer_solver(c, opts, phi0)
    k, n = s.solve_keff()
    assert n == 1 and s.info("last_path") == path and (s.history()["cg"] == 2).all(), (name, label, n, s.info("last_path"), s.history()["cg"])
    if path == 3: assert s.info("xcd_refused") == 0
    phi = s.get_phi()
    assert np.isfinite(phi).all() and np.isfinite(k)
    if variant is not None:
        assert s.info("last_resident_serial") == serial, (name, label)
        # the instantiation: nf_solve_keff_batch of one twin handle names it and leaves the bits of the single call
        want = int(variant(min(c["rt"], c["p"]), c["shape"][0]))
        t = _outer_solver(c, opts, phi0)
        kb, nb_, st, res = capi.solve_keff_batch([t])
        assert list(st) == [0] and res == dict(n_batched=1, n_sequential=0, n_launches=1, variant=want), (name, label, st, res)
        assert kb[0] == k and nb_[0] == 1 and np.array_equal(t.get_phi(), phi) and t.info("last_resident_serial") == serial
        t.close()
        REACHED.setdefault(want, []).append(name)
        print(f"\nVARIANT {want} {name} {label}; reached so far: {sorted(REACHED)}")
    print(f"\nPATH {path} {name} {label}")
    _judge("outer" if start == "flat" else "outer-rough", name, label, outer_rho(phi, ref), ref["rho_o"])
    s.close()


def test_every_bubble_instantiation_has_a_case():
    """by the selection arithmetic of resident_choose (NB > 0: the lanes take 2 + NB, the scans 5 + 2 NB + (nx even)) the case table reaches
    variants 3, 4 and 7 - 10; test_one_outer asserts through nf_batch_result::variant that each case ran the one named here"""
    lanes = {int(OUTER["lanes"][3](min(rt, p), shape[0])) for rt, p, shape, _ in ORDER_CASES.values()}
    scans = {int(OUTER["scans"][3](min(rt, p), shape[0])) for rt, p, shape, _ in ORDER_CASES.values()}
    assert lanes >= {3, 4} and scans >= {7, 8, 9, 10}, (lanes, scans)
