"""The form of the CG iteration is chosen in one place (cg_plan in neutfem_amd/csrc/neutfem_hip.hip): the read-only report names it before
the solve (apply_plan(True)["form"]), the solve runs it and names it afterwards (nf_info "cg_form"), and the two must agree -- on every form
one process can reach, at the smallest meshes of tests/test_gpu_variants.py where the form engages, with that file's helpers and bars:

  undivided    solve_group against the oracle's CG on the conditioned twin: equal iteration counts, rel_l2 < 1e-10
  slab teams   fixed-work solve_keff against the oracle: k-history 1e-9, flux 1e-8

team_vec needs ranks: tests/test_gpu_multiproc.py (test_reduction_routes_agree) asserts it, with team_sr and team_lean, on every rank."""
import ctypes as C

import numpy as np
import pytest

from helpers import CG_FORMS, rel_l2
from test_gpu_variants import B, CLASSIC, FIXED, SLAB_SHAPE, WINDOW, _inputs, _ref_cg, _ref_keff, _set, _solver, _solves
from neutfem_amd.capi import HipTeam

pytestmark = pytest.mark.gpu


def _ran(s):
    return CG_FORMS[s.info("cg_form")]


UNDIVIDED = [("xcd", WINDOW[0], {}), ("fuse3", WINDOW[0], dict(cg_xcd=0)), ("lean", B, dict(CLASSIC)),
             ("fused", B, dict(CLASSIC, cg_lean=0)), ("classic", B, dict(CLASSIC, cg_fuse=0))]


@pytest.mark.parametrize("form,mesh,opts", UNDIVIDED, ids=[u[0] for u in UNDIVIDED])
def test_undivided_forms_are_planned_run_and_reported(form, mesh, opts):
    (shape, rt) = mesh
    s = _solver(shape, rt, opts, conditioned=True)
    assert s.apply_plan(False)["form"] == ""                        # outside CG there is no form
    plan = s.apply_plan(True)
    assert plan["form"] == form, plan
    # the keys the report had before the form was named: derived from the same plan
    assert plan["fused"] == int(form != "classic") and plan["lean"] == int(form in ("xcd", "fuse3", "lean")) and plan["single_reduce"] == 0, plan
    _solves(s, _ref_cg(shape, rt), form)
    assert _ran(s) == form and s.info("cg_reductions") == 0 and s.info("vec_reduce") == 0
    assert s.info("last_xcd") == int(form == "xcd") and s.info("xcd_refused") == 0
    s.close()


def test_refused_one_xcd_start_reports_the_form_it_continued_with():
    """cg_xcd_id = 8 names no XCD: nobody registers, the kernel says so before touching a vector and the solve goes on through the launches"""
    (shape, rt) = WINDOW[0]
    s = _solver(shape, rt, dict(cg_xcd_id=8), conditioned=True)
    assert s.apply_plan(True)["form"] == "xcd"                      # the plan cannot know what the device will answer
    _solves(s, _ref_cg(shape, rt), "xcd refused", groups=[0])
    assert _ran(s) == "fuse3" and s.info("xcd_refused") == 1 and s.info("last_xcd") == 0 and s.info("xcd_solves") == 0
    assert s.apply_plan(True)["form"] == "fuse3"                    # the solver stays off the one-XCD path, and the plan knows
    _solves(s, _ref_cg(shape, rt), "after the refusal", groups=[1])
    assert _ran(s) == "fuse3" and s.info("xcd_refused") == 1
    s.close()


def _team(inp, planes, rt, opts):
    t = HipTeam(rt, rt, int(inp["ng"]), inp["x_breaks"], inp["y_breaks"], inp["z_breaks"], planes)
    t.set_linear_solver(6)
    for a, ty in zip(inp["bc_attr"], inp["bc_type"]):
        t.set_bc(int(a), int(ty))
    t.upload_xs_global(inp["D"], inp["SigR"], inp["NSF"], inp["Chi"], inp["SigS"])
    t.build()
    _set(t.head, opts)
    return t


def _prepare(t):
    """one team apply (of zeros): the report needs the separator sweeps and endpoint weights that a team settles on its first apply or solve"""
    xs, ys = [s.vector().upload(np.zeros(s.n_phi)) for s in t.slabs], [s.vector() for s in t.slabs]
    xa, ya = (C.c_void_p * len(xs))(*[v.ptr for v in xs]), (C.c_void_p * len(ys))(*[v.ptr for v in ys])
    t.head._chk(t.L.nf_team_schur_apply(t.head.h, 0, xa, ya))
    for v in xs + ys:
        v.free()


THREE = [(0, 8), (8, 16), (16, 24)]
# classic on a team: RT1-P1 has no fused update to ride in a pass.  The oracle's fixed-work solve of R (70, 8, 8) at RT1-P1 takes 22 s, so
# the case runs on the RT1-P1 mesh of WINDOW as two slabs, against the reference test_one_xcd_kernels_with_other_workgroup_counts already
# computes (the same fixed work, inner limit 5000): four transverse modes per interface, 2 x 3 tiles per slab pass
FIXED_RT1 = (0.0, 1e-11, 1e-11, 6, 5000)
TEAMS = [("team_sr", SLAB_SHAPE, 0, THREE, dict(cg_single_reduce=1), 1, FIXED), ("team_lean", SLAB_SHAPE, 0, THREE, dict(cg_single_reduce=0), 2, FIXED),
         ("fused", SLAB_SHAPE, 0, THREE, dict(cg_lean=0), 2, FIXED), ("classic", WINDOW[1][0], WINDOW[1][1], [(0, 3), (3, 6)], {}, 2, FIXED_RT1)]


@pytest.mark.parametrize("form,shape,rt,planes,opts,reductions,tol", TEAMS, ids=[t[0] for t in TEAMS])
def test_team_forms_are_planned_run_and_reported(form, shape, rt, planes, opts, reductions, tol):
    ref = _ref_keff(shape, rt, tol=tol)
    t = _team(_inputs(shape), planes, rt, opts); t.set_tol(*tol)
    _prepare(t)
    for x in t.slabs:
        plan = x.apply_plan(True)
        assert plan["form"] == form and x.apply_plan(False)["form"] == "", plan
        assert plan["fused"] == int(form != "classic") and plan["lean"] == 0 and plan["single_reduce"] == int(form == "team_sr"), plan
    k, n = t.solve_keff()
    assert n == 6 and _ran(t.head) == form and t.head.info("cg_reductions") == reductions and t.head.info("vec_reduce") == 0
    h = t.history()
    phi = np.concatenate([s.get_phi().reshape(2, -1) for s in t.slabs], axis=1)
    errs = (np.abs(h["k"] / ref["hk"] - 1).max(), rel_l2(phi.ravel(), ref["phi"].ravel()))
    print(f"team {form}: k-history {errs[0]:.3e} (bar 1e-9), flux {errs[1]:.3e} (bar 1e-8)")
    np.testing.assert_allclose(h["k"], ref["hk"], rtol=1e-9)
    assert errs[1] < 1e-8
    t.close()
