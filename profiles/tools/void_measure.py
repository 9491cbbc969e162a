"""Measurements of DESIGN.md 17 (set_void) on one GPU.
  python profiles/tools/void_measure.py cost [n]        time per CG iteration of an n^3 (default 128) RT0-P0 mesh with the stepped mask of
                                                        tests/test_gpu_void.py against the same mesh without it: fixed work of 3 outers x 2
                                                        groups x 200 CG iterations, three rounds in alternating order
  python profiles/tools/void_measure.py iaea3d RT M     IAEA-3D as specified (tests/golden/iaea3d_as_specified.json) at RT = P, M cells per
                                                        assembly and axis: k, pcm, outer and CG counts, build and solve time
One JSON line per result, prefixed RESULT."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import CG_FORMS, synthetic_inputs          # noqa: E402
import test_gpu_void as T                                # noqa: E402


def cost(n):
    inp = synthetic_inputs(n, n, n, 2, seed=7, dirichlet=(1, 3, 5))
    mask = T.void_mask(n, n, n)
    inp["NSF"][:, mask] = 0.0; inp["Chi"][:, mask] = 0.0; inp["SigS"][:, :, mask] = 0.0
    print("void cells", int(mask.sum()), "of", mask.size, flush=True)
    tol = (0.0, 1e-30, 1e-30, 3, 200)                              # every group solve runs its 200 iterations, whatever the residual
    res = {}
    for rnd in range(3):
        for label, m in ((("masked", mask), ("plain", None)) if rnd % 2 == 0 else (("plain", None), ("masked", mask))):
            s = T._hip(inp, 0, m)
            s.set_tol(*tol)
            s.solve_keff()                                        # warm-up: allocations, plan
            s.reset_flux(); s.set_warm_state(0, 1.0)
            t0 = time.perf_counter(); s.solve_keff(); dt = time.perf_counter() - t0
            its = s.info("last_cg_total")
            rec = dict(round=rnd, its=its, seconds=dt, us_per_it=1e6 * dt / its, form=CG_FORMS[s.info("cg_form")], path=s.info("last_path"), void=s.info("void_cells"))
            print(label, json.dumps(rec), flush=True)
            res.setdefault(label, []).append(rec["us_per_it"])
            s.close()
    print("RESULT masked_cost", json.dumps(res), flush=True)


def iaea3d(rt, m):
    inp, blank = T._iaea3d_spec(m)
    t0 = time.perf_counter(); s = T._hip(inp, rt, blank); tb = time.perf_counter() - t0
    s.set_tol(1e-8, 1e-7, 1e-7, 1000, 5000)
    t0 = time.perf_counter(); k, n = s.solve_keff(); dt = time.perf_counter() - t0
    print("RESULT iaea3d_spec", json.dumps(dict(rt=rt, m=m, k=k, pcm=1e5 * (1 / 1.029096 - 1 / k), outers=n, cg=s.info("last_cg_total"), solve_s=dt, build_s=tb,
          form=CG_FORMS[s.info("cg_form")], n_phi=s.n_phi, void=s.info("void_cells"))), flush=True)
    s.close()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "cost":
        cost(int(sys.argv[2]) if len(sys.argv) > 2 else 128)
    elif len(sys.argv) == 4 and sys.argv[1] == "iaea3d":
        iaea3d(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(__doc__)
