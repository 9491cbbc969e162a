"""nf_set_option / nf_get_option through the C ABI on one tiny RT0-P0 mesh (8 x 6 x 5 cells, 2 groups): what a key stores, what
NEUTFEM_OPTS sets at creation, and which options the fine handle of nf_refine -- a twin of the caller's mesh kind -- starts with.
The expected values are written out from the documented behaviour of the keys (include/neutfem_hip.h, neutfem_amd/csrc/nf_options.h);
the table itself and the copy to a coarse twin are checked without a device in tests/test_options_host.py, the coarse twin under
options in tests/test_gpu_driver_forms.py."""
import os
import subprocess
import sys

import pytest

from helpers import make_hip, synthetic_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = (8, 6, 5, 2)

BOOLS = ("vec_reduce", "endpoint_weights", "xchg_comm", "xy_overlap", "cg_fuse", "host_pub", "nt_loads", "outer_dev", "cg_lean", "sep_fold", "resident",
         "resident_lds", "resident_serial", "resident_two_sided", "cg_fuse3", "cg_xcd", "keff_xcd", "transient_rebalance")
RAW = ("nt_min_cells", "cg_lean_max_cells", "resident_serial_max_dofs", "cg_xcd_min_cells", "cg_xcd_max_cells", "cg_fuse3_max_cells")
# key: (input in range, stored), (input out of range, stored)
STORED = {
    **{k: ((0, 0), (5, 1)) for k in BOOLS},
    **{k: ((0, 0), (9, 1)) for k in ("cg_single_reduce", "s_long", "s_stage", "tile_full", "line_dict")},
    "c_early": ((0, 0), (9, 2)), "split_dot": ((2, 2), (-3, 0)), "s_wsmin": ((7, 7), (10**7, 100000)), "s_stage_grid": ((12, 12), (2**40, 2**20)),
    "s_long_min": ((100, 100), (0, 1)), "s_long_min_y": ((100, 100), (10**7, 10**6)), "line_dict_max_bytes": ((4096, 4096), (2**40, 2**30)),
    "line_dict_fp_bits": ((64, 64), (1000, 128)), "direct_max_dofs": ((100, 100), (10**7, 8192)), "cg_xcd_groups": ((8, 8), (100, 64)),
    "cg_lean_grid": ((16, 16), (4096, 1024)), "kin_grid": ((16, 16), (4096, 1024)), "sens_grid": ((16, 16), (10**7, 65536)),
    "cg_single_reduce_max_cells": ((4096, 4096), (-7, 0)), "xy_overlap_max_cells": ((4096, 4096), (-7, 0)),
    "s_long_dirs": ((2, 2), (5, 1)), "line_dict_dirs": ((5, 5), (10, 2)), "cg_xcd_id": ((9, 9), (19, 3)), "xcd": ((5, 5), (-7, -1)),
    "cg_batch": ((4, 4), (2**40 + 3, 3)),                        # narrowed to int
    **{k: ((4096, 4096), (-7, -7)) for k in RAW},                # stored as given
    "resident_max_dofs": ((100, 100), (10**7, 10**7)),
    "s_pair": ((1, 0), (-7, 0)), "x_two_phase": ((1, 0), (-7, 0)),   # retired: accepted, read 0
}
# key: legal value, refused value, the message of the refusal
REFUSED = {"s_tx": (16, 5, "nf_set_option: s_tx must be 0 (auto), 8, 16, 32 or 64"), "s_seg": (8, 64, "nf_set_option: s_seg must be 0 (auto), 4, 8, 16 or 32"),
           "prof_every": (3, 0, "prof_every must be >= 1")}
# what stays with the handle it was set on: a twin shows the default
NOT_COPIED = {"xchg_comm": 0, "transient_rebalance": 1, "s_pair": 0, "x_two_phase": 0}


@pytest.fixture(scope="module")
def inputs():
    return synthetic_inputs(*MESH)


def test_every_key_stores_its_normalised_value(inputs):
    assert len(STORED) + len(REFUSED) == 55
    s = make_hip(inputs)
    try:
        for key, cases in STORED.items():
            for value, want in cases:
                s.set_option(key, value)
                assert s.get_option(key) == want, (key, value)
        assert s.get_option("resident_serial_max_dofs") == 5120  # resident_max_dofs = 10^7 capped the serial variant at its structural limit
        s.set_option("resident_max_dofs", 100)
        assert s.get_option("resident_serial_max_dofs") == 100
        for key, (good, bad, message) in REFUSED.items():
            s.set_option(key, good)
            with pytest.raises(RuntimeError) as e:
                s.set_option(key, bad)
            assert str(e.value).endswith(": " + message), (key, str(e.value))
            assert s.get_option(key) == good, key
        for call in (lambda: s.set_option("bogus", 1), lambda: s.get_option("bogus")):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "unknown key bogus" in str(e.value)
    finally:
        s.close()


CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from helpers import make_hip, synthetic_inputs
s = make_hip(synthetic_inputs(*{mesh!r}))
print("OPTS", s.get_option("s_tx"), s.get_option("cg_lean"), s.get_option("s_seg"), s.get_option("cg_fuse"))
s.close()
"""


def test_environment_options_at_creation():
    env = dict(os.environ, NEUTFEM_OPTS="s_tx=16,cg_lean=0,bogus=1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, mesh=MESH)], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "OPTS 16 0 0 1" in r.stdout                           # the two that were named; their neighbours at the defaults
    assert "NEUTFEM_OPTS: nf_set_option: unknown key bogus" in r.stderr


def test_refined_twin_starts_with_the_callers_options(inputs):
    s = make_hip(inputs)
    fine = None
    try:
        defaults = {key: s.get_option(key) for key in list(STORED) + list(REFUSED)}
        assert all(defaults[key] == want for key, want in NOT_COPIED.items())
        chosen = {**{key: cases[0][0] for key, cases in STORED.items()}, **{key: good for key, (good, _, _) in REFUSED.items()}}
        chosen.update(xchg_comm=1, cg_single_reduce=1, s_long=1, s_stage=1, tile_full=1, line_dict=1, c_early=1, resident_serial_max_dofs=4096)
        del chosen["resident_max_dofs"]                          # it would move resident_serial_max_dofs as well: set last, below
        for key, value in chosen.items():
            s.set_option(key, value)
        s.set_option("resident_max_dofs", 100); s.set_option("resident_serial_max_dofs", 4096)
        mine = {key: s.get_option(key) for key in defaults}
        moved = [key for key in defaults if mine[key] != defaults[key]]
        assert sorted(moved) == sorted(set(defaults) - {"s_pair", "x_two_phase"}), "every key but the retired ones holds a non-default value"
        fine = s.refine(1, 1, 2)
        for key in defaults:
            assert fine.get_option(key) == (NOT_COPIED[key] if key in NOT_COPIED else mine[key]), key
        assert {key: s.get_option(key) for key in defaults} == mine   # the copy reads the caller's options, it does not touch them
    finally:
        if fine is not None:
            fine.close()
        s.close()
