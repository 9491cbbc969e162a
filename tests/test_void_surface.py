"""CPU-only tests of the cut-out-cells interface (nf_set_void): the pybind11 class keeps the mask on the object until
BuildMatrices(), validates it when it is set, and the C ABI declares and exports the two entry points.  No compute call is made here."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as m
    return m


def _solver(m, dim=3):
    yb = np.linspace(0, 20, 3) if dim >= 2 else np.array([0.0])
    zb = np.linspace(0, 10, 6) if dim == 3 else np.array([0.0])
    s = m.NeutFEM(0, 2, np.linspace(0, 30, 4), yb, zb)
    s.set_verbosity(m.VerbosityLevel.SILENT)
    return s


def test_methods_exist_and_round_trip():
    m = _module()
    for name in ("set_void", "clear_void", "get_void"):
        assert hasattr(m.NeutFEM, name), name
    s = _solver(m)
    assert s.get_void() is None
    mask = np.zeros(s.get_D().shape[1:], bool); mask[4] = True; mask[0, 1, 2] = True
    s.set_void(mask, 0.4692)
    got, gamma = s.get_void()
    assert got.dtype == bool and got.shape == mask.shape and np.array_equal(got, mask) and gamma == 0.4692
    for dtype in (np.uint8, np.int32, np.int64):                 # any integer dtype, non-zero = void
        s.set_void(7 * mask.astype(dtype), 0.5)
        got, gamma = s.get_void()
        assert np.array_equal(got, mask) and gamma == 0.5
    s.clear_void()
    assert s.get_void() is None


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_wrong_shape_raises(dim):
    m = _module()
    s = _solver(m, dim)
    shape = s.get_D().shape[1:]
    assert len(shape) == dim
    s.set_void(np.zeros(shape, bool), 0.4692)                    # the right shape is taken (no set byte: no mask at the next build)
    for bad in (shape + (1,), shape[:-1] + (shape[-1] + 1,), (int(np.prod(shape)),) if dim > 1 else (shape[0], 1), s.get_D().shape):
        with pytest.raises((ValueError, RuntimeError)):
            s.set_void(np.zeros(bad, bool), 0.4692)
    assert np.array_equal(s.get_void()[0], np.zeros(shape, bool))    # a refused call changes nothing


@pytest.mark.parametrize("gamma", [0.0, -0.4692, float("inf"), float("nan")])
def test_bad_gamma_raises(gamma):
    m = _module()
    s = _solver(m)
    mask = np.zeros(s.get_D().shape[1:], bool); mask[0] = True
    with pytest.raises((ValueError, RuntimeError)):
        s.set_void(mask, gamma)
    assert s.get_void() is None


def test_all_void_raises():
    m = _module()
    s = _solver(m)
    with pytest.raises((ValueError, RuntimeError)):
        s.set_void(np.ones(s.get_D().shape[1:], bool), 0.4692)


def test_header_declares_and_library_exports():
    src = open(os.path.join(ROOT, "include", "neutfem_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+nf_set_void\s*\(\s*nf_handle\s+\w+\s*,\s*const\s+unsigned\s+char\s*\*\s*\w+\s*,\s*double\s+\w+\s*\)\s*;", code)
    assert re.search(r"int\s+nf_get_void\s*\(\s*nf_handle\s+\w+\s*,\s*unsigned\s+char\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", code)
    assert "void_cells" in src
    from neutfem_amd import capi
    L = capi.load()
    assert hasattr(L, "nf_set_void") and hasattr(L, "nf_get_void")
    assert hasattr(capi.HipSolver, "set_void") and hasattr(capi.HipSolver, "get_void")
    assert L.nf_set_void(None, None, 0.4692) != 0 and b"nf_set_void" in L.nf_last_error()
    assert L.nf_get_void(None, None, None) != 0
