"""CPU-only: the surfaces of nf_solve_keff_batch exist in the C header, the ctypes binding and the pybind11 module.
No compute call is made here; tests/test_gpu_batch.py runs them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "neutfem_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_batch_call_and_its_result():
    h = _header()
    m = re.search(r"typedef\s+struct\s+nf_batch_result\s*\{(.*?)\}\s*nf_batch_result\s*;", h, flags=re.S)
    assert m, "include/neutfem_hip.h lacks nf_batch_result"
    fields = re.findall(r"\b(n_batched|n_sequential|n_launches|variant)\b", m.group(1))
    assert fields == ["n_batched", "n_sequential", "n_launches", "variant"] and re.match(r"\s*int\b", m.group(1))
    proto = re.search(r"int\s+nf_solve_keff_batch\s*\(([^)]*)\)\s*;", h)
    assert proto, "include/neutfem_hip.h lacks nf_solve_keff_batch"
    args = [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]
    assert args == ["nf_handle *h", "int n", "const nf_keff_opts *opts", "int n_opts", "double *keff", "int *n_outer", "int *status", "nf_batch_result *res"]


def test_capi_exposes_solve_keff_batch():
    import ctypes as C
    from neutfem_amd import capi
    assert callable(capi.solve_keff_batch) and "nf_solve_keff_batch" in capi.SYMBOLS
    L = capi.load()
    assert hasattr(L, "nf_solve_keff_batch")
    assert [n for n, _ in capi.BatchResult._fields_] == ["n_batched", "n_sequential", "n_launches", "variant"]
    assert C.sizeof(capi.BatchResult) == 4 * C.sizeof(C.c_int)
    # refused before any device call, the status array untouched: no handles, and a NULL handle
    st = (C.c_int * 2)(77, 77)
    o = capi.KeffOpts()
    assert L.nf_solve_keff_batch(None, 0, C.byref(o), 1, None, None, st, None) == -1 and b"nf_solve_keff_batch" in L.nf_last_error()
    hs = (C.c_void_p * 2)(None, None)
    assert L.nf_solve_keff_batch(hs, 2, C.byref(o), 1, None, None, st, None) == -1 and list(st) == [77, 77]


def test_pybind_module_exposes_the_batch_functions():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as m
    import pytest
    assert callable(m.SolveKeffBatch) and callable(m.get_batch_info)
    for name in ("SolveKeff", "GetLastKeff", "get_flux", "reset_flux", "BuildMatrices"):   # the methods the batch works over (tests/test_boundary.py lists them)
        assert hasattr(m.NeutFEM, name), name
    doc = m.SolveKeffBatch.__doc__
    for arg in ("solvers", "use_coarse_init", "coarse_factors", "use_diagonal_solver", "use_cmfd"):
        assert arg in doc, arg
    with pytest.raises(ValueError):
        m.SolveKeffBatch([])
    import numpy as np
    s = m.NeutFEM(0, 2, np.linspace(0, 30, 4), np.linspace(0, 20, 3), np.array([0.0]))
    s.set_verbosity(m.VerbosityLevel.SILENT)
    with pytest.raises(RuntimeError, match="BuildMatrices"):
        m.SolveKeffBatch([s])                                  # not built: the message SolveKeff gives
    with pytest.raises(ValueError):
        m.SolveKeffBatch([s, s])
