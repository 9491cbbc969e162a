"""CPU tests of the fixed-source (subcritical) solve: the exact yardstick of tests/subcrit_exact.py and the pybind surface.

The homogeneous medium has no leakage-free closed form on this discretisation: MIRROR (like NEUMANN) is the natural condition of the
mixed form, i.e. a weak zero-flux condition, not a reflective one, so a uniform source in a homogeneous box does not give
the infinite-medium flux Q / (Sigma_r - nuSigma_f).  What holds exactly is the homogeneous medium's own closed form: removal and fission act
through the same mass matrix, so with one group the fission solve equals the no-fission solve with Sigma_r - nuSigma_f, and
M = Phi0[Sigma_r - nuSigma_f] / Phi0[Sigma_r]."""
import copy

import numpy as np
import pytest

from subcrit_exact import exact_subcritical, homogeneous_inputs, ref_from_inputs


@pytest.mark.parametrize("rt,p", [(0, 0), (1, 1)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_exact_helper_homogeneous_closed_form(rt, p, dim):
    inp = homogeneous_inputs(dim, 1, n=(4, 3, 2))
    src = np.full((1, inp["D"][0].size), 2.5)
    ex = exact_subcritical(ref_from_inputs(inp, rt, p), src)
    red = copy.deepcopy(inp)
    red["SigR"] = inp["SigR"] - inp["NSF"]; red["NSF"] = np.zeros_like(inp["NSF"])
    ex_red = exact_subcritical(ref_from_inputs(red, rt, p), src)
    np.testing.assert_allclose(ex["phi"], ex_red["phi0"], rtol=1e-12, atol=1e-12 * np.abs(ex["phi"]).max())
    assert abs(ex["M"] - ex_red["phi_int_nofission"] / ex["phi_int_nofission"]) <= 1e-12 * ex["M"]
    assert ex["M"] > 1.0 and 0.0 < ex["k_source"] < 1.0
    assert abs(ex["source"] - 2.5 * (np.diff(inp["x_breaks"]).sum() * (np.diff(inp["y_breaks"]).sum() if dim >= 2 else 1.0)
                                     * (np.diff(inp["z_breaks"]).sum() if dim == 3 else 1.0))) <= 1e-12 * ex["source"]
    # a uniform source in this box is NOT the infinite medium (weak zero-flux faces): the flux stays below Q / (Sigma_r - nuSigma_f)
    assert ex["phi"].reshape(1, -1, ex["phi"].shape[1] // inp["D"][0].size)[..., 0].max() < 2.5 / (inp["SigR"] - inp["NSF"]).max()


def test_exact_helper_two_groups_loads_dof0_only():
    inp = homogeneous_inputs(2, 2, n=(3, 3, 1))
    r = ref_from_inputs(inp, 1, 1)
    src = np.array([np.arange(9.0) + 1.0, np.zeros(9)])
    ex = exact_subcritical(r, src)
    q = ex["q"].reshape(2, 9, 4)
    assert (q[..., 1:] == 0).all() and (q[1] == 0).all()
    np.testing.assert_allclose(q[0, :, 0], src[0] * 2.0 * 2.5)          # |e| = 2 x 2.5
    assert ex["M"] > 1.0 and ex["phi"][1].sum() > 0                      # downscatter feeds group 2


def test_pybind_solve_subcritical_needs_build_and_info_is_bound():
    import neutfem_amd
    neutfem_amd.install_compat()
    import neutfem._neutfem_eigen as m
    assert hasattr(m.NeutFEM, "get_subcritical_info")
    s = m.NeutFEM(0, 2, np.linspace(0, 30, 4), np.linspace(0, 20, 3), np.array([0.0]))
    s.set_verbosity(m.VerbosityLevel.SILENT)
    s.get_SRC()[0] = 1.0
    with pytest.raises(RuntimeError, match=r"call BuildMatrices\(\) first"):
        s.SolveSubcritical()
    with pytest.raises(RuntimeError, match="SolveSubcritical"):
        s.get_subcritical_info()
