"""Long y / z lines: the kernel branches BASELINE config 4 (synthetic 512^3) runs and every other length class of the
segmented line kernels (neutfem_amd/csrc: launch_s / k_schur_s / the chunked long-line pass), against the oracle's
SchurProduct (src/solvers.cpp:535-547) at 1e-12, plus a full SolveKeff on the C5 generator with 512-cell z lines."""
import numpy as np
import pytest

from helpers import make_hip, make_oracle, rel_l2, synthetic_inputs

pytestmark = pytest.mark.gpu

# (nx, ny, nz): y or z lines of 505 ... 2100 cells on thin meshes -- 512 / 600 / 1023 / 1024 (one segment class), 576 and 1024
# (the lengths the round-2 wavefront scan hung on: 72 ... 128 segments), 1100 / 2047 (16-cell segments), 2100 (32-cell segments)
LONG = [(16, 16, 512), (24, 600, 3), (8, 8, 1024), (8, 576, 2), (40, 1023, 2), (3, 5, 1023), (8, 4, 1100), (6, 3, 2047), (4, 2100, 2),
        (70, 512, 3), (33, 3, 640), (64, 2, 515),
        # 256-cell lines: both run the one-chunk kernel (32 segments x 32 columns) -- y lines of 256 cells are past s_long_min_y, but below 1024
        # tiles chunk_plan leaves lines of at most 256 cells to it (the chunked kernel at this length: 256^3 and tests/test_gpu_variants.py);
        # 255 / 257 either side of both thresholds: 257 and 300 take the chunked kernel
        (40, 256, 3), (8, 4, 256), (33, 255, 2), (9, 257, 2), (5, 3, 257), (70, 300, 2)]


def _apply(inp, rt=0, p=0, tol=1e-12, opts=None, groups=None):
    o, s = make_oracle(inp, rt, p), make_hip(inp, rt, p)
    for k, v in (opts or {}).items():
        s.set_option(k, v)
    rng = np.random.default_rng(3)
    out = []
    for g in (groups if groups is not None else range(int(inp["ng"]))):
        x = rng.standard_normal(o.n_phi)
        x[rng.random(o.n_phi) < 0.1] *= 1e-12
        ya, yb = s.schur_apply(g, x), o.schur_apply(g, x)
        assert np.isfinite(ya).all()
        assert np.abs(ya - yb).max() <= tol * np.abs(yb).max(), (g, np.abs(ya - yb).max() / np.abs(yb).max())
        out.append(ya)
    s.close()
    return out


@pytest.mark.parametrize("shape", LONG)
def test_schur_apply_long_lines(shape):
    nx, ny, nz = shape
    _apply(synthetic_inputs(nx, ny, nz, 2, seed=nx + 7 * ny + 13 * nz))


@pytest.mark.parametrize("shape", [(16, 16, 512), (12, 600, 2), (8, 8, 1024)])
@pytest.mark.parametrize("opts", [dict(s_long=0), dict(s_long=0, s_wsmin=8), dict(s_long=0, s_wsmin=100000), dict(s_long=1), dict(s_long=1, s_tx=64), dict(s_long=1, s_tx=16)])
def test_long_line_variants_agree(shape, opts):
    """every variant a long line can take (classic one-chunk kernel with serial / wavefront-scanned segment summaries, chunked
    long-line kernel at several tile widths) against the oracle, and bitwise-comparable among themselves to 1e-13"""
    nx, ny, nz = shape
    inp = synthetic_inputs(nx, ny, nz, 1, seed=11)
    ya = _apply(inp, opts=opts)[0]
    yb = _apply(inp, opts=dict(s_long=0, s_wsmin=100000))[0]
    assert rel_l2(ya, yb) < 1e-13


@pytest.mark.parametrize("seed", range(10))
def test_chunked_kernel_random_shapes(seed):
    """the chunked long-line kernel forced onto every y / z line (s_long = 1), shapes drawn at random: line lengths from 2 cells (one
    segment, an empty second chunk) to 700, odd lengths, meshes narrower than a tile, every tile width -- against the oracle, and inside
    a CG solve (split dot product: per-pass shares of p.q, z.w form) against the one-chunk kernels"""
    rng = np.random.default_rng(100 + seed)
    nx = int(rng.integers(6, 70)); ny = int(rng.integers(3, 12 if seed % 2 else 700)); nz = int(rng.integers(3, 700 if seed % 2 else 12))
    while nx * ny * nz < 200: nx += 5
    if seed == 0: nx, ny, nz = 30, 2, 4                            # two-cell y lines: one segment, an empty second chunk (>= 200 unknowns: below,
                                                                   # the reference's Schur solver forms S explicitly, src/solvers.cpp:114-124)
    if seed == 1: nx, ny, nz = 64, 17, 33
    inp = synthetic_inputs(nx, ny, nz, 1, seed=seed)
    opts = dict(s_long=1, s_tx=[0, 8, 16, 32, 64][seed % 5])
    _apply(inp, opts=opts)
    o, s = make_oracle(inp), make_hip(inp)
    for k, v in dict(opts, resident=0, cg_fuse3=0, cg_lean=0, split_dot=2).items():
        s.set_option(k, v)
    rhs = np.abs(rng.standard_normal(o.n_phi))
    o.set_tol(1e-5, 1e-11, 1e-11, 200, 5000)
    xo, _, its_o = o.solve_group(0, rhs)
    xs, its_s, res = s.solve_group(0, rhs, 1e-11, 5000)
    assert res < 1e-11 and abs(its_s - its_o) <= max(2, 0.05 * its_o), (its_s, its_o)
    assert rel_l2(xs, xo) < 1e-9
    s.close()


@pytest.mark.parametrize("rt,p", [(1, 1), (2, 2), (1, 0)])
@pytest.mark.parametrize("shape", [(6, 300, 2), (5, 3, 600), (8, 512, 1), (4, 2, 1000)])
def test_schur_apply_long_lines_higher_order(rt, p, shape):
    nx, ny, nz = shape
    _apply(synthetic_inputs(nx, ny, nz, 1, seed=nx + ny + nz + rt), rt, p)


def test_solve_keff_c5_generator_512_cell_lines():
    """the C5 generator (neutfem_amd.cases.synthetic_checkerboard: 16-cell checkerboard, 8 groups, one up-scatter block) cut to a
    16 x 16 x 512 column -- 512-cell z lines as in the 512^3 benchmark -- full SolveKeff against the oracle:
      (a) 2 outers with the inner CG converged to 1e-10: the iteration path does not depend on CG counts -> k 1e-9, flux 1e-8;
      (b) the bench's fixed work (exactly 50 CG iterations per group solve, 3 outers).  Fifty iterations leave the CG unconverged, and
          an unconverged Krylov iterate amplifies rounding differences: two builds of the ORACLE itself (with / without FMA contraction,
          tests/golden/rounding_spread.json "c5_column_fixed50:0") end 1.6e-7 apart in k and 1.9e-5 in flux on this run.  Equal CG
          counts, k within 0.1 pcm, flux within three times that measured spread."""
    from neutfem_amd import cases
    c = cases.synthetic_checkerboard(512, 8, nxy=16)
    inp = dict(c, bc_attr=np.array([1, 2, 3, 4, 5, 6]), bc_type=np.zeros(6, int))
    o, s = make_oracle(inp), make_hip(inp)
    import json, os
    with open(os.path.join(os.path.dirname(__file__), "golden", "rounding_spread.json")) as f:
        spread = json.load(f)["c5_column_fixed50:0"]["flux_rel_l2"]
    for tol, kbar, fbar in [((0.0, 1e-10, 1e-10, 2, 4000), 1e-9, 1e-8), ((0.0, 0.0, 1e-4, 3, 50), 1e-6, 3.0 * spread)]:
        o.reset_flux(); s.reset_flux()
        o.set_tol(*tol); s.set_tol(*tol)
        ko = o.SolveKeff(); ks, n = s.solve_keff()
        assert n == tol[3] and abs(ks - ko) / ko < kbar, (tol, ks, ko)
        np.testing.assert_allclose(s.history()["k"], o.history()["k"], rtol=2 * kbar)
        assert rel_l2(s.get_phi().ravel(), o.phi_dofs().ravel()) < fbar, tol
        if tol[4] == 50:
            assert np.array_equal(s.history()["cg"], o.history()["cg"])
    s.close()


def test_full_size_512cube_properties():
    """BASELINE config 4 at full size and with ALL 8 of its groups (synthetic checkerboard 512^3 x 8 groups: 134 M cells, ~130 GB of HBM,
    512-cell lines in all three directions, the chunked y / z passes with 32 columns x 1024 threads), where the oracle is not run:
    size-independent properties of EVERY S_g -- linear, symmetric, positive -- through the same nf_schur_apply the bench times; a CG
    solve that really leaves |S x - b| <= tol |b| (checked with a separate apply; inside CG the split dot product is in use); the same
    apply against the one-chunk kernels (s_long = 0) at 1e-13; and one outer iteration of the bench's fixed work (50 CG iterations per
    group solve through the Gauss-Seidel sweep with its 8 scatter blocks).  bench.py's C5 leg repeats the group 0 / 7 checks on the
    kernels it has just timed and compares all 8 groups with the oracle on a 32 x 32 x 512 column; test_solve_keff_c5_generator_512_cell_lines runs
    the whole 8-group SolveKeff against the oracle on a 16 x 16 x 512 column."""
    from bench import make_solver
    from neutfem_amd import capi, cases
    free_b, _ = capi.mem_info(0)
    with open("/proc/meminfo") as f:
        avail_kb = next(int(l.split()[1]) for l in f if l.startswith("MemAvailable"))
    ng = 8 if (free_b >= 180e9 and avail_kb * 1024 >= 110e9) else 2     # a box without the HBM / host memory of an MI355X node still checks two groups
    c = cases.synthetic_checkerboard(512, ng)
    s = make_solver(c, 0)
    c.pop("SigS", None)
    n = s.n_phi
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    z = 2.0 * x - 3.0 * y
    Sx = None
    for g in range(ng):
        Sx, Sy = s.schur_apply(g, x), s.schur_apply(g, y)
        Sxy = s.schur_apply(g, z)
        assert rel_l2(Sxy, 2.0 * Sx - 3.0 * Sy) < 1e-12, g
        assert abs(y @ Sx - x @ Sy) <= 1e-10 * abs(y @ Sx), g
        assert x @ Sx > 0, g
        del Sy, Sxy
    g = ng - 1
    b = np.abs(y)
    xs, its, res = s.solve_group(g, b, 1e-5, 3000)
    assert 0 < its < 3000 and res < 1e-5
    assert np.linalg.norm(s.schur_apply(g, xs) - b) < 1.05e-5 * np.linalg.norm(b)
    s.set_tol(0.0, 0.0, 1e-4, 1, 50)                               # fixed work
    k, n_out = s.solve_keff()
    h = s.history()
    assert n_out == 1 and (h["cg"] == 50).all() and h["cg"].shape == (1, ng) and np.isfinite(h["dphi"][0]) and h["dk"][0] > 0
    phi = s.get_phi()
    assert np.isfinite(phi).all() and abs(np.linalg.norm(phi) - 1.0) < 1e-12 and (phi >= 0).all()
    s.set_option("s_long", 0)
    assert rel_l2(s.schur_apply(g, x), Sx) < 1e-13                 # Sx = the last group from the loop above
    s.close()
