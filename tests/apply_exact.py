"""Extended-precision restatement of the RT0-P0 Schur apply y = C_g x + B A_g^-1 B^T x, with a per-component scale (test infrastructure).

Plain numpy in np.longdouble (x87 extended: 64 bits of mantissa), 1D / 2D / 3D.  The inputs are taken as the input dict gives them
(doubles), converted once, and everything after that -- geometric factors, the closed-form line tridiagonals, a sequential Thomas
sweep batched over the lines of a direction, the sums -- runs in extended precision.  No part of it is shared with the oracle, the
scipy twin or the kernels.

Closed forms (oracle/nf_oracle.c geom_factors / boundary_face_integral), dim = 1, 2, 3, w = 2^(dim-1):
  A_LL = A_RR = w (2/3) f_d / D,  A_LR = w (1/3) f_d / D,  B = -+ beta with beta = w,  C = Sigma_R V
  f_d:  1D  hx / 2;   2D  f_x = hy / hx, f_y = hx / hy (the reference's 2D factor, kept as it is: tests/test_gpu_assembly.py);
        3D  f_x = 2 hx / (hy hz) and cyclic
  Dirichlet (boundary attribute of type 0): + 2 D (1D), 8 D / area (2D), 32 D / area (3D) on the boundary face's diagonal entry
In 3D: A_LL = (8/3) f_d / D, A_LR = (4/3) f_d / D, beta = 4 -- what tests/slab_numpy.py states.

The scale of component i is the magnitude of the terms that ANY evaluation order has to add to form y_i,
    s_i = |C_i x_i| + sum_d beta (|u_d,i| + |u_d,i+1|),    u_d = A_d^-1 B_d^T x  the face solution of direction d,
and the metric is rho = max_i |y_i - y_exact,i| / s_i: "per component".  A normwise bar (max |dy| / max |y|) sees only the largest
entries: with IAEA-3D's filler material (D = 1e-3, Sigma_R = 1e15) max |y| is 1e19 and the fuel cells, |y| in the hundreds, could hold
anything.

Also here: f6_block_inputs (block-structured inputs with that filler), exact_cg2 (two CG steps on the exact apply), and ExactTwin, the
same yardstick for the higher orders: the scipy twin's operator with exact local tables, applied by iterative refinement.  exact_cg2_op
runs the two CG steps on any such operator, ExactTwin.outer one outer iteration of SolveKeff for any order, and ORDER_CASES with
order_ref_cg / order_ref_outer are the cases and shared references of tests/test_gpu_orders_exact.py."""
import numpy as np

LD = np.longdouble
# the reference must carry more digits than what it judges; on a platform where long double is double this file proves nothing
assert np.finfo(LD).eps <= 2.0 ** -63, "apply_exact needs an extended-precision np.longdouble (x87), eps = %r" % np.finfo(LD).eps

EPS = 2.0 ** -53
# bars of the GPU tests, rho <= K x 2^-53: measured on an MI355X, table and rule in the docstring of tests/test_gpu_apply_exact.py
K_APPLY, K_SOLVE, K_HIGHER = 64, 8192, 256
F6_D, F6_SIGR = 1e-3, 1e15                                        # IAEA-3D's filler (tests/iaea3d/iaea3d.py of the reference: material 6)


def _mesh(inp):
    xb, yb, zb = (np.asarray(inp[k], dtype=np.float64) for k in ("x_breaks", "y_breaks", "z_breaks"))
    nx = len(xb) - 1; ny = len(yb) - 1 if len(yb) > 1 else 1; nz = len(zb) - 1 if len(zb) > 1 else 1
    dim = 3 if nz > 1 else (2 if ny > 1 else 1)
    one = np.ones(1, dtype=LD)
    hx = np.diff(xb).astype(LD)
    hy = np.diff(yb).astype(LD) if dim >= 2 else one
    hz = np.diff(zb).astype(LD) if dim == 3 else one
    return dim, (nz, ny, nx), (hx[None, None, :], hy[None, :, None], hz[:, None, None])


def _attr(dim, d, upper):
    """boundary attribute of the lower / upper side of direction d (src/NeutFEM.cpp:2338-2347)"""
    if dim == 1: return 2 if upper else 1
    if dim == 2: return (2 if upper else 1) if d == 0 else (3 if upper else 4)
    return [(3, 4), (6, 5), (1, 2)][d][1 if upper else 0]


def thomas(diag, off, rhs):
    """sequential tridiagonal solve along axis 0, batched over the rest: diag (n, ...), off (n-1, ...) symmetric, rhs (n, ...)"""
    n = diag.shape[0]
    d = diag.copy(); b = rhs.copy()
    for i in range(1, n):
        w = off[i - 1] / d[i - 1]
        d[i] = d[i] - w * off[i - 1]
        b[i] = b[i] - w * b[i - 1]
    u = np.empty_like(b)
    u[n - 1] = b[n - 1] / d[n - 1]
    for i in range(n - 2, -1, -1):
        u[i] = (b[i] - off[i] * u[i + 1]) / d[i]
    return u


class ExactApply:
    """the operator of one group of an input dict: apply(x) -> (y, s), both np.longdouble of shape (cells,)"""

    def __init__(self, inp, g):
        dim, shape, (HX, HY, HZ) = _mesh(inp)
        self.dim, self.shape = dim, shape
        D = np.asarray(inp["D"], dtype=np.float64)[g].reshape(shape).astype(LD)
        Sig = np.asarray(inp["SigR"], dtype=np.float64)[g].reshape(shape).astype(LD)
        two, three = LD(2), LD(3)
        self.C = Sig * (HX * HY * HZ)
        if dim == 1: fac, area, dterm = [HX / two], [None], LD(2)
        elif dim == 2: fac, area, dterm = [HY / HX, HX / HY], [HY * HZ, HX * HZ], LD(8)
        else: fac, area, dterm = [two * HX / (HY * HZ), two * HY / (HX * HZ), two * HZ / (HX * HY)], [HY * HZ, HX * HZ, HX * HY], LD(32)
        w = LD(2 ** (dim - 1))
        self.beta = w
        bc = {int(a): int(t) for a, t in zip(inp["bc_attr"], inp["bc_type"])}
        self.lines = []                                           # per direction: (numpy axis, diag (n+1, ...), off (n, ...))
        for d in range(dim):
            ax = 2 - d
            a2 = np.moveaxis(np.broadcast_to(w * (two / three) * fac[d] / D, shape), ax, 0)
            a1 = np.moveaxis(np.broadcast_to(w * (LD(1) / three) * fac[d] / D, shape), ax, 0)
            t = D * dterm if dim == 1 else dterm * D / area[d]
            t = np.moveaxis(np.broadcast_to(t, shape), ax, 0)
            n = a2.shape[0]
            diag = np.zeros((n + 1,) + a2.shape[1:], dtype=LD)
            diag[:-1] += a2; diag[1:] += a2
            if bc.get(_attr(dim, d, False)) == 0: diag[0] += t[0]
            if bc.get(_attr(dim, d, True)) == 0: diag[-1] += t[-1]
            self.lines.append((ax, diag, a1.copy()))

    def apply(self, x):
        x = np.asarray(x).astype(LD).reshape(self.shape)
        beta = self.beta
        cx = self.C * x
        y, s = cx.copy(), np.abs(cx)
        for ax, diag, off in self.lines:
            xm = np.moveaxis(x, ax, 0)
            n = xm.shape[0]
            t = np.zeros((n + 1,) + xm.shape[1:], dtype=LD)
            t[1:] += beta * xm; t[:-1] -= beta * xm               # B^T x: face f sees beta (x_{f-1} - x_f)
            u = thomas(diag, off, t)
            y += np.moveaxis(beta * (u[1:] - u[:-1]), 0, ax)
            s += np.moveaxis(beta * (np.abs(u[1:]) + np.abs(u[:-1])), 0, ax)
        return y.ravel(), s.ravel()

    def currents(self, x, diag=False):
        """The face currents of the field x -> (J, s), np.longdouble in the reference DOF order (x faces, y faces, z faces; each block the
        face array in C order with the line axis put back).  Full path: J = -u, A u = B^T x by the Thomas sweep, with the componentwise bound
        of a solve as the scale, s = |A^-1| (|A| |u| + |B^T| |x|): a line's matrix is a symmetric positive definite tridiagonal, so
        |A^-1| = M(A)^-1 with M(A) its comparison matrix (same diagonal, off-diagonals negated) -- one more Thomas sweep.  diag = True: the
        diagonal path's J_f = +(B^T x)_f / A_ff (src/NeutFEM.cpp:620-633) with s_f = beta (|x_f-1| + |x_f|) / A_ff"""
        x = np.asarray(x).astype(LD).reshape(self.shape)
        beta = self.beta
        Js, ss = [], []
        for ax, dg, off in self.lines:
            xm = np.moveaxis(x, ax, 0)
            n = xm.shape[0]
            t = np.zeros((n + 1,) + xm.shape[1:], dtype=LD); ta = np.zeros_like(t)
            t[1:] += beta * xm; t[:-1] -= beta * xm               # B^T x: face f sees beta (x_{f-1} - x_f)
            ta[1:] += beta * np.abs(xm); ta[:-1] += beta * np.abs(xm)
            if diag:
                J, s = t / dg, ta / dg
            else:
                u = thomas(dg, off, t)
                au = dg * np.abs(u)
                au[1:] += off * np.abs(u[:-1]); au[:-1] += off * np.abs(u[1:])
                J, s = -u, thomas(dg, -off, au + ta)
            Js.append(np.moveaxis(J, 0, ax).ravel()); ss.append(np.moveaxis(s, 0, ax).ravel())
        return np.concatenate(Js), np.concatenate(ss)


def exact_apply(inp, g, x):
    """(y, s) of group g: the apply and the per-component scale, np.longdouble"""
    return ExactApply(inp, g).apply(x)


def rho(y, y_exact, s):
    """max_i |y_i - y_exact,i| / s_i (a component whose scale is 0 has y_exact = 0 and must be matched exactly)"""
    d = np.abs(np.asarray(y).astype(LD).ravel() - y_exact)
    ok = s > 0
    if np.any(d[~ok] != 0):
        return float("inf")
    return float((d[ok] / s[ok]).max()) if ok.any() else 0.0


def normwise(y, y_ref):
    """the metric of the other operator-level tests: max |y - y_ref| / max |y_ref|"""
    y_ref = np.asarray(y_ref)
    return float(np.abs(np.asarray(y) - y_ref).max() / np.abs(y_ref).max())


def exact_cg2_op(apply, b):
    """two CG steps from x = 0 (src/solvers.cpp:577-636 with tol = 0, maxit = 2) in extended precision on any operator apply(x) -> (y, s):
    x2 = c b - a0 a1 S b, c = a0 + a1 (1 + b0).  Returns (x2, scale) with scale_i = |c| |b_i| + a0 a1 s_i(b)"""
    b = np.asarray(b).astype(LD).ravel()
    Sb, sb = apply(b)
    rr0 = (b * b).sum()
    a0 = rr0 / (b * Sb).sum()
    r1 = b - a0 * Sb
    rr1 = (r1 * r1).sum()
    b0 = rr1 / rr0
    p1 = r1 + b0 * b
    q1, _ = apply(p1)
    a1 = rr1 / (p1 * q1).sum()
    c = a0 + a1 * (LD(1) + b0)
    return a0 * b + a1 * p1, np.abs(c) * np.abs(b) + a0 * a1 * sb


def exact_cg2(inp, g, b):
    """exact_cg2_op on the closed-form RT0-P0 apply of group g"""
    return exact_cg2_op(ExactApply(inp, g).apply, b)


def f6_block_inputs(shape, block, seed=11, ng=2):
    """block_inputs of tests/test_gpu_line_dict.py at the benchmark's contrast: piecewise-constant cross-sections on blocks of `block`
    cells, widths exactly 1.25, a palette of four materials of which the last is IAEA-3D's filler (D = 1e-3, Sigma_R = 1e15, no fission,
    no scattering) -- drawn with p = (0.25, 0.25, 0.17, 0.33); the removal cross-section of the other three lies in 0.01 ... 0.13.
    shape = (nx, ny, nz) with block = (bx, by, bz), or the 2D form (nx, ny) with (bx, by): arrays (ng, ny, nx), z_breaks = [0.0], attributes
    1 ... 4 -- the same palette and the same draw."""
    dims = tuple(shape)[::-1]                                     # (nz, ny, nx), or (ny, nx) of a 2D mesh
    rng = np.random.default_rng(seed)
    npal = 4
    pal = dict(D=rng.uniform(0.3, 1.8, (ng, npal)), SigR=rng.uniform(0.01, 0.13, (ng, npal)), NSF=rng.uniform(0.0, 0.3, (ng, npal)),
               S=rng.uniform(0.005, 0.05, npal))
    pal["D"][:, 3] = F6_D; pal["SigR"][:, 3] = F6_SIGR; pal["NSF"][:, 3] = 0.0; pal["S"][3] = 0.0
    nb = [-(-n // b) for n, b in zip(dims, block[::-1])]
    mat = rng.choice(npal, size=nb, p=(0.25, 0.25, 0.17, 0.33))
    for ax, b in enumerate(block[::-1]):
        mat = np.repeat(mat, b, axis=ax)
    mat = mat[tuple(slice(0, n) for n in dims)]
    D, SigR, NSF = (np.stack([pal[k][g][mat] for g in range(ng)]) for k in ("D", "SigR", "NSF"))
    Chi = np.zeros((ng,) + mat.shape); Chi[0] = 0.8; Chi[1:2] = 0.2; Chi[:, mat == 3] = 0.0
    SigS = np.zeros((ng, ng) + mat.shape)
    if ng > 1: SigS[1, 0] = pal["S"][mat]
    brk = lambda n: 1.25 * np.arange(n + 1)
    nattr = 2 * len(dims)
    return dict(x_breaks=brk(dims[-1]), y_breaks=brk(dims[-2]), z_breaks=brk(dims[0]) if len(dims) == 3 else np.array([0.0]), D=D, SigR=SigR,
                NSF=NSF, Chi=Chi, SigS=SigS, bc_attr=np.arange(1, nattr + 1), bc_type=np.zeros(nattr, int), coarse_factors=np.array([1, 1, 1]),
                kref=1.0, ng=ng)


def f6_mask(inp, g=0):
    """cells of the filler material (flat, cell order)"""
    return (np.asarray(inp["SigR"])[g] >= 1e14).ravel()


def input_vector(n, g):
    """the input vector of the operator-level tests (tests/test_gpu_parity.py::_apply_case): normal, 10 % of the entries x 1e-12; the
    generator advances from group to group"""
    rng = np.random.default_rng(3)
    for _ in range(g + 1):
        x = rng.standard_normal(n); x[rng.random(n) < 0.1] *= 1e-12
    x.setflags(write=False)
    return x



# ---- higher orders: the scipy twin's operator with exact local tables --------------------------------------------------------------
def _legendre_ld(n, x):
    """(P_n(x), P_n'(x)) by the three-term recurrence, every operation in the precision of x (numpy's legval rounds its Clenshaw
    coefficients to double)"""
    x = np.asarray(x)
    p0, p1, d0, d1 = np.ones_like(x), x.copy(), np.zeros_like(x), np.ones_like(x)
    if n == 0:
        return p0, d0
    for k in range(1, n):
        p0, p1, d0, d1 = p1, ((2 * k + 1) * x * p1 - k * p0) / (k + 1), d1, ((2 * k + 1) * (p1 + x * d1) - k * d0) / (k + 1)
    return p1, d1


def gauss_legendre_ld(n):
    """n-point Gauss-Legendre rule in extended precision: numpy's double nodes polished by Newton steps on P_n, w = 2 / ((1 - x^2) P_n'(x)^2)"""
    from numpy.polynomial import legendre as npleg
    x = npleg.leggauss(n)[0].astype(LD)
    for _ in range(4):
        p, dp = _legendre_ld(n, x)
        x = x - p / dp
    return x, LD(2) / ((LD(1) - x * x) * _legendre_ld(n, x)[1] ** 2)


_ABS_INVERSE = {}                                                 # ExactTwin._abs_inverse: the block inverses of one twin at a time


class ExactTwin:
    """RT_k-P_m of any order: the operator oracle/ref_scipy.RefScipy assembles, in extended precision.

    The reference tabulates its 5-point Gauss rule to 15 digits (include/FEM.hpp:82-123; the weights are off by up to 1e-15 relative and sum
    to 2 - 1e-15), and the oracle and the twin keep those digits -- so for RT1 / RT2 the two agree with each other far better than either
    agrees with the operator itself, while the kernels use the closed forms of the condensed line blocks (2/15, 1/30, ...).  Here the local
    tables come from RefScipy._tables run on a rule that is exact to extended precision (basis, DOF numbering and index maps are the
    twin's: this is its operator, not a third assembly), the matrices are kept as extended-precision triplets, and A u = B^T x is solved
    by iterative refinement: the twin's SuperLU factors as the approximate inverse, residuals in extended precision.
    apply(g, x) -> (y, s, last relative correction), s = |C| |x| + |B| |u| the per-component scale."""

    def __init__(self, r):
        self.r = r
        import oracle.ref_scipy as twin
        qp, qw, P, dP = r.qp, r.qw, twin._P, twin._dP
        try:                                                      # the twin's own table code on an exact rule, with Legendre values in the precision of their argument
            r.qp, r.qw = gauss_legendre_ld(len(qp) + 2)
            twin._P, twin._dP = (lambda n, x: _legendre_ld(n, x)[0]), (lambda n, x: _legendre_ld(n, x)[1])
            r._tables()
            Ah, Bh, Ch = [np.asarray(a) for a in r.Ahat], np.asarray(r.Bhat), np.asarray(r.Chat)
        finally:
            r.qp, r.qw, twin._P, twin._dP = qp, qw, P, dP
            r._tables()
        assert all(a.dtype == LD for a in Ah) and Bh.dtype == LD and Ch.dtype == LD
        d, nper, nP = r.dim, r.nper, r.nloc
        hx, hy, hz = (np.asarray(h).astype(LD) for h in (r.hx, r.hy, r.hz))
        iz, iy, ix = np.meshgrid(np.arange(r.nz), np.arange(r.ny), np.arange(r.nx), indexing="ij")
        iz, iy, ix = iz.ravel(), iy.ravel(), ix.ravel()               # cell order e = (iz ny + iy) nx + ix
        HX, HY, HZ = hx[ix], hy[iy], hz[iz]
        if d == 1: fac, detJ, area = [HX / 2], HX / 2, [None]
        elif d == 2: fac, detJ, area = [HY / HX, HX / HY], HX * HY / 4, [HY * HZ, HX * HZ]
        else: fac, detJ, area = [2 * HX / (HY * HZ), 2 * HY / (HX * HZ), 2 * HZ / (HX * HY)], HX * HY * HZ / 8, [HY * HZ, HX * HZ, HX * HY]
        J = np.array([r._faces(int(a), int(b), int(c)) for a, b, c in zip(ix, iy, iz)])      # (cells, nJloc)
        self.Apat = []                                            # per direction: rows, cols, values without 1 / D, the cell of every entry
        for a in range(d):
            blk = J[:, a * nper:(a + 1) * nper]
            self.Apat.append((np.repeat(blk, nper, axis=1).ravel(), np.tile(blk, (1, nper)).ravel(),
                              (fac[a][:, None] * Ah[a].ravel()[None, :]).ravel(), np.repeat(np.arange(r.ne), nper * nper)))
        self.B = (np.repeat(np.arange(r.nPhi).reshape(r.ne, nP), r.nJloc, axis=1).ravel(), np.tile(J, (1, nP)).ravel(), np.tile(Bh.ravel(), r.ne))
        self.cd = (detJ[:, None] * np.diag(Ch)[None, :]).ravel()     # C diagonal without Sigma_R
        self.dirichlet = []                                       # (dof, value without D, cell)
        n_a = [r.nx, r.ny, r.nz]
        for a in range(d):
            for upper in (False, True):
                if r.bc.get(r._attr(a, upper)) != 0: continue
                on = np.flatnonzero([ix, iy, iz][a] == (n_a[a] - 1 if upper else 0))
                for f in range(r.nf):
                    if d == 1: I = np.ones(on.size, dtype=LD)
                    elif d == 2: I = LD(2) * (LD(2) / (2 * f + 1)) / area[a][on]
                    else: I = LD(4) * (LD(2) / (2 * (f % (r.k + 1)) + 1)) * (LD(2) / (2 * (f // (r.k + 1)) + 1)) / area[a][on]
                    self.dirichlet.append((J[on, a * nper + (r.nf if upper else 0) + f], 2 * I, on))

    @staticmethod
    def _mv(rows, cols, vals, v, n):
        out = np.zeros(n, dtype=LD)
        np.add.at(out, rows, vals * v[cols])
        return out

    def apply(self, g, x, sweeps=5):
        r = self.r
        D = np.asarray(r.D[g]).astype(LD)
        x = np.asarray(x).astype(LD)
        A = [(rows, cols, vals / D[cell]) for rows, cols, vals, cell in self.Apat] + [(dof, dof, val * D[cell]) for dof, val, cell in self.dirichlet]
        Au = lambda u: sum(self._mv(rows, cols, vals, u, r.nJ) for rows, cols, vals in A)
        br, bc, bv = self.B
        t = self._mv(bc, br, bv, x, r.nJ)                          # B^T x
        u = r.lu[g].solve(np.asarray(t, dtype=np.float64)).astype(LD)
        for _ in range(sweeps):
            du = r.lu[g].solve(np.asarray(t - Au(u), dtype=np.float64)).astype(LD)
            u = u + du
        cx = np.repeat(np.asarray(r.SigR[g]).astype(LD), r.nloc) * self.cd * x
        y = cx + self._mv(br, bc, bv, u, r.nPhi)
        s = np.abs(cx) + self._mv(br, bc, np.abs(bv), np.abs(u), r.nPhi)
        return y, s, float(np.abs(du).max() / np.abs(u).max())

    def currents(self, g, x, sweeps=5):
        """The currents of the field x of group g (host DOF order) -> (J, s, last relative correction): J = -u with A_g u = B^T x, in the
        twin's numbering (RefScipy._faces: x, y, z face DOFs, then x, y, z bubbles -- the reference's, and get_J's).

        Structural zeros are exact zeros: the twin's own drop rules (RefScipy.build: B-hat entries <= 1e-14, element entries of A <= 1e-13 x
        the largest) are applied to the extended-precision triplets.  Without them entries that vanish by orthogonality sit at 1e-17 ...
        1e-20, the RT modes that see no flux moment at P < RT get a reference of 1e-25 on a scale of 1e-28, and the metric means nothing
        there.  With them those DOFs have reference 0 and scale 0, and rho demands an exact match.

        Scale: a solve is backward stable, not componentwise forward accurate -- a tiny u_f beside large ones carries its neighbours'
        error -- so s = |A^-1| (|A| |u| + |B^T| |x|), the componentwise bound of the solve, in double.  A is block diagonal by line and
        transverse mode: |A^-1| block by block (_abs_inverse), never of the whole matrix"""
        r = self.r
        D = np.asarray(r.D[g]).astype(LD)
        x = np.asarray(x).astype(LD).ravel()
        A = [(rows, cols, vals / D[cell]) for rows, cols, vals, cell in self.Apat]
        vmax = max(float(np.abs(v).max()) for _, _, v in A)
        kept = [np.abs(v) > 1e-13 * vmax for _, _, v in A]
        A = [(rows[k], cols[k], v[k]) for (rows, cols, v), k in zip(A, kept)] + [(dof, dof, val * D[cell]) for dof, val, cell in self.dirichlet]
        Au = lambda u: sum(self._mv(rows, cols, vals, u, r.nJ) for rows, cols, vals in A)
        br, bc, bv = self.B
        keep = np.abs(bv) > 1e-14
        t = self._mv(bc[keep], br[keep], bv[keep], x, r.nJ)         # B^T x
        u = r.lu[g].solve(np.asarray(t, dtype=np.float64)).astype(LD)
        for _ in range(sweeps):
            du = r.lu[g].solve(np.asarray(t - Au(u), dtype=np.float64)).astype(LD)
            u = u + du
        ua, xa = np.abs(np.asarray(u, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64))
        rhs = abs(r.A[g]) @ ua + abs(r.BT) @ xa
        s = np.zeros(r.nJ)
        for dofs, inv in self._abs_inverse(g):
            s[dofs] = np.einsum("bij,bj->bi", inv, rhs[dofs])
        umax = np.abs(u).max()
        return -u, s.astype(LD), float(np.abs(du).max() / umax) if umax > 0 else 0.0

    def _abs_inverse(self, g):
        """|A_g^-1| as [(dofs (blocks, n), |inverse| (blocks, n, n)) for every block size n]: the connected components of the twin's A_g
        (one per line and transverse mode), inverted densely in double.  One twin's inverses are kept at a time"""
        if _ABS_INVERSE.get("owner") is not self:
            _ABS_INVERSE.clear(); _ABS_INVERSE["owner"] = self
        if g not in _ABS_INVERSE:
            from scipy.sparse.csgraph import connected_components
            A = self.r.A[g].tocoo()
            nblk, lab = connected_components(self.r.A[g], directed=False)
            sizes = np.bincount(lab, minlength=nblk)
            assert sizes.max() <= 512, sizes.max()                    # a line's faces and bubbles; anything larger is not a line
            order = np.argsort(lab, kind="stable")
            pos = np.empty(lab.size, dtype=np.int64)
            pos[order] = np.arange(lab.size) - np.repeat(np.cumsum(sizes) - sizes, sizes)
            out = []
            for n in np.unique(sizes):
                which = np.full(nblk, -1); which[sizes == n] = np.arange((sizes == n).sum())
                m = sizes[lab[A.row]] == n
                M = np.zeros((int((sizes == n).sum()), n, n))
                np.add.at(M, (which[lab[A.row[m]]], pos[A.row[m]], pos[A.col[m]]), A.data[m])
                dofs = np.empty(M.shape[:2], dtype=np.int64)
                sel = np.flatnonzero(sizes[lab] == n)
                dofs[which[lab[sel]], pos[sel]] = sel
                out.append((dofs, np.abs(np.linalg.inv(M))))
            _ABS_INVERSE[g] = out
        return _ABS_INVERSE[g]

    def operator(self, g, dus):
        """group g as apply(x) -> (y, s) for exact_cg2_op; the last relative correction of every apply is appended to dus"""
        def apply(x):
            y, s, du = self.apply(g, x)
            dus.append(du)
            return y, s
        return apply

    def outer(self, phi0=None):
        """One outer iteration of SolveKeff from the start flux (phi0 (ng, nPhi); None: 1 in every DOF; k = 1) with two CG steps per group, in extended precision:
        the right-hand sides as oracle/ref_scipy.py solve_keff states them -- tf = sum_g Mf_g phi_g, rhs = chi_g tf / k with chi / k below
        1e-14 set to 0 when a cell has more than one flux DOF, plus the Ms blocks in Gauss-Seidel order -- formed from this twin's own
        diagonals, never rounded to double.  Returns dict(b, y, s: per group; du: every apply's last relative correction)"""
        r = self.r
        ng, nloc = r.ng, r.nloc
        per_dof = lambda a: np.repeat(np.asarray(a).astype(LD), nloc)
        vol = np.einsum("k,j,i->kji", *(np.asarray(h).astype(LD) for h in (r.hz, r.hy, r.hx))).ravel()
        w = vol if r.m == 0 else self.cd                               # the mass diagonal without its cross-section (RefScipy.build)
        phi = [np.ones(r.nPhi, dtype=LD) if phi0 is None else np.asarray(phi0[g]).astype(LD).ravel() for g in range(ng)]
        tf = sum(per_dof(r.NSF[g]) * w * phi[g] for g in range(ng))
        k = LD(1)
        out = dict(b=[], y=[], s=[], du=[])
        for g in range(ng):
            chi = per_dof(r.Chi[g]) / k
            if nloc > 1:
                chi = np.where(np.abs(chi) < 1e-14, LD(0), chi)
            rhs = chi * tf
            for gp in range(ng):
                ms = per_dof(r.SigS[g, gp]) * w
                if gp != g and np.any(np.abs(ms) > 1e-14):
                    rhs = rhs + ms * phi[gp]
            x2, sc = exact_cg2_op(self.operator(g, out["du"]), rhs)
            phi[g] = x2
            out["b"].append(rhs); out["y"].append(x2); out["s"].append(sc)
        return out


def outer_rho(phi, ref):
    """SolveKeff returns the normalised iterate: one scalar is fitted on group 0 (phi_0 . y_0 / y_0 . y_0, in extended precision) and
    every group is then judged per component with it.  ref: y and s per group (ExactTwin.outer)"""
    ng = len(ref["y"])
    phi = np.asarray(phi).reshape(ng, -1).astype(LD)
    c = (phi[0] * ref["y"][0]).sum() / (ref["y"][0] * ref["y"][0]).sum()
    return [rho(phi[g] / c, ref["y"][g], ref["s"][g]) for g in range(ng)]


# ---- the orders with bubble moments at the benchmark's contrast: cases and references of tests/test_gpu_orders_exact.py ---------------
# name: (RT order, P order, shape, block).  a ... f cover NB = 1 and 2, 2D and 3D, P = RT and P < RT, even and odd nx; g is the even-nx RT2
# case (the scan variants' VEC follows nx parity); h has y and z lines shorter than 4 cells (one-sided lanes beside the two-sided x
# lanes); i is RT2-P0.  The flux carries NB = min(RT, P) bubble moments: the P0 cases e and i run the RT0-P0 instantiations on the line
# factors of their order.  All fit a line-per-lane variant (tests/test_apply_exact.py asks lane_plan).
ORDER_CASES = {
    "a": (1, 1, (20, 18), (4, 3)), "b": (2, 2, (21, 20), (3, 4)), "c": (1, 1, (8, 6, 5), (4, 3, 5)), "d": (2, 2, (5, 5, 4), (2, 3, 2)),
    "e": (1, 0, (20, 18), (4, 3)), "f": (2, 1, (8, 6, 5), (4, 3, 5)),
    "g": (2, 2, (4, 5, 5), (2, 3, 2)), "h": (1, 1, (9, 3, 2), (3, 1, 1)), "i": (2, 0, (8, 6, 5), (4, 3, 5)),
}
ORDER_BAR = 4                                                     # GPU rho <= 4 x the double oracle's own rho on the same case, group and quantity


_order_cache = {}


def order_case(name):
    """inputs, the built oracle factory's arguments and the exact twin of a case of ORDER_CASES, computed once"""
    if name not in _order_cache:
        from subcrit_exact import ref_from_inputs
        rt, p, shape, block = ORDER_CASES[name]
        inp = f6_block_inputs(shape, block)
        ex = ExactTwin(ref_from_inputs(inp, rt, p))
        _order_cache[name] = dict(name=name, rt=rt, p=p, shape=shape, inp=inp, ex=ex, nloc=ex.r.nloc, filler=np.repeat(f6_mask(inp), ex.r.nloc))
    return _order_cache[name]


def order_ref_cg(name):
    """per group: b = |input vector| off the filler and 0 on it (the mask is per cell, a cell has nloc flux DOFs), the exact two CG steps
    on the twin, their scale, the double oracle's own two steps and their rho.  Computed once, read-only"""
    c = order_case(name)
    if "cg" not in c:
        from helpers import make_oracle
        o = make_oracle(c["inp"], c["rt"], c["p"]); o.set_tol(1e-5, 0.0, 0.0, 200, 2)
        out = dict(inp=c["inp"], groups=tuple(range(int(c["inp"]["ng"]))), x={}, y={}, s={}, rho_o={}, its_o={}, du=[])
        for g in out["groups"]:
            b = np.abs(np.asarray(input_vector(o.n_phi, g))) * ~c["filler"]
            b.setflags(write=False)
            x2, sc = exact_cg2_op(c["ex"].operator(g, out["du"]), b)
            xo, _, its = o.solve_group(g, b, with_J=False)
            out["x"][g], out["y"][g], out["s"][g], out["rho_o"][g], out["its_o"][g] = b, x2, sc, rho(xo, x2, sc), its
        c["cg"] = out
    return c["cg"]


def order_start_flux(name, start):
    """the start flux of the one-outer runs, (ng, nPhi) in the host DOF layout or None.  "flat": SolveKeff's own, 1 in every DOF -- then the
    right-hand sides are equal in moments of equal mass, and an apply that confuses two such moments shows in the second CG step only,
    which enters x2 through the one scalar a1.  "rough": uniform in 0.5 ... 1.5 per DOF, so that the first apply of every group sees a vector
    without that symmetry"""
    if start == "flat":
        return None
    assert start == "rough", start
    r = order_case(name)["ex"].r
    phi0 = np.random.default_rng(7).uniform(0.5, 1.5, (r.ng, r.nPhi))
    phi0.setflags(write=False)
    return phi0


def order_ref_outer(name, start="flat"):
    """ExactTwin.outer of the case from order_start_flux with the double oracle's own one-outer SolveKeff from the same start judged by it
    under the same scalar fit"""
    c = order_case(name)
    key = "outer " + start
    if key not in c:
        from helpers import make_oracle
        phi0 = order_start_flux(name, start)
        out = c["ex"].outer(phi0)
        o = make_oracle(c["inp"], c["rt"], c["p"]); o.set_tol(0.0, 0.0, 0.0, 1, 2)
        if phi0 is not None:
            o.phi_dofs()[...] = phi0
        o.SolveKeff()
        h = o.history()
        out["n_outer_o"], out["cg_o"] = int(h["n_outer"]), np.asarray(h["cg"]).copy()
        out["rho_o"] = outer_rho(o.phi_dofs(), out)
        c[key] = out
    return c[key]


# ---- the reconstructed currents: cases, DOF classes and the oracle's own figures for tests/test_gpu_currents_exact.py ------------------
# RT0-P0 beside ORDER_CASES: R and T are shapes R and T of tests/test_gpu_apply_exact.py (the resident kernel's; the slab teams'), 2D is case a's mesh
P0_CASES = {"R": ((12, 11, 10), (4, 4, 5)), "2D": ((20, 18), (4, 3)), "T": ((16, 8, 96), (4, 4, 8))}
_p0_cache = {}


def rough_start(ng, nphi):
    """the rough start flux of order_start_flux for any input: uniform in 0.5 ... 1.5 per DOF, (ng, nphi), read-only"""
    phi0 = np.random.default_rng(7).uniform(0.5, 1.5, (ng, nphi))
    phi0.setflags(write=False)
    return phi0


def p0_case(name):
    """inputs and the closed-form operators of both groups of a case of P0_CASES, computed once"""
    if name not in _p0_cache:
        inp = f6_block_inputs(*P0_CASES[name])
        _p0_cache[name] = dict(name=name, rt=0, p=0, shape=P0_CASES[name][0], inp=inp, ea=[ExactApply(inp, g) for g in range(int(inp["ng"]))])
    return _p0_cache[name]


def current_classes(dims, rt, interfaces=()):
    """DOF class -> indices into one group's J (reference numbering): "x", "y", "z" faces and "bubbles"; the z faces on the planes listed
    in `interfaces` (the planes at which a slab team is cut) leave "z" for a class of their own, "z interface".  dims = (nx, ny[, nz])"""
    d = len(dims)
    nx, ny, nz = tuple(dims) + (1,) * (3 - d)
    k = min(rt, 2)
    nf, ni = (k + 1) ** (d - 1), k * (k + 1) ** (d - 1)
    n = [(nx + 1) * ny * nz * nf, nx * (ny + 1) * nz * nf if d >= 2 else 0, nx * ny * (nz + 1) * nf if d == 3 else 0]
    lo = np.concatenate([[0], np.cumsum(n)])
    out = {"xyz"[a]: np.arange(lo[a], lo[a + 1]) for a in range(d)}
    if interfaces:
        plane = (out["z"] - lo[2]) // (nx * ny * nf)
        cut = np.isin(plane, list(interfaces))
        out["z interface"], out["z"] = out["z"][cut], out["z"][~cut]
    if ni:
        out["bubbles"] = np.arange(lo[3], lo[3] + d * nx * ny * nz * ni)
    return out, int(lo[3] + d * nx * ny * nz * ni)


def exact_outer_p0(inp, phi0, diag=False):
    """RT0-P0: the raw iterate of one outer iteration of SolveKeff from phi0 (ng, cells) with k = 1, per group in extended precision, on the
    closed forms: the right-hand sides of ExactTwin.outer written with cell volumes, then two CG steps (exact_cg2) -- or, diag = True, the
    diagonal path's phi = rhs / (C + sum_faces beta^2 / A_ff) (src/NeutFEM.cpp:483-634)"""
    ng, cells = int(inp["ng"]), inp["D"][0].size
    V = np.einsum("k,j,i->kji", *(np.diff(inp[k]).astype(LD) if len(inp[k]) > 1 else np.ones(1, dtype=LD) for k in ("z_breaks", "y_breaks", "x_breaks"))).ravel()
    flat = lambda a, *lead: np.asarray(a, dtype=np.float64).reshape(*lead, cells).astype(LD)
    NSF, Chi, SigS = flat(inp["NSF"], ng), flat(inp["Chi"], ng), flat(inp["SigS"], ng, ng)
    phi = [np.asarray(phi0[g]).astype(LD).ravel() for g in range(ng)]
    tf = sum(NSF[g] * V * phi[g] for g in range(ng))
    for g in range(ng):
        rhs = Chi[g] * tf
        for gp in range(ng):
            if gp != g: rhs = rhs + SigS[g, gp] * V * phi[gp]
        if diag:
            ea = ExactApply(inp, g)
            S = ea.C.copy()
            for ax, dg, _ in ea.lines:
                S += np.moveaxis(ea.beta * ea.beta * (1 / dg[1:] + 1 / dg[:-1]), 0, ax)
            phi[g] = rhs / S.ravel()
        else:
            phi[g] = exact_cg2(inp, g, rhs)[0]
    return phi


def currents_reference(case, phi, diag=False):
    """per group (J, s) of the field phi (ng, n_phi: a solver's returned flux, doubles) on a case of order_case / p0_case / a dict with "ex"
    or "ea"; the refinement's last corrections are appended to case["du_J"]"""
    out = []
    for g in range(len(phi)):
        if "ea" in case:
            out.append(case["ea"][g].currents(phi[g], diag))
        else:
            J, s, du = case["ex"].currents(g, phi[g])
            case.setdefault("du_J", []).append(du)
            out.append((J, s))
    return out


def currents_fit(J, ref):
    """the one scalar of a normalised solve, fitted on the currents of group 0 in extended precision: J_0 = c J_ref,0"""
    J0 = np.asarray(J[0]).astype(LD)
    return (J0 * ref[0][0]).sum() / (ref[0][0] * ref[0][0]).sum()


def currents_rho(J, ref, classes, c=None):
    """class -> [rho of every group], J / c judged per component against ref = currents_reference(...); c = None: no scalar (the field is
    the one J was built from)"""
    out = {}
    for name, idx in classes.items():
        out[name] = []
        for g, (Jr, s) in enumerate(ref):
            Jg = np.asarray(J[g]).astype(LD)[idx]
            out[name].append(rho(Jg if c is None else Jg / c, Jr[idx], s[idx]))
    return out


def _case_of(family, name):
    return order_case(name) if family == "higher" else p0_case(name)


def currents_cg_oracle(family, name):
    """fit-free: the oracle's solve_group(g, b, with_J = True) with two CG steps on order_ref_cg's b returns phi and J of the same
    unnormalised field -- its J against the reference applied to its phi.  dict(J, ref, rho: class -> per group), computed once"""
    c = _case_of(family, name)
    if "J cg" not in c:
        from helpers import make_oracle
        o = make_oracle(c["inp"], c["rt"], c["p"]); o.set_tol(1e-5, 0.0, 0.0, 200, 2)
        filler = np.repeat(f6_mask(c["inp"]), o.n_phi // o.ne)
        phis, Js = [], []
        for g in range(int(c["inp"]["ng"])):
            b = np.abs(np.asarray(input_vector(o.n_phi, g))) * ~filler
            phi, J, its = o.solve_group(g, b, with_J=True)
            assert its == 2, (name, g, its)
            phis.append(phi); Js.append(J)
        ref = currents_reference(c, phis)
        classes, nJ = current_classes(c["shape"], c["rt"])
        assert nJ == o.n_J
        c["J cg"] = dict(J=Js, ref=ref, classes=classes, rho=currents_rho(Js, ref, classes))
    return c["J cg"]


def currents_outer_oracle(family, name):
    """the procedure of the GPU tests on the oracle: one outer iteration from the rough start with two CG steps per group (diagonal family: the
    diagonal path), phi_dofs() and J_dofs(), the reference applied to that phi, the scalar fitted on the currents of group 0.
    dict(rho: class -> per group, c, c_flux: the scalar of the flux against the exact outer, kappa, phi: the oracle's returned flux, y0: the exact raw iterate of group 0),
    computed once"""
    c = _case_of("higher" if family == "higher" else "p0", name)
    key = "J outer " + family
    if key not in c:
        from helpers import make_oracle
        diag = family == "diag"
        o = make_oracle(c["inp"], c["rt"], c["p"]); o.set_tol(0.0, 0.0, 0.0, 1, 2)
        phi0 = rough_start(o.ng, o.n_phi)
        o.phi_dofs()[...] = phi0
        o.SolveKeff(False, [], diag)
        h = o.history()
        assert int(h["n_outer"]) == 1 and (np.asarray(h["cg"]) == (0 if diag else 2)).all(), (name, h["n_outer"], h["cg"])
        phi, J = o.phi_dofs().copy(), o.J_dofs().copy()
        y0 = order_ref_outer(name, "rough")["y"][0] if family == "higher" else exact_outer_p0(c["inp"], phi0, diag)[0]
        c[key] = dict(currents_judge(c, phi, J, y0, diag), phi=phi, y0=y0)
    return c[key]


def currents_judge(case, phi, J, y0, diag=False, interfaces=()):
    """what every one-outer test of the currents does with a solver's (phi, J): the reference applied to phi, the scalar fitted on the currents
    of group 0, rho per class and group; beside them c_flux = phi_0 . y0 / y0 . y0 against the exact raw iterate y0 of group 0 (c c_flux = 1 up to
    rounding: a wrong global factor or sign is O(1)) and kappa = sum s |J_ref| / sum J_ref^2 on group 0, which bounds what the fit itself can add.
    rho_flux is the same judgement with 1 / c_flux for the scalar: a wrong class drags the least-squares c with it and so shows in every class
    of rho; rho_flux, whose scalar never saw J, says which class it was (printed by the tests, not asserted: its scalar carries the error of
    the flux iterate)"""
    ref = currents_reference(case, phi, diag)
    classes, nJ = current_classes(case["shape"], case["rt"], interfaces)
    assert np.asarray(J).shape == (len(ref), nJ), (np.asarray(J).shape, nJ)
    cJ = currents_fit(J, ref)
    p0 = np.asarray(phi[0]).astype(LD).ravel()
    c_flux = (p0 * y0).sum() / (y0 * y0).sum()
    kappa = float((ref[0][1] * np.abs(ref[0][0])).sum() / (ref[0][0] * ref[0][0]).sum())
    return dict(rho=currents_rho(J, ref, classes, cJ), rho_flux=currents_rho(J, ref, classes, 1 / c_flux), c=cJ, c_flux=c_flux, kappa=kappa,
                zero_scale=[int((s == 0).sum()) for _, s in ref], classes=classes)


CURRENT_FAMILIES = {"higher": list(ORDER_CASES), "p0": list(P0_CASES), "diag": list(P0_CASES)}


def currents_bar(family):
    """the bar of a family of tests/test_gpu_currents_exact.py: ORDER_BAR x the oracle's largest rho over the family's case table, groups and
    classes under the same procedure (currents_outer_oracle), floored at 2^-53.  Pooled over the table: the oracle's per-case figures
    scatter by a factor of three for one and the same algorithm, and a per-case bar would judge luck.  Returns (bar, the pool's maximum)"""
    worst = max(r for name in CURRENT_FAMILIES[family] for rs in currents_outer_oracle(family, name)["rho"].values() for r in rs)
    return ORDER_BAR * max(worst, EPS), worst
