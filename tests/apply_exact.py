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
