// The outer step of the power iteration (src/NeutFEM.cpp:1766-1802, ChebyshevAccel(15, 0.98) of src/solvers.cpp:664-756), written once
// for every loop that runs it: the host-driven loop of solve_keff_impl, k_outer_logic + k_normalize_fission (diagonal path), k_keff_xcd,
// k_resident_keff, and -- the Chebyshev part only -- nf_solve_adjoint ("The outer step").  Plain C++: no HIP headers and no device-only
// intrinsics, so that it can be built and run on its own (tests/host/outer_main.cpp).
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define NF_HD __host__ __device__
#else
#define NF_HD
#endif

// ---- ChebyshevAccel: the coefficient table and the schedule ---------------------------------------------------------------------------
constexpr int CHEB_NMAX = 15;            // restart length: steps 0 .. CHEB_NMAX - 1, then again from the stored iterate
constexpr double CHEB_SIGMA = 0.98;
// a_1, and for n >= 2 the coefficients as the three-term update takes them: a3[n] = (4/sigma) a_n, cb[n] = b_n.  Kernel argument structs
// hold one by value: the host forms it, every loop reads the same bits.
struct ChebTable { double ca1, a3[16], cb[16]; };
inline ChebTable cheb_table()
{
    const double sigma = CHEB_SIGMA, Gm = std::acosh(2. / sigma - 1.);
    ChebTable t = {};
    t.ca1 = 2. / (2. - sigma);
    for (int i = 2; i < CHEB_NMAX; ++i) {
        const double ca = std::cosh((i - 1) * Gm) / std::cosh(i * Gm);
        t.a3[i] = (4. / sigma) * ca; t.cb[i] = std::cosh((i - 2) * Gm) / std::cosh(i * Gm);
    }
    return t;
}
// mode 0: no acceleration, 1: store phi0, 2: phi1 = phi0 + a (phi - phi0), 3: three-term with a, b
struct ChebStep { int mode; double a, b; };
// The step of this outer iteration; `on` is the caller's own condition (from which outer it accelerates, and whether at all).
NF_HD inline ChebStep cheb_next(int &cheb_it, const ChebTable &t, bool on)
{
    ChebStep s = { 0, 0.0, 0.0 };
    if (!on) return s;
    if (cheb_it == CHEB_NMAX) cheb_it = 0;
    if (cheb_it == 0) s.mode = 1;
    else if (cheb_it == 1) { s.mode = 2; s.a = t.ca1; }
    else { s.mode = 3; s.a = t.a3[cheb_it]; s.b = t.cb[cheb_it]; }
    ++cheb_it;
    return s;
}
// phi[i] = Chebyshev(v / norm), v the loaded raw value: stores into pa / pb what the mode keeps and returns the new phi, which the caller
// stores.  After a mode-3 step the caller swaps pa and pb (pa <- old pb, pb <- new).
NF_HD inline double cheb_update(double v, bool do_norm, double norm, const ChebStep &s, double *pa, double *pb, long i)
{
    if (do_norm) v /= norm;
    if (s.mode == 1) pa[i] = v;
    else if (s.mode == 2) { const double a = pa[i]; v = a + s.a * (v - a); pb[i] = v; }
    else if (s.mode == 3) { const double a = pa[i], b = pb[i]; v = b + s.a * (v - b) + s.b * (b - a); pa[i] = v; }
    return v;
}

// ---- the scalars of an outer iteration (:1766-1779) -----------------------------------------------------------------------------------
// From the four sums prod_old = sum M_f phi, prod_new = sum M_f raw, nsq = |raw|^2, dsq = |raw - phi|^2.  keff is the value to go on
// with: the first outer reports its dk but keeps the start value (:1774).  !finite: the iteration diverged, the caller stops.
struct OuterStep { double keff, keff_new, dk, dphi, norm; bool do_norm, finite; };
NF_HD inline OuterStep outer_step(double keff, int it, double prod_old, double prod_new, double nsq, double dsq)
{
    OuterStep s;
    s.keff_new = keff * (prod_new / prod_old);
    s.dk = std::fabs(s.keff_new - keff);
    s.keff = it >= 1 ? s.keff_new : keff;
    s.dphi = std::sqrt(dsq / nsq); s.norm = std::sqrt(nsq);
    s.do_norm = s.norm > 1e-14;
    s.finite = std::isfinite(s.keff_new) && std::isfinite(s.dphi);
    return s;
}
// the stop test (:1799-1802)
NF_HD inline bool outer_converged(double dk, double dphi, double tol_keff, double tol_flux) { return dk < tol_keff && dphi < tol_flux; }
