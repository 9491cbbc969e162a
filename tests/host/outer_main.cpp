// Stand-alone check of the outer step of the power iteration (neutfem_amd/csrc/nf_outer.h): the Chebyshev schedule and its coefficients,
// the scalar rule and the stop test, against values written out here by hand.  No device.  Meant to be built with
// -fsanitize=address,undefined as well as plainly; exits non-zero on a mismatch.
#include "../../neutfem_amd/csrc/nf_outer.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAIL " __VA_ARGS__); fputc('\n', stderr); } } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool within_1ulp(double a, double b) { return a == b || std::nextafter(a, b) == b; }

int main()
{
    const ChebTable t = cheb_table();

    // the schedule over 40 accelerated steps: store, two-term, thirteen three-term steps, and again
    {
        static const int WANT[40] = { 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3,
                                      1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3,
                                      1, 2, 3, 3, 3, 3, 3, 3, 3, 3 };
        int cheb_it = 0;
        for (int n = 0; n < 40; ++n) {
            const ChebStep s = cheb_next(cheb_it, t, true);
            CHECK(s.mode == WANT[n], "schedule: step %d has mode %d, not %d", n, s.mode, WANT[n]);
        }
        CHECK(cheb_it == 10, "schedule: the counter stands at %d after 40 steps, not 10", cheb_it);
        printf("ok schedule\n");
    }
    // the coefficients of steps 1, 2, 14 and 16 (the second step of the second round)
    {
        int cheb_it = 0; ChebStep at[17];
        for (int n = 0; n < 17; ++n) at[n] = cheb_next(cheb_it, t, true);
        CHECK(at[0].mode == 1 && at[0].a == 0.0 && at[0].b == 0.0, "step 0 carries coefficients");
        CHECK(at[1].mode == 2 && same_bits(at[1].a, t.ca1) && at[1].b == 0.0, "step 1: a = %.17g, not a_1 = %.17g", at[1].a, t.ca1);
        CHECK(at[2].mode == 3 && same_bits(at[2].a, t.a3[2]) && same_bits(at[2].b, t.cb[2]), "step 2: (%.17g, %.17g)", at[2].a, at[2].b);
        CHECK(at[14].mode == 3 && same_bits(at[14].a, t.a3[14]) && same_bits(at[14].b, t.cb[14]), "step 14: (%.17g, %.17g)", at[14].a, at[14].b);
        CHECK(at[15].mode == 1, "step 15 does not restart");
        CHECK(at[16].mode == 2 && same_bits(at[16].a, t.ca1) && at[16].b == 0.0, "step 16: a = %.17g, not a_1", at[16].a);
        printf("ok coefficients\n");
    }
    // on = false: mode 0, and the counter stays where it is
    {
        int cheb_it = 7;
        const ChebStep s = cheb_next(cheb_it, t, false);
        CHECK(s.mode == 0 && s.a == 0.0 && s.b == 0.0 && cheb_it == 7, "on = false: mode %d, counter %d", s.mode, cheb_it);
        cheb_it = 15;
        (void)cheb_next(cheb_it, t, false);
        CHECK(cheb_it == 15, "on = false wrapped the counter");
        printf("ok off\n");
    }
    // the table against ChebyshevAccel(15, 0.98): a_1 = 2 / (2 - sigma), a_n = cosh((n-1) G) / cosh(n G), b_n = cosh((n-2) G) / cosh(n G),
    // G = acosh(2 / sigma - 1); the table holds (4 / sigma) a_n
    {
        const double sigma = 0.98, G = std::acosh(2.0 / 0.98 - 1.0);
        CHECK(within_1ulp(t.ca1, 2.0 / 1.02), "a_1 = %.17g", t.ca1);
        CHECK(t.a3[0] == 0.0 && t.a3[1] == 0.0 && t.a3[15] == 0.0 && t.cb[0] == 0.0 && t.cb[1] == 0.0 && t.cb[15] == 0.0, "unused entries are not 0");
        for (int n = 2; n < 15; ++n) {
            const double a = std::cosh((n - 1) * G) / std::cosh(n * G), b = std::cosh((n - 2) * G) / std::cosh(n * G);
            CHECK(within_1ulp(t.a3[n], 4.0 / sigma * a), "a3[%d] = %.17g, formula %.17g", n, t.a3[n], 4.0 / sigma * a);
            CHECK(within_1ulp(t.cb[n], b), "cb[%d] = %.17g, formula %.17g", n, t.cb[n], b);
            CHECK(t.cb[n] > 0.0 && t.cb[n] < 1.0 && t.a3[n] > 0.0, "coefficients of step %d out of range", n);
        }
        printf("ok table\n");
    }
    // the scalar rule: keff_new = keff * prod_new / prod_old, dk = |keff_new - keff|, dphi = sqrt(dsq / nsq), norm = sqrt(nsq)
    {
        OuterStep s = outer_step(1.0, 0, 2.0, 2.5, 16.0, 4.0);      // the first outer reports dk and keeps the start value
        CHECK(s.keff == 1.0 && s.keff_new == 1.25 && s.dk == 0.25 && s.dphi == 0.5 && s.norm == 4.0 && s.do_norm && s.finite,
              "it = 0: keff %.17g keff_new %.17g dk %.17g dphi %.17g norm %.17g", s.keff, s.keff_new, s.dk, s.dphi, s.norm);
        s = outer_step(1.0, 1, 2.0, 2.5, 16.0, 4.0);                // from the second on keff_new is taken
        CHECK(s.keff == 1.25 && s.keff_new == 1.25 && s.dk == 0.25, "it = 1: keff %.17g dk %.17g", s.keff, s.dk);
        s = outer_step(0.5, 7, 4.0, 3.0, 0.25, 0.0625);
        CHECK(s.keff == 0.375 && s.dk == 0.125 && s.dphi == 0.5 && s.norm == 0.5 && s.do_norm && s.finite, "it = 7: keff %.17g dk %.17g", s.keff, s.dk);
        s = outer_step(1.0, 3, 2.0, 2.5, 0.0, 4.0);                 // nsq = 0: dphi = inf
        CHECK(!s.finite && !s.do_norm, "nsq = 0 counts as finite");
        s = outer_step(1.0, 3, 2.0, 2.5, 0.0, 0.0);                 // 0 / 0
        CHECK(!s.finite, "nsq = dsq = 0 counts as finite");
        s = outer_step(1.0, 3, 0.0, 2.5, 16.0, 4.0);                // prod_old = 0: keff_new = inf
        CHECK(!s.finite, "prod_old = 0 counts as finite");
        s = outer_step(1.0, 3, 2.0, std::numeric_limits<double>::quiet_NaN(), 16.0, 4.0);
        CHECK(!s.finite, "a NaN sum counts as finite");
        s = outer_step(1.0, 3, 2.0, 2.5, 2.5e-29, 1e-30);           // norm = 5e-15: not above 1e-14
        CHECK(s.finite && !s.do_norm && s.norm <= 1e-14, "norm %.17g: do_norm set", s.norm);
        s = outer_step(1.0, 3, 2.0, 2.5, 4e-28, 1e-30);             // norm = 2e-14
        CHECK(s.finite && s.do_norm, "norm %.17g: do_norm clear", s.norm);
        printf("ok outer_step\n");
    }
    // the stop test: both strictly below their tolerance
    {
        CHECK(outer_converged(0.9e-6, 0.9e-5, 1e-6, 1e-5), "both below: not converged");
        CHECK(!outer_converged(1e-6, 0.9e-5, 1e-6, 1e-5), "dk at its tolerance: converged");
        CHECK(!outer_converged(1.1e-6, 0.9e-5, 1e-6, 1e-5), "dk above: converged");
        CHECK(!outer_converged(0.9e-6, 1e-5, 1e-6, 1e-5), "dphi at its tolerance: converged");
        CHECK(!outer_converged(0.9e-6, 1.1e-5, 1e-6, 1e-5), "dphi above: converged");
        CHECK(!outer_converged(0.0, 0.0, 0.0, 1e-5) && !outer_converged(0.0, 0.0, 1e-6, 0.0), "a tolerance of 0 never stops");
        printf("ok stop\n");
    }
    // the element update, one entry per mode
    {
        double pa[2] = { 0.0, 0.0 }, pb[2] = { 0.0, 0.0 };
        const ChebStep m0 = { 0, 0.0, 0.0 }, m1 = { 1, 0.0, 0.0 }, m2 = { 2, 1.5, 0.0 }, m3 = { 3, 2.0, 0.5 };
        CHECK(cheb_update(6.0, true, 2.0, m0, pa, pb, 1) == 3.0 && pa[1] == 0.0 && pb[1] == 0.0, "mode 0");
        CHECK(cheb_update(6.0, false, 2.0, m0, pa, pb, 1) == 6.0, "mode 0 without the norm");
        CHECK(cheb_update(6.0, true, 2.0, m1, pa, pb, 1) == 3.0 && pa[1] == 3.0 && pb[1] == 0.0, "mode 1");
        CHECK(cheb_update(10.0, true, 2.0, m2, pa, pb, 1) == 6.0 && pa[1] == 3.0 && pb[1] == 6.0, "mode 2: 3 + 1.5 (5 - 3)");
        CHECK(cheb_update(14.0, true, 2.0, m3, pa, pb, 1) == 9.5 && pa[1] == 9.5 && pb[1] == 6.0, "mode 3: 6 + 2 (7 - 6) + 0.5 (6 - 3)");
        CHECK(pa[0] == 0.0 && pb[0] == 0.0, "the update touched another entry");
        printf("ok update\n");
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    return 0;
}
