// Stand-alone check of the bookkeeping behind the batched x_sol update of the fused CG (neutfem_amd/csrc/nf_xsol_ring.h): the rules are run
// on scalar stand-ins for the vectors, no device.  Meant to be built with -fsanitize=address,undefined as well as plainly; exits non-zero
// on a mismatch.
#include "../../neutfem_amd/csrc/nf_xsol_ring.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; fprintf(stderr, "FAIL M=%d n=%d pend=%d: ", M, n, pend); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return; } } while (0)

// A solve of n iterations.  pend = 1: it ended behind the |r|^2 reduction of iteration n-1 (converged, maxit); pend = 0: p.q broke down in
// iteration n, whose x pass had run.
static void run(int M, int n, int pend)
{
    std::vector<int> slot((size_t)M, -1);                        // which direction a slot holds
    std::vector<double> ring((size_t)M, 0.0);
    int ah_tag[NF_XSOL_RING_MAX]; double ah[NF_XSOL_RING_MAX];
    for (int i = 0; i < NF_XSOL_RING_MAX; ++i) { ah_tag[i] = -1; ah[i] = 0.0; }
    auto alpha_of = [](int j) { return 0.37 + 0.11 * j; };
    auto p_of = [](int j) { return 1.0 / (3.0 + j); };
    int applied = 0;                                             // alpha_j p_j is in x_sol for every j < applied
    double x = 0.125, want = 0.125;
    for (int j = 0; j < n; ++j) want = std::fma(alpha_of(j), p_of(j), want);
    auto apply = [&](const NfRingBatch &B, const char *who) -> bool {
        if (B.n < 0 || B.n > M) { fprintf(stderr, "%s: %d updates\n", who, B.n); return false; }
        for (int i = 0; i < B.n; ++i) {
            const NfRingUpdate u = B.u[i];
            if (u.slot < 0 || u.slot >= M || u.alpha < 0 || u.alpha >= NF_XSOL_RING_MAX) { fprintf(stderr, "%s: slot %d, alpha %d\n", who, u.slot, u.alpha); return false; }
            if (slot[(size_t)u.slot] != applied || ah_tag[u.alpha] != applied)
                { fprintf(stderr, "%s: update %d is due, slot %d holds p_%d, alpha entry %d holds alpha_%d\n", who, applied, u.slot, slot[(size_t)u.slot], u.alpha, ah_tag[u.alpha]); return false; }
            x = std::fma(ah[u.alpha], ring[(size_t)u.slot], x);
            ++applied;
        }
        return true;
    };
    const int lastx = pend ? n - 1 : n;
    for (int k = 0; k <= lastx; ++k) {
        const int rd = nf_ring_read(k, M), wr = nf_ring_write(k, M);
        CHECK(rd >= 0 && rd < M && wr >= 0 && wr < M, "x pass %d: slots %d -> %d", k, rd, wr);
        const NfRingBatch B = nf_ring_apply(k, M);
        if (k == 0) { CHECK(rd == 0 && wr == 0 && B.n == 0, "x pass 0 must find p_0 where the solve's start left it"); slot[0] = 0; ring[0] = p_of(0); }
        else {
            CHECK(slot[(size_t)rd] == k - 1, "x pass %d reads slot %d, which holds p_%d", k, rd, slot[(size_t)rd]);
            CHECK(B.n == 0 || (B.n == M && B.u[B.n - 1].slot == rd), "x pass %d: a batch of %d that does not end with the direction it reads", k, B.n);
            CHECK(apply(B, "x pass"), "x pass %d", k);
            CHECK(slot[(size_t)wr] < applied, "x pass %d overwrites slot %d: p_%d is still pending", k, wr, slot[(size_t)wr]);
            slot[(size_t)wr] = k; ring[(size_t)wr] = p_of(k);
        }
        if (k < n) {                                             // FIN_PAP of iteration k
            const int a = nf_ring_alpha(k);
            CHECK(a >= 0 && a < NF_XSOL_RING_MAX && ah_tag[a] < applied, "alpha_%d overwrites entry %d: alpha_%d is still pending", k, a, ah_tag[a]);
            ah_tag[a] = k; ah[a] = alpha_of(k);
        }
    }
    CHECK(apply(nf_ring_pending(n, pend, M), "flush"), "flush");
    CHECK(applied == n, "%d updates applied", applied);
    CHECK(std::memcmp(&x, &want, sizeof x) == 0, "x_sol = %.17g, the chain gives %.17g", x, want);
}

int main()
{
    int cases = 0;
    for (int M = 1; M <= NF_XSOL_RING_MAX; ++M)
        for (int n = 0; n <= 4 * M + 3; ++n)
            for (int pend = 0; pend <= 1; ++pend) { run(M, n, pend); ++cases; }
    {   // M = 1 is today's rule: every x pass after the first applies the one update it reads, in place; the flush applies the last one
        bool ok = true;
        for (int k = 1; k < 20; ++k) { const NfRingBatch B = nf_ring_apply(k, 1); ok = ok && nf_ring_read(k, 1) == 0 && nf_ring_write(k, 1) == 0 && B.n == 1 && B.u[0].slot == 0 && B.u[0].alpha == (k - 1) % 8; }
        ok = ok && nf_ring_pending(5, 1, 1).n == 1 && nf_ring_pending(5, 0, 1).n == 0 && nf_ring_pending(0, 1, 4).n == 0;
        if (!ok) { ++failures; fprintf(stderr, "FAIL M = 1 is not the in-place rule\n"); }
    }
    if (!failures) printf("ok   %d solves\n", cases);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
