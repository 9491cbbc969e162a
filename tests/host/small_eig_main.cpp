// Stand-alone driver of neutfem_amd/csrc/nf_small_eig.h (plain C++, no device): reads problems on stdin, prints the results.
//   eig n  a11 a12 ... ann      (row by row)  ->  "eig n rc" and, when rc == 0, one line "w wr wi" per eigenvalue, one line "v ..." per
//                                                  COLUMN of V, and "res r" = max_ij |A V - V Theta| with Theta the real block form
//   chol n g11 g12 ... gnn                    ->  "chol n rc" and, when rc == 0, one line "l ..." per ROW of L and "res r" = max |L L^T - G|,
//                                                  "orth r" = max |X^T G X - I| with X = L^-T
// Meant to be built with -fsanitize=address,undefined; tests/test_small_eig_host.py does that and compares with numpy.
#include "../../neutfem_amd/csrc/nf_small_eig.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    char what[16];
    int n;
    while (scanf("%15s %d", what, &n) == 2) {
        if (n < 0 || n > 64) { fprintf(stderr, "FAIL: bad n %d\n", n); return 2; }
        std::vector<double> row((size_t)n * n), A((size_t)n * n);
        for (auto &v : row) if (scanf("%lf", &v) != 1) { fprintf(stderr, "FAIL: short input\n"); return 2; }
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) A[(size_t)j * n + i] = row[(size_t)i * n + j];
        if (!strcmp(what, "eig")) {
            std::vector<double> wr(n + 1), wi(n + 1), V((size_t)n * n + 1);
            const int rc = nf::small_eig(n, A.data(), wr.data(), wi.data(), V.data());
            printf("eig %d %d\n", n, rc);
            if (rc != 0) continue;
            for (int j = 0; j < n; ++j) printf("w %.17g %.17g\n", wr[j], wi[j]);
            for (int j = 0; j < n; ++j) { printf("v"); for (int i = 0; i < n; ++i) printf(" %.17g", V[(size_t)j * n + i]); printf("\n"); }
            double res = 0.0;
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i) {
                    double av = 0.0;
                    for (int k = 0; k < n; ++k) av += A[(size_t)k * n + i] * V[(size_t)j * n + k];
                    double vt = wr[j] * V[(size_t)j * n + i];       // A (u + i w) = (a + i b)(u + i w): A u = a u - b w, A w = b u + a w
                    if (wi[j] > 0) vt -= wi[j] * V[(size_t)(j + 1) * n + i];
                    if (wi[j] < 0) vt -= wi[j] * V[(size_t)(j - 1) * n + i];
                    res = std::max(res, std::fabs(av - vt));
                }
            printf("res %.3e\n", res);
        } else if (!strcmp(what, "chol")) {
            std::vector<double> L((size_t)n * n + 1), X((size_t)n * n + 1);
            const int rc = nf::small_cholesky(n, A.data(), L.data());
            printf("chol %d %d\n", n, rc);
            if (rc != 0) continue;
            nf::small_inv_lt(n, L.data(), X.data());
            double res = 0.0, orth = 0.0;
            for (int i = 0; i < n; ++i) { printf("l"); for (int j = 0; j < n; ++j) printf(" %.17g", L[(size_t)j * n + i]); printf("\n"); }
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    double v = 0.0, o = 0.0;
                    for (int k = 0; k < n; ++k) v += L[(size_t)k * n + i] * L[(size_t)k * n + j];
                    res = std::max(res, std::fabs(v - A[(size_t)j * n + i]));
                    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) o += X[(size_t)i * n + a] * A[(size_t)b * n + a] * X[(size_t)j * n + b];
                    orth = std::max(orth, std::fabs(o - (i == j ? 1.0 : 0.0)));
                }
            printf("res %.3e\north %.3e\n", res, orth);
        } else { fprintf(stderr, "FAIL: unknown problem %s\n", what); return 2; }
    }
    return 0;
}
