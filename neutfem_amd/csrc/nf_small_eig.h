// nf_small_eig.h -- host-only dense algebra on the small matrices of the block outer iteration (nf_solve_modes):
// the eigen-decomposition of a real nonsymmetric n x n matrix, n <= 8, and the Cholesky factor of a Gram matrix.  No HIP, no LAPACK:
// plain C++ so that it can be compiled and checked on its own (tests/host/small_eig_main.cpp).
//
// small_eig: Householder reduction to Hessenberg form, the Francis double-shift QR iteration on it with the transformations accumulated,
// and back-substitution for the eigenvectors of the quasi-triangular form (the classical EISPACK orthes / hqr2 pair).  A complex pair
// is NOT split: it is reported as wi != 0 on two neighbouring entries and its two columns of V hold the real and the imaginary part of
// the eigenvector, a real basis of the pair's invariant plane.  A repeated eigenvalue with a full eigenspace gives independent columns
// (a zero pivot of the back-substitution is replaced by eps * norm, which leaves the earlier components 0).
#ifndef NF_SMALL_EIG_H
#define NF_SMALL_EIG_H
#include <algorithm>
#include <cmath>

namespace nf {

static const int SMALL_EIG_MAX = 8;

namespace small_eig_detail {
inline void cdiv(double xr, double xi, double yr, double yi, double *cr, double *ci)
{
    double r, d;
    if (std::fabs(yr) > std::fabs(yi)) { r = yi / yr; d = yr + r * yi; *cr = (xr + r * xi) / d; *ci = (xi - r * xr) / d; }
    else { r = yr / yi; d = yi + r * yr; *cr = (r * xr + xi) / d; *ci = (r * xi - xr) / d; }
}
}

// A: n x n, column-major, leading dimension n (not modified).  Out: wr / wi = real and imaginary parts of the eigenvalues ordered by
// descending real part (the two members of a complex pair stay neighbours, wi > 0 first), V = n x n column-major, column j the
// eigenvector of eigenvalue j scaled to unit 2-norm (complex pair at j, j + 1: column j the real part, column j + 1 the imaginary part,
// scaled together).  Returns 0, -1 for a bad n or a non-finite entry, -2 when the QR iteration does not converge.
inline int small_eig(int nn, const double *A, double *wr, double *wi, double *Vout)
{
    using small_eig_detail::cdiv;
    const int NM = SMALL_EIG_MAX;
    if (nn < 1 || nn > NM) return -1;
    double H[NM][NM], V[NM][NM], ort[NM], d[NM], e[NM];
    for (int i = 0; i < nn; ++i)
        for (int j = 0; j < nn; ++j) { H[i][j] = A[j * nn + i]; V[i][j] = i == j ? 1.0 : 0.0; if (!std::isfinite(H[i][j])) return -1; }
    const int low = 0, high = nn - 1;
    // ---- Householder reduction to Hessenberg form, transformations accumulated in V
    for (int m = low + 1; m <= high - 1; ++m) {
        double scale = 0.0;
        for (int i = m; i <= high; ++i) scale += std::fabs(H[i][m - 1]);
        if (scale == 0.0) { ort[m] = 0.0; continue; }
        double h = 0.0;
        for (int i = high; i >= m; --i) { ort[i] = H[i][m - 1] / scale; h += ort[i] * ort[i]; }
        double g = std::sqrt(h);
        if (ort[m] > 0) g = -g;
        h -= ort[m] * g; ort[m] -= g;
        for (int j = m; j < nn; ++j) {
            double f = 0.0;
            for (int i = high; i >= m; --i) f += ort[i] * H[i][j];
            f /= h;
            for (int i = m; i <= high; ++i) H[i][j] -= f * ort[i];
        }
        for (int i = 0; i <= high; ++i) {
            double f = 0.0;
            for (int j = high; j >= m; --j) f += ort[j] * H[i][j];
            f /= h;
            for (int j = m; j <= high; ++j) H[i][j] -= f * ort[j];
        }
        ort[m] *= scale;
        H[m][m - 1] = scale * g;
    }
    // column m - 1 still holds the unscaled tail of step m's vector below the subdiagonal, ort[m] its head
    for (int m = high - 1; m >= low + 1; --m) {
        if (H[m][m - 1] == 0.0 || ort[m] == 0.0) continue;
        for (int i = m + 1; i <= high; ++i) ort[i] = H[i][m - 1];
        for (int j = m; j <= high; ++j) {
            double g = 0.0;
            for (int i = m; i <= high; ++i) g += ort[i] * V[i][j];
            g = (g / ort[m]) / H[m][m - 1];
            for (int i = m; i <= high; ++i) V[i][j] += g * ort[i];
        }
    }
    for (int m = low + 1; m <= high - 1; ++m) for (int i = m + 1; i <= high; ++i) H[i][m - 1] = 0.0;
    // ---- Francis double-shift QR on the Hessenberg matrix
    int n = nn - 1;
    const double eps = std::ldexp(1.0, -52);
    double exshift = 0.0, p = 0, q = 0, r = 0, s = 0, z = 0, t, w, x, y;
    double norm = 0.0;
    for (int i = 0; i < nn; ++i) for (int j = std::max(i - 1, 0); j < nn; ++j) norm += std::fabs(H[i][j]);
    int iter = 0, total = 0;
    while (n >= low) {
        int l = n;
        while (l > low) {
            s = std::fabs(H[l - 1][l - 1]) + std::fabs(H[l][l]);
            if (s == 0.0) s = norm;
            if (std::fabs(H[l][l - 1]) < eps * s) break;
            --l;
        }
        if (l == n) {                                             // one root
            H[n][n] += exshift; d[n] = H[n][n]; e[n] = 0.0; --n; iter = 0;
        } else if (l == n - 1) {                                  // two roots
            w = H[n][n - 1] * H[n - 1][n];
            p = (H[n - 1][n - 1] - H[n][n]) / 2.0; q = p * p + w; z = std::sqrt(std::fabs(q));
            H[n][n] += exshift; H[n - 1][n - 1] += exshift; x = H[n][n];
            if (q >= 0) {                                         // a real pair
                z = p >= 0 ? p + z : p - z;
                d[n - 1] = x + z; d[n] = d[n - 1];
                if (z != 0.0) d[n] = x - w / z;
                e[n - 1] = 0.0; e[n] = 0.0;
                x = H[n][n - 1]; s = std::fabs(x) + std::fabs(z); p = x / s; q = z / s; r = std::sqrt(p * p + q * q); p /= r; q /= r;
                for (int j = n - 1; j < nn; ++j) { z = H[n - 1][j]; H[n - 1][j] = q * z + p * H[n][j]; H[n][j] = q * H[n][j] - p * z; }
                for (int i = 0; i <= n; ++i) { z = H[i][n - 1]; H[i][n - 1] = q * z + p * H[i][n]; H[i][n] = q * H[i][n] - p * z; }
                for (int i = low; i <= high; ++i) { z = V[i][n - 1]; V[i][n - 1] = q * z + p * V[i][n]; V[i][n] = q * V[i][n] - p * z; }
            } else { d[n - 1] = x + p; d[n] = x + p; e[n - 1] = z; e[n] = -z; }   // a complex pair
            n -= 2; iter = 0;
        } else {
            x = H[n][n]; y = 0.0; w = 0.0;
            if (l < n) { y = H[n - 1][n - 1]; w = H[n][n - 1] * H[n - 1][n]; }
            if (iter == 10) {                                     // Wilkinson's ad hoc shift
                exshift += x;
                for (int i = low; i <= n; ++i) H[i][i] -= x;
                s = std::fabs(H[n][n - 1]) + std::fabs(H[n - 1][n - 2]);
                x = y = 0.75 * s; w = -0.4375 * s * s;
            }
            if (iter == 30) {                                     // a second ad hoc shift
                s = (y - x) / 2.0; s = s * s + w;
                if (s > 0) {
                    s = std::sqrt(s); if (y < x) s = -s;
                    s = x - w / ((y - x) / 2.0 + s);
                    for (int i = low; i <= n; ++i) H[i][i] -= s;
                    exshift += s; x = y = w = 0.964;
                }
            }
            ++iter;
            if (++total > 60 * nn) return -2;
            int m = n - 2;
            while (m >= l) {                                      // two consecutive small subdiagonal elements
                z = H[m][m]; r = x - z; s = y - z;
                p = (r * s - w) / H[m + 1][m] + H[m][m + 1];
                q = H[m + 1][m + 1] - z - r - s;
                r = H[m + 2][m + 1];
                s = std::fabs(p) + std::fabs(q) + std::fabs(r);
                p /= s; q /= s; r /= s;
                if (m == l) break;
                if (std::fabs(H[m][m - 1]) * (std::fabs(q) + std::fabs(r)) <
                    eps * (std::fabs(p) * (std::fabs(H[m - 1][m - 1]) + std::fabs(z) + std::fabs(H[m + 1][m + 1])))) break;
                --m;
            }
            for (int i = m + 2; i <= n; ++i) { H[i][i - 2] = 0.0; if (i > m + 2) H[i][i - 3] = 0.0; }
            for (int k = m; k <= n - 1; ++k) {                    // the double QR step on rows l..n, columns m..n
                const bool notlast = k != n - 1;
                if (k != m) {
                    p = H[k][k - 1]; q = H[k + 1][k - 1]; r = notlast ? H[k + 2][k - 1] : 0.0;
                    x = std::fabs(p) + std::fabs(q) + std::fabs(r);
                    if (x == 0.0) break;
                    p /= x; q /= x; r /= x;
                }
                s = std::sqrt(p * p + q * q + r * r);
                if (p < 0) s = -s;
                if (s == 0.0) continue;
                if (k != m) H[k][k - 1] = -s * x;
                else if (l != m) H[k][k - 1] = -H[k][k - 1];
                p += s; x = p / s; y = q / s; z = r / s; q /= p; r /= p;
                for (int j = k; j < nn; ++j) {
                    p = H[k][j] + q * H[k + 1][j];
                    if (notlast) { p += r * H[k + 2][j]; H[k + 2][j] -= p * z; }
                    H[k][j] -= p * x; H[k + 1][j] -= p * y;
                }
                for (int i = 0; i <= std::min(n, k + 3); ++i) {
                    p = x * H[i][k] + y * H[i][k + 1];
                    if (notlast) { p += z * H[i][k + 2]; H[i][k + 2] -= p * r; }
                    H[i][k] -= p; H[i][k + 1] -= p * q;
                }
                for (int i = low; i <= high; ++i) {
                    p = x * V[i][k] + y * V[i][k + 1];
                    if (notlast) { p += z * V[i][k + 2]; V[i][k + 2] -= p * r; }
                    V[i][k] -= p; V[i][k + 1] -= p * q;
                }
            }
        }
    }
    // ---- eigenvectors of the quasi-triangular form by back-substitution, then back to the original basis
    if (norm != 0.0) {
        for (n = nn - 1; n >= 0; --n) {
            p = d[n]; q = e[n];
            if (q == 0.0) {                                       // a real vector
                int l = n;
                H[n][n] = 1.0;
                for (int i = n - 1; i >= 0; --i) {
                    w = H[i][i] - p; r = 0.0;
                    for (int j = l; j <= n; ++j) r += H[i][j] * H[j][n];
                    if (e[i] < 0.0) { z = w; s = r; }
                    else {
                        l = i;
                        if (e[i] == 0.0) H[i][n] = w != 0.0 ? -r / w : -r / (eps * norm);
                        else {                                    // a 2 x 2 block above: two real equations
                            x = H[i][i + 1]; y = H[i + 1][i];
                            q = (d[i] - p) * (d[i] - p) + e[i] * e[i];
                            t = (x * s - z * r) / q;
                            H[i][n] = t;
                            H[i + 1][n] = std::fabs(x) > std::fabs(z) ? (-r - w * t) / x : (-s - y * t) / z;
                        }
                        t = std::fabs(H[i][n]);
                        if ((eps * t) * t > 1) for (int j = i; j <= n; ++j) H[j][n] /= t;
                    }
                }
            } else if (q < 0) {                                   // a complex vector: columns n - 1 (real part) and n (imaginary part)
                int l = n - 1;
                if (std::fabs(H[n][n - 1]) > std::fabs(H[n - 1][n])) { H[n - 1][n - 1] = q / H[n][n - 1]; H[n - 1][n] = -(H[n][n] - p) / H[n][n - 1]; }
                else cdiv(0.0, -H[n - 1][n], H[n - 1][n - 1] - p, q, &H[n - 1][n - 1], &H[n - 1][n]);
                H[n][n - 1] = 0.0; H[n][n] = 1.0;
                for (int i = n - 2; i >= 0; --i) {
                    double ra = 0.0, sa = 0.0, vr, vi;
                    for (int j = l; j <= n; ++j) { ra += H[i][j] * H[j][n - 1]; sa += H[i][j] * H[j][n]; }
                    w = H[i][i] - p;
                    if (e[i] < 0.0) { z = w; r = ra; s = sa; }
                    else {
                        l = i;
                        if (e[i] == 0.0) cdiv(-ra, -sa, w, q, &H[i][n - 1], &H[i][n]);
                        else {
                            x = H[i][i + 1]; y = H[i + 1][i];
                            vr = (d[i] - p) * (d[i] - p) + e[i] * e[i] - q * q; vi = (d[i] - p) * 2.0 * q;
                            if (vr == 0.0 && vi == 0.0) vr = eps * norm * (std::fabs(w) + std::fabs(q) + std::fabs(x) + std::fabs(y) + std::fabs(z));
                            cdiv(x * r - z * ra + q * sa, x * s - z * sa - q * ra, vr, vi, &H[i][n - 1], &H[i][n]);
                            if (std::fabs(x) > std::fabs(z) + std::fabs(q)) {
                                H[i + 1][n - 1] = (-ra - w * H[i][n - 1] + q * H[i][n]) / x;
                                H[i + 1][n] = (-sa - w * H[i][n] - q * H[i][n - 1]) / x;
                            } else cdiv(-r - y * H[i][n - 1], -s - y * H[i][n], z, q, &H[i + 1][n - 1], &H[i + 1][n]);
                        }
                        t = std::max(std::fabs(H[i][n - 1]), std::fabs(H[i][n]));
                        if ((eps * t) * t > 1) for (int j = i; j <= n; ++j) { H[j][n - 1] /= t; H[j][n] /= t; }
                    }
                }
            }
        }
        for (int j = nn - 1; j >= low; --j)
            for (int i = low; i <= high; ++i) {
                z = 0.0;
                for (int k = low; k <= std::min(j, high); ++k) z += V[i][k] * H[k][j];
                V[i][j] = z;
            }
    }
    // ---- order by descending real part (stable: a pair stays together), unit columns
    int idx[NM];
    for (int i = 0; i < nn; ++i) idx[i] = i;
    std::stable_sort(idx, idx + nn, [&](int a, int b) { return d[a] > d[b]; });
    for (int c = 0; c < nn; ++c) {
        const int j = idx[c];
        wr[c] = d[j]; wi[c] = e[j];
        double s2 = 0.0;
        if (e[j] == 0.0) for (int i = 0; i < nn; ++i) s2 += V[i][j] * V[i][j];
        else { const int ja = e[j] > 0 ? j : j - 1; for (int i = 0; i < nn; ++i) s2 += V[i][ja] * V[i][ja] + V[i][ja + 1] * V[i][ja + 1]; }
        const double sc = s2 > 0.0 ? 1.0 / std::sqrt(s2) : 1.0;
        for (int i = 0; i < nn; ++i) Vout[c * nn + i] = V[i][j] * sc;
    }
    return 0;
}

// Cholesky factor of the symmetric positive definite n x n matrix G (column-major, the lower triangle is read): L (column-major, lower,
// the strict upper triangle set to 0) with G = L L^T.  Returns 0, or -(j + 1) when pivot j is not positive (or not finite): the matrix
// has lost rank there and L is not valid.
inline int small_cholesky(int n, const double *G, double *L)
{
    if (n < 1 || n > SMALL_EIG_MAX) return -(SMALL_EIG_MAX + 1);
    for (int i = 0; i < n * n; ++i) L[i] = 0.0;
    for (int j = 0; j < n; ++j) {
        double dj = G[j * n + j];
        for (int k = 0; k < j; ++k) dj -= L[k * n + j] * L[k * n + j];
        // a pivot that rounding alone can produce from the diagonal entry is no pivot
        if (!(dj > 0.0) || !std::isfinite(dj) || !(dj > 1e-14 * std::fabs(G[j * n + j]))) return -(j + 1);
        const double ljj = std::sqrt(dj);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double v = G[j * n + i];
            for (int k = 0; k < j; ++k) v -= L[k * n + i] * L[k * n + j];
            L[j * n + i] = v / ljj;
        }
    }
    return 0;
}

// X = L^-T (column-major, upper triangular) of a Cholesky factor L: the columns of Z X are orthonormal when Z^T Z = L L^T
inline void small_inv_lt(int n, const double *L, double *X)
{
    for (int i = 0; i < n * n; ++i) X[i] = 0.0;
    for (int j = 0; j < n; ++j) {                                 // column j of L^-T solves L^T x = e_j: back-substitution
        for (int i = j; i >= 0; --i) {
            double v = i == j ? 1.0 : 0.0;
            for (int k = i + 1; k <= j; ++k) v -= L[i * n + k] * X[j * n + k];
            X[j * n + i] = v / L[i * n + i];
        }
    }
}

}  // namespace nf
#endif
