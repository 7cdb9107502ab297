// The arithmetic of movba_two_view (include/movba.h): the five-point minimal solver, the Sampson score, the decomposition of
// an essential matrix with its cheirality test, the local optimisation of movba_two_view_lo (tv_lo_*), and the body of
// TwoViewReconstruction::CheckRT (TwoViewReconstruction.cc:120-245) for one match.  Plain C++ over doubles, shared by the
// kernels (two_view.hip), by the host-only test build's fake device (tests/hipstub/fake_two_view.cpp) and by the serial
// driver of the refit (tests/two_view_lo/lo_main.cpp).
//
// The solver (tv_five_point) is written for a GROUP of `nl` co-operating lanes that share one TvWork (LDS on the device) and
// meet at `sync()`; every loop over independent items is strided by the lane, so the same text runs on one host thread
// (nl = 1, sync = nothing) and on a 256-thread workgroup (sync = __syncthreads).  Each item is computed by exactly one lane
// with the same statements whatever nl is: the result does not depend on the group's size.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "magsac.h"
#include "movba.h"
#include "triangulate_math.h"

namespace movba {

constexpr int kTvMaxSol = 10;           // real roots of the degree-10 polynomial at most
constexpr int kTvBisect = 44;           // bisection steps per bracket ([-1, 1] -> 1e-13), then ...
constexpr int kTvNewton = 3;            // ... safeguarded Newton steps
constexpr int kTvPolish = 2;             // Gauss-Newton steps on a candidate
constexpr int kTvSvdSweeps = 15;
constexpr int kTvOutDoubles = 32;       // per pair: pose 7, E 9, parallax, outcome, n_inliers, n_pass, n_good, samples_used, winner
constexpr double kTvCosGood = 0.99998;  // (TwoViewReconstruction.cc:195, :201, :230)

struct TvWork {
    double A[10][20];       // the ten cubic constraints over the 20 monomials, then its reduced row echelon form
    double basis[4][9];     // null space of the epipolar system: E = x basis[0] + y basis[1] + z basis[2] + basis[3]
    double tmp[10][16];     // per-row products of two linear forms / scratch of the determinant
    double M5[5][9];
    double bz[3][3][5];     // B(z): coefficients in z, ascending, of the 3 x 3 system over (x, y, 1)
    double C[2][11];        // det B(z) ascending, and the reversed polynomial z^10 p(1 / z)
    double D[2][10][11];    // D[p][d - 1]: the (10 - d)-th derivative of C[p] over (10 - d)!: degree d
    double R[2][2][12];     // roots of two successive levels
    double slot[2][12];
    double root[kTvMaxSol];
    int perm[9];
    int cnt[2][2];
    int rev[kTvMaxSol];
    int nroot, ok;
};

struct TvSyncNone { __host__ __device__ void operator()() const {} };

// column of the monomial x^ex y^ey z^ez, given as a product of three of (x, y, z, 1) = (0, 1, 2, 3); the order is Nister's:
// x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ __forceinline__ int tv_col(int a, int b, int c)
{
    const int ex = (a == 0) + (b == 0) + (c == 0), ey = (a == 1) + (b == 1) + (c == 1), ez = (a == 2) + (b == 2) + (c == 2);
    switch (ex * 16 + ey * 4 + ez) {
    case 48: return 0;
    case 12: return 1;
    case 36: return 2;
    case 24: return 3;
    case 33: return 4;
    case 32: return 5;
    case 9: return 6;
    case 8: return 7;
    case 21: return 8;
    case 20: return 9;
    case 18: return 10;
    case 17: return 11;
    case 16: return 12;
    case 6: return 13;
    case 5: return 14;
    case 4: return 15;
    case 3: return 16;
    case 2: return 17;
    case 1: return 18;
    default: return 19;
    }
}

__host__ __device__ __forceinline__ double tv_horner(const double *c, int deg, double x)
{
    double v = c[deg];
    for (int i = deg - 1; i >= 0; --i) v = v * x + c[i];
    return v;
}

// The root of f (degree deg) in [a, b], where f is monotonic: NaN without a sign change.  The sign test takes 0 for positive
// at both ends, so a zero exactly ON an inner interval end is found by the one neighbour on whose other end f is negative
// (once, never twice; a zero that f only touches there is a double root and is left out).  The outer ends -1 and +1 have no
// neighbour: a zero exactly there is taken here.
__host__ __device__ inline double tv_refine(const double *f, int deg, double a, double b)
{
    const double fa = tv_horner(f, deg, a), fb = tv_horner(f, deg, b);
    if (fa == 0.0 && a == -1.0) return a;
    if (fb == 0.0 && b == 1.0) return b;
    const bool sa = fa < 0.0;
    if (sa == (fb < 0.0)) return __builtin_nan("");
    double lo = a, hi = b;
    for (int it = 0; it < kTvBisect; ++it) {
        const double mid = 0.5 * (lo + hi);
        if ((tv_horner(f, deg, mid) < 0.0) == sa) lo = mid; else hi = mid;
    }
    double x = 0.5 * (lo + hi);
    for (int it = 0; it < kTvNewton; ++it) {
        double v = f[deg], dv = 0.0;
        for (int i = deg - 1; i >= 0; --i) { dv = dv * x + v; v = v * x + f[i]; }
        const double xn = x - v / dv;
        if (xn > lo && xn < hi) x = xn;
    }
    return x;
}

#define TV_E(i, j, a) w.basis[a][3 * (i) + (j)]

// Five-point relative pose (Nister, PAMI 2004).  q: the five matches, (x1 y1 x2 y2) each, normalised coordinates.  Writes
// up to ten essential matrices (row-major, Frobenius norm sqrt 2) to Eout and their number to *nsol.
//   1. null space of the 5 x 9 epipolar system (Gauss-Jordan with full pivoting, then two Gram-Schmidt passes);
//   2. det E = 0 and 2 E E^T E - tr(E E^T) E = 0 expanded over the 20 monomials of degree <= 3 in (x, y, z): a 10 x 20 matrix;
//   3. Gauss-Jordan with partial pivoting (the lanes own the columns), rows x^2z - z x^2, y^2z - z y^2, xyz - z xy: B(z) (x y 1)^T = 0;
//   4. det B(z): degree 10.  Real roots by the derivative chain: the roots of p^(k + 1) split [-1, 1] into intervals on which
//      p^(k) is monotonic, so every interval with a sign change holds exactly one root (bisection + Newton); |z| > 1 through
//      the reversed polynomial in 1 / z on (-1, 1).  Work bound: 2 polynomials x 10 levels x <= 11 intervals x (44 + 3) evaluations;
//   5. per root: (x, y, 1) from the largest cross product of two rows of B(z), two Gauss-Newton steps on the constraints, E,
//      normalisation.
template <class Sync>
__host__ __device__ inline void tv_five_point(TvWork &w, const double *q, double *Eout, int *nsol, int lane, int nl, Sync sync)
{
    // ---- 1 ----
    if (lane == 0) {
        w.ok = 1;
        for (int m = 0; m < 5; ++m) {
            const double x1 = q[4 * m], y1 = q[4 * m + 1], x2 = q[4 * m + 2], y2 = q[4 * m + 3];
            double *r = w.M5[m];
            r[0] = x2 * x1; r[1] = x2 * y1; r[2] = x2; r[3] = y2 * x1; r[4] = y2 * y1; r[5] = y2; r[6] = x1; r[7] = y1; r[8] = 1.0;
        }
        for (int c = 0; c < 9; ++c) w.perm[c] = c;
        for (int k = 0; k < 5; ++k) {
            int pr = k, pc = k;
            double best = -1.0;
            for (int r = k; r < 5; ++r)
                for (int c = k; c < 9; ++c) {
                    const double v = fabs(w.M5[r][c]);
                    if (v > best) { best = v; pr = r; pc = c; }
                }
            for (int c = 0; c < 9; ++c) { const double t = w.M5[k][c]; w.M5[k][c] = w.M5[pr][c]; w.M5[pr][c] = t; }
            for (int r = 0; r < 5; ++r) { const double t = w.M5[r][k]; w.M5[r][k] = w.M5[r][pc]; w.M5[r][pc] = t; }
            { const int t = w.perm[k]; w.perm[k] = w.perm[pc]; w.perm[pc] = t; }
            double piv = w.M5[k][k];
            if (!(fabs(piv) > 0.0)) { w.ok = 0; piv = 1.0; }
            const double ip = 1.0 / piv;
            for (int c = 0; c < 9; ++c) w.M5[k][c] *= ip;
            for (int r = 0; r < 5; ++r) {
                if (r == k) continue;
                const double f = w.M5[r][k];
                for (int c = 0; c < 9; ++c) w.M5[r][c] -= f * w.M5[k][c];
            }
        }
        for (int j = 0; j < 4; ++j) {
            for (int c = 0; c < 9; ++c) w.basis[j][c] = 0.0;
            w.basis[j][w.perm[5 + j]] = 1.0;
            for (int i = 0; i < 5; ++i) w.basis[j][w.perm[i]] = -w.M5[i][5 + j];
        }
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < 4; ++j) {
                for (int i = 0; i < j; ++i) {
                    double d = 0.0;
                    for (int c = 0; c < 9; ++c) d += w.basis[i][c] * w.basis[j][c];
                    for (int c = 0; c < 9; ++c) w.basis[j][c] -= d * w.basis[i][c];
                }
                double nn = 0.0;
                for (int c = 0; c < 9; ++c) nn += w.basis[j][c] * w.basis[j][c];
                const double inv = 1.0 / sqrt(nn);
                for (int c = 0; c < 9; ++c) w.basis[j][c] *= inv;
            }
        w.cnt[0][0] = 0; w.cnt[1][0] = 0;
    }
    sync();
    // ---- 2: lane r expands constraint r into row r ----
    for (int r = lane; r < 10; r += nl) {
        double *row = w.A[r], *t = w.tmp[r];
        for (int c = 0; c < 20; ++c) row[c] = 0.0;
        if (r < 9) {
            const int i = r / 3, j = r % 3;
            for (int k = 0; k < 3; ++k) {
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b)
                        t[4 * a + b] = TV_E(i, 0, a) * TV_E(k, 0, b) + TV_E(i, 1, a) * TV_E(k, 1, b) + TV_E(i, 2, a) * TV_E(k, 2, b);
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b)
                        for (int c = 0; c < 4; ++c) row[tv_col(a, b, c)] += 2.0 * t[4 * a + b] * TV_E(k, j, c);
            }
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) {
                    double s = 0.0;
                    for (int e = 0; e < 9; ++e) s += w.basis[a][e] * w.basis[b][e];
                    t[4 * a + b] = s;
                }
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b)
                    for (int c = 0; c < 4; ++c) row[tv_col(a, b, c)] -= t[4 * a + b] * TV_E(i, j, c);
        } else {
            for (int pm = 0; pm < 6; ++pm) {
                const int p0 = pm >> 1, p1 = (pm & 1) ? (p0 + 2) % 3 : (p0 + 1) % 3, p2 = 3 - p0 - p1;
                const double sg = (pm & 1) ? -1.0 : 1.0;
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b)
                        for (int c = 0; c < 4; ++c) row[tv_col(a, b, c)] += sg * (TV_E(0, p0, a) * TV_E(1, p1, b)) * TV_E(2, p2, c);
            }
        }
    }
    sync();
    // ---- 3: Gauss-Jordan, partial pivoting; every lane reads column k, then updates the columns it owns ----
    bool bad = false;
    for (int k = 0; k < 10; ++k) {
        int p = k;
        double best = fabs(w.A[k][k]);
        for (int r = k + 1; r < 10; ++r) {
            const double v = fabs(w.A[r][k]);
            if (v > best) { best = v; p = r; }
        }
        double f[10];
#pragma unroll
        for (int r = 0; r < 10; ++r) f[r] = w.A[r == k ? p : (r == p ? k : r)][k];
        sync();
        double piv = 0.0;
#pragma unroll
        for (int r = 0; r < 10; ++r) piv = r == k ? f[r] : piv;
        if (!(fabs(piv) > 0.0)) { bad = true; piv = 1.0; }
        const double ip = 1.0 / piv;
        for (int c = lane; c < 20; c += nl) {
            const double ak = w.A[p][c], ap = w.A[k][c];
            w.A[p][c] = ap;
            const double s = ak * ip;
            w.A[k][c] = s;
#pragma unroll
            for (int r = 0; r < 10; ++r) {
                if (r == k) continue;
                const double base = r == p ? ap : w.A[r][c];
                w.A[r][c] = base - f[r] * s;
            }
        }
        sync();
    }
    // ---- 4: B(z), its determinant, the derivative chain ----
    if (lane == 0) {
        if (bad) w.ok = 0;
        for (int i = 0; i < 3; ++i) {
            const double *a = w.A[4 + 2 * i], *b = w.A[5 + 2 * i];
            double *bx = w.bz[i][0], *by = w.bz[i][1], *b1 = w.bz[i][2];
            bx[0] = a[12]; bx[1] = a[11] - b[12]; bx[2] = a[10] - b[11]; bx[3] = -b[10]; bx[4] = 0.0;
            by[0] = a[15]; by[1] = a[14] - b[15]; by[2] = a[13] - b[14]; by[3] = -b[13]; by[4] = 0.0;
            b1[0] = a[19]; b1[1] = a[18] - b[19]; b1[2] = a[17] - b[18]; b1[3] = a[16] - b[17]; b1[4] = -b[16];
        }
        double *mn = w.tmp[0], *P = w.tmp[1];       // minor (9 coefficients), determinant (13)
        for (int e = 0; e < 13; ++e) P[e] = 0.0;
        for (int j = 0; j < 3; ++j) {
            const int c1 = (j + 1) % 3, c2 = (j + 2) % 3;       // cofactor of (0, j): cyclic columns, no sign
            for (int e = 0; e < 9; ++e) mn[e] = 0.0;
            for (int u = 0; u < 5; ++u)
                for (int v = 0; v < 5; ++v)
                    mn[u + v] += w.bz[1][c1][u] * w.bz[2][c2][v] - w.bz[1][c2][u] * w.bz[2][c1][v];
            for (int u = 0; u < 5; ++u)
                for (int v = 0; v < 9; ++v) P[u + v] += w.bz[0][j][u] * mn[v];
        }
        double big = 0.0;
        for (int e = 0; e <= 10; ++e) big = fmax(big, fabs(P[e]));
        if (!(big > 0.0) || big > DBL_MAX) { w.ok = 0; big = 1.0; }
        const double sc = 1.0 / big;
        for (int e = 0; e <= 10; ++e) { w.C[0][e] = P[e] * sc; }
        for (int e = 0; e <= 10; ++e) w.C[1][e] = w.C[0][10 - e];
    }
    sync();
    for (int it = lane; it < 20; it += nl) {
        const int p = it / 10, d = it % 10 + 1, k = 10 - d;
        for (int i = 0; i <= d; ++i) {
            double bn = 1.0;
            for (int u = 1; u <= k; ++u) bn = bn * (double)(i + u) / (double)u;
            w.D[p][d - 1][i] = bn * w.C[p][i + k];
        }
    }
    sync();
    for (int d = 1; d <= 10; ++d) {
        const int cur = (d - 1) & 1, nxt = d & 1;
        for (int it = lane; it < 24; it += nl) {
            const int p = it / 12, i = it % 12, m = w.cnt[p][cur];
            if (i <= m) {
                const double a = i == 0 ? -1.0 : w.R[p][cur][i - 1], b = i == m ? 1.0 : w.R[p][cur][i];
                w.slot[p][i] = tv_refine(w.D[p][d - 1], d, a, b);
            }
        }
        sync();
        for (int p = lane; p < 2; p += nl) {
            const int m = w.cnt[p][cur];
            int n = 0;
            for (int i = 0; i <= m; ++i) {
                const double r = w.slot[p][i];
                if (r == r) w.R[p][nxt][n++] = r;
            }
            w.cnt[p][nxt] = n;
        }
        sync();
    }
    if (lane == 0) {
        int n = 0;
        if (w.ok) {
            for (int i = 0; i < w.cnt[0][0] && n < kTvMaxSol; ++i) { w.root[n] = w.R[0][0][i]; w.rev[n++] = 0; }
            for (int i = 0; i < w.cnt[1][0] && n < kTvMaxSol; ++i) {
                const double r = w.R[1][0][i];
                if (r != 0.0 && fabs(r) < 1.0) { w.root[n] = r; w.rev[n++] = 1; }
            }
        }
        w.nroot = n;
        *nsol = n;
    }
    sync();
    // ---- 5 ----
    for (int s = lane; s < w.nroot; s += nl) {
        const double z = w.root[s];
        const bool rev = w.rev[s] != 0;
        double B[3][3];
        for (int i = 0; i < 3; ++i) {
            if (!rev) {
                for (int j = 0; j < 3; ++j) B[i][j] = tv_horner(w.bz[i][j], 4, z);
            } else {            // the row times z^-4, in u = 1 / z
                for (int j = 0; j < 2; ++j) { const double *c = w.bz[i][j]; B[i][j] = z * (c[3] + z * (c[2] + z * (c[1] + z * c[0]))); }
                const double *c = w.bz[i][2];
                B[i][2] = c[4] + z * (c[3] + z * (c[2] + z * (c[1] + z * c[0])));
            }
        }
        double v[3] = { 0.0, 0.0, 0.0 }, bn = -1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int a = i, b = (i + 1) % 3;
            const double c0 = B[a][1] * B[b][2] - B[a][2] * B[b][1], c1 = B[a][2] * B[b][0] - B[a][0] * B[b][2],
                         c2 = B[a][0] * B[b][1] - B[a][1] * B[b][0];
            const double nn = c0 * c0 + c1 * c1 + c2 * c2;
            if (nn > bn) { bn = nn; v[0] = c0; v[1] = c1; v[2] = c2; }
        }
        // Two roots can lie close together in z while their (x, y) differ (z is one coordinate of the solution): B(z) is then
        // nearly of rank 1 and (x, y) from it is inexact.  Polish (x, y, z) on the ten constraints themselves (their reduced
        // form: the same solution set) by kTvPolish Gauss-Newton steps, kept when the residual does not grow.
        double xs = v[0] / v[2], ys = v[1] / v[2], zs = rev ? 1.0 / z : z, res0 = 0.0;
        bool polished = false;
        if (xs == xs && ys == ys && fabs(xs) < DBL_MAX && fabs(ys) < DBL_MAX) {
            double xc = xs, yc = ys, zc = zs;
#pragma unroll 1
            for (int it = 0; it <= kTvPolish; ++it) {
                const double x = xc, y = yc, zz = zc;
                const double m[20] = { x * x * x, y * y * y, x * x * y, x * y * y, x * x * zz, x * x, y * y * zz, y * y, x * y * zz, x * y,
                                       x * zz * zz, x * zz, x, y * zz * zz, y * zz, y, zz * zz * zz, zz * zz, zz, 1.0 };
                const double dx[20] = { 3.0 * x * x, 0.0, 2.0 * x * y, y * y, 2.0 * x * zz, 2.0 * x, 0.0, 0.0, y * zz, y,
                                        zz * zz, zz, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
                const double dy[20] = { 0.0, 3.0 * y * y, x * x, 2.0 * x * y, 0.0, 0.0, 2.0 * y * zz, 2.0 * y, x * zz, x,
                                        0.0, 0.0, 0.0, zz * zz, zz, 1.0, 0.0, 0.0, 0.0, 0.0 };
                const double dz[20] = { 0.0, 0.0, 0.0, 0.0, x * x, 0.0, y * y, 0.0, x * y, 0.0,
                                        2.0 * x * zz, x, 0.0, 2.0 * y * zz, y, 0.0, 3.0 * zz * zz, 2.0 * zz, 1.0, 0.0 };
                double N[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, g[3] = { 0.0, 0.0, 0.0 }, rr = 0.0;
#pragma unroll 1
                for (int k = 0; k < 10; ++k) {       // (one row at a time: the 20 monomials and their derivatives stay in registers)
                    double r = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
#pragma unroll
                    for (int c = 0; c < 20; ++c) {
                        const double a = w.A[k][c];
                        r += a * m[c]; jx += a * dx[c]; jy += a * dy[c]; jz += a * dz[c];
                    }
                    rr += r * r;
                    N[0] += jx * jx; N[1] += jx * jy; N[2] += jx * jz; N[3] += jy * jy; N[4] += jy * jz; N[5] += jz * jz;
                    g[0] += jx * r; g[1] += jy * r; g[2] += jz * r;
                }
                if (it == 0) res0 = rr;
                if (it == kTvPolish) { polished = rr <= res0; break; }
                const double c00 = N[3] * N[5] - N[4] * N[4], c01 = N[2] * N[4] - N[1] * N[5], c02 = N[1] * N[4] - N[2] * N[3];
                const double det = N[0] * c00 + N[1] * c01 + N[2] * c02;
                const double c11 = N[0] * N[5] - N[2] * N[2], c12 = N[1] * N[2] - N[0] * N[4], c22 = N[0] * N[3] - N[1] * N[1];
                const double id = 1.0 / det;
                xc = x - (c00 * g[0] + c01 * g[1] + c02 * g[2]) * id;
                yc = y - (c01 * g[0] + c11 * g[1] + c12 * g[2]) * id;
                zc = zz - (c02 * g[0] + c12 * g[1] + c22 * g[2]) * id;
            }
            if (polished) { xs = xc; ys = yc; zs = zc; }
        }
        double E[9], nn = 0.0;
        for (int e = 0; e < 9; ++e) {
            E[e] = polished ? xs * w.basis[0][e] + ys * w.basis[1][e] + zs * w.basis[2][e] + w.basis[3][e]
                 : !rev ? v[0] * w.basis[0][e] + v[1] * w.basis[1][e] + v[2] * (z * w.basis[2][e] + w.basis[3][e])
                        : z * (v[0] * w.basis[0][e] + v[1] * w.basis[1][e] + v[2] * w.basis[3][e]) + v[2] * w.basis[2][e];
            nn += E[e] * E[e];
        }
        const double sc = 1.4142135623730951 / sqrt(nn);
        for (int e = 0; e < 9; ++e) Eout[9 * s + e] = E[e] * sc;
    }
    sync();
}
#undef TV_E

// squared Sampson distance of a match to E in normalised coordinates (times f^2: in pixels, F = K_f^-T E K_f^-1)
__host__ __device__ __forceinline__ double tv_sampson2(const double *E, double x1, double y1, double x2, double y2)
{
    const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
    const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
    const double num = x2 * a0 + y2 * a1 + a2;
    return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// the stopping rule over the samples in drawing order (sl / sc / sb: loss, inlier count and candidate index of each sample's
// best candidate, sb < 0: the sample has none): N = log(1 - confidence) / log(1 - w^5), w the inlier ratio of the best so far
__host__ __device__ inline void tv_walk(const double *sl, const int *sc, const int *sb, int n_hyp, int n, double conf, int *best_out, int *used_out)
{
    int best = -1, used = n_hyp;
    double bl = DBL_MAX, need = DBL_MAX;
    const bool stop_rule = conf > 0.0 && conf < 1.0;
    const double lconf = stop_rule ? log(1.0 - conf) : 0.0;
    for (int h = 0; h < n_hyp; ++h) {
        if (sb[h] >= 0 && sl[h] < bl) {
            best = sb[h]; bl = sl[h];
            if (stop_rule) {
                const double wr = (double)sc[h] / (double)n, w5 = wr * wr * wr * wr * wr;
                const double l = w5 >= 1.0 ? 0.0 : log(1.0 - w5);
                need = w5 >= 1.0 ? 0.0 : (l < 0.0 ? lconf / l : DBL_MAX);
            }
        }
        if (stop_rule && best >= 0 && (double)(h + 1) >= need) { used = h + 1; break; }
    }
    *best_out = best; *used_out = used;
}

// E = U diag(s, s, 0) V^T by a one-sided Jacobi iteration on E itself; the four poses are (R1, t), (R2, t), (R1, -t), (R2, -t)
// with R1 = U W V^T, R2 = U W^T V^T, t = u3, U = [u1 u2 u1 x u2] and V likewise (both proper): det R = +1.
__host__ __device__ inline void tv_decompose(const double *Ein, double *R1, double *R2, double *t)
{
    double A[9], V[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { A[k] = Ein[k]; V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kTvSvdSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    alpha += A[3 * r + p] * A[3 * r + p];
                    beta += A[3 * r + q] * A[3 * r + q];
                    gamma += A[3 * r + p] * A[3 * r + q];
                }
                if (fabs(gamma) > 2.2e-16 * sqrt(alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma), az = fabs(zeta);
                    double tt = 1.0 / (az + sqrt(1.0 + az * az));
                    if (zeta < 0.0) tt = -tt;
                    const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const double ap = A[3 * r + p], aq = A[3 * r + q];
                        A[3 * r + p] = c * ap - s * aq; A[3 * r + q] = s * ap + c * aq;
                        const double vp = V[3 * r + p], vq = V[3 * r + q];
                        V[3 * r + p] = c * vp - s * vq; V[3 * r + q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    double nn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nn[c] = A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c];
    const int cm = (nn[0] <= nn[1] && nn[0] <= nn[2]) ? 0 : (nn[1] <= nn[2] ? 1 : 2);
    double u1[3], u2[3], v1[3], v2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a0 = A[3 * r], a1 = A[3 * r + 1], a2 = A[3 * r + 2], b0 = V[3 * r], b1 = V[3 * r + 1], b2 = V[3 * r + 2];
        u1[r] = cm == 0 ? a1 : (cm == 1 ? a2 : a0); u2[r] = cm == 0 ? a2 : (cm == 1 ? a0 : a1);
        v1[r] = cm == 0 ? b1 : (cm == 1 ? b2 : b0); v2[r] = cm == 0 ? b2 : (cm == 1 ? b0 : b1);
    }
    const double i1 = 1.0 / sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]), i2 = 1.0 / sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] *= i1; u2[r] *= i2; }
    const double u3[3] = { u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0] };
    const double v3[3] = { v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0] };
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double skew = u1[r] * v2[c] - u2[r] * v1[c], ax = u3[r] * v3[c];
            R1[3 * r + c] = skew + ax;
            R2[3 * r + c] = ax - skew;
        }
        t[r] = u3[r];
    }
}

// cv::recoverPose's test of one match against [I | 0], [R | t] (normalised coordinates): linear triangulation, both depths in (0, max_depth)
__host__ __device__ __forceinline__ bool tv_cheirality(const double *R, const double *t, double x1, double y1, double x2, double y2, double max_depth)
{
    double A[16], x[4];
    A[0] = -1.0; A[1] = 0.0; A[2] = x1; A[3] = 0.0;
    A[4] = 0.0; A[5] = -1.0; A[6] = y1; A[7] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double p0 = c < 3 ? R[c] : t[0], p1 = c < 3 ? R[3 + c] : t[1], p2 = c < 3 ? R[6 + c] : t[2];
        A[8 + c] = x2 * p2 - p0;
        A[12 + c] = y2 * p2 - p1;
    }
    tri_null4(A, x);
    const double X0 = x[0] / x[3], X1 = x[1] / x[3], X2 = x[2] / x[3];
    const double z2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
    return X2 > 0.0 && X2 < max_depth && z2 > 0.0 && z2 < max_depth;
}

// One match through CheckRT (TwoViewReconstruction.cc:163-231), pixels, the true fx and fy.  Returns MOVBA_TV_CHK_*; X (camera 1)
// and *cosp are written for an accepted match only (X: NaN otherwise).
__host__ __device__ __forceinline__ uint8_t tv_check(const double *R, const double *t, double fx, double fy, double cx, double cy,
                                                     double u1, double w1, double u2, double w2, double th2, double *X, double *cosp)
{
    const double nan = __builtin_nan("");
    X[0] = nan; X[1] = nan; X[2] = nan;
    double A[16], x[4];
    A[0] = -fx; A[1] = 0.0; A[2] = u1 - cx; A[3] = 0.0;
    A[4] = 0.0; A[5] = -fy; A[6] = w1 - cy; A[7] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double r0 = c < 3 ? R[c] : t[0], r1 = c < 3 ? R[3 + c] : t[1], r2 = c < 3 ? R[6 + c] : t[2];
        const double p0 = fx * r0 + cx * r2, p1 = fy * r1 + cy * r2;
        A[8 + c] = u2 * r2 - p0;
        A[12 + c] = w2 * r2 - p1;
    }
    tri_null4(A, x);
    if (x[3] == 0.0) return MOVBA_TV_CHK_REJ_W0;
    const double P0 = x[0] / x[3], P1 = x[1] / x[3], P2 = x[2] / x[3];
    // O2 = -R^T t (:150); parallax (:186-192)
    const double o0 = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), o1 = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]),
                 o2 = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
    const double n0 = P0 - o0, n1 = P1 - o1, n2 = P2 - o2;
    const double dist1 = sqrt(P0 * P0 + P1 * P1 + P2 * P2), dist2 = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double cosv = (P0 * n0 + P1 * n1 + P2 * n2) / (dist1 * dist2);
    if (P2 <= 0.0 && cosv < kTvCosGood) return MOVBA_TV_CHK_REJ_BEHIND1;
    const double q0 = R[0] * P0 + R[1] * P1 + R[2] * P2 + t[0], q1 = R[3] * P0 + R[4] * P1 + R[5] * P2 + t[1],
                 q2 = R[6] * P0 + R[7] * P1 + R[8] * P2 + t[2];
    if (q2 <= 0.0 && cosv < kTvCosGood) return MOVBA_TV_CHK_REJ_BEHIND2;
    const double iz1 = 1.0 / P2;
    const double e1x = fx * P0 * iz1 + cx - u1, e1y = fy * P1 * iz1 + cy - w1;
    if (e1x * e1x + e1y * e1y > th2) return MOVBA_TV_CHK_REJ_REPROJ1;
    const double iz2 = 1.0 / q2;
    const double e2x = fx * q0 * iz2 + cx - u2, e2y = fy * q1 * iz2 + cy - w2;
    if (e2x * e2x + e2y * e2y > th2) return MOVBA_TV_CHK_REJ_REPROJ2;
    X[0] = P0; X[1] = P1; X[2] = P2;
    *cosp = cosv;
    return cosv < kTvCosGood ? MOVBA_TV_CHK_GOOD : MOVBA_TV_CHK_LOW_PARALLAX;
}

// ---- stage 2b: local optimisation of the winner (movba_two_view_lo, include/movba.h) ----
// Iteratively reweighted Gauss-Newton on the signed Sampson distance with sigma-consensus++ weights over E = [t]x R, |t| = 1.
constexpr int kTvLoAcc = 21;        // per pass: the 15 entries of H's upper triangle (row-major), g 5, the loss
constexpr int kTvLoDoubles = 24;    // per-pair slot: kept E 9, E0 9, loss0, loss, kept, steps, n_inliers0, mark

struct TvLoState {
    double R[9], t[3];
    double E[9];            // what the pass scores: E0 itself at iterate 0, [t]x R afterwards
    double dE[5][9];        // dE / d omega_k = [t]x [e_k]x R, dE / d tau_j = [b_j]x R
};

// out = [v]x M (row-major 3 x 3)
__host__ __device__ __forceinline__ void tv_skew_mul(const double *v, const double *M, double *out)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c] = v[1] * M[6 + c] - v[2] * M[3 + c];
        out[3 + c] = v[2] * M[c] - v[0] * M[6 + c];
        out[6 + c] = v[0] * M[3 + c] - v[1] * M[c];
    }
}

// the tangent basis of the unit vector t: b1 = normalise(t x e_k), k the index of the smallest |t_k| (the lowest on a tie), b2 = t x b1
__host__ __device__ inline void tv_lo_tangent(const double *t, double *b1, double *b2)
{
    int k = 0;
    if (fabs(t[1]) < fabs(t[k])) k = 1;
    if (fabs(t[2]) < fabs(t[k])) k = 2;
    const double e[3] = { k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0 };
    b1[0] = t[1] * e[2] - t[2] * e[1]; b1[1] = t[2] * e[0] - t[0] * e[2]; b1[2] = t[0] * e[1] - t[1] * e[0];
    const double inv = 1.0 / sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
    b1[0] *= inv; b1[1] *= inv; b1[2] *= inv;
    b2[0] = t[1] * b1[2] - t[2] * b1[1]; b2[1] = t[2] * b1[0] - t[0] * b1[2]; b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// the five derivative matrices at (R, t)
__host__ __device__ inline void tv_lo_derivatives(TvLoState &s)
{
    const double *t = s.t;
    double b1[3], b2[3];
    tv_lo_tangent(t, b1, b2);
    for (int a = 0; a < 3; ++a) {
        const double ea[3] = { a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0 };
        double M[9];
        tv_skew_mul(ea, s.R, M);
        tv_skew_mul(t, M, s.dE[a]);
    }
    tv_skew_mul(b1, s.R, s.dE[3]);
    tv_skew_mul(b2, s.R, s.dE[4]);
}

// Rule 1: (R, t) of the winner E0 - of the decomposition's two rotations the one with the larger trace, the first on equal
// traces; t's sign so that <[t]x R, E0> >= 0.  Iterate 0 scores E0 itself.
__host__ __device__ inline void tv_lo_start(const double *E0, TvLoState &s)
{
    double R1[9], R2[9], E[9];
    tv_decompose(E0, R1, R2, s.t);
    const bool second = R2[0] + R2[4] + R2[8] > R1[0] + R1[4] + R1[8];
    for (int e = 0; e < 9; ++e) s.R[e] = second ? R2[e] : R1[e];
    tv_skew_mul(s.t, s.R, E);
    double dot = 0.0;
    for (int e = 0; e < 9; ++e) dot += E[e] * E0[e];
    if (dot < 0.0) { s.t[0] = -s.t[0]; s.t[1] = -s.t[1]; s.t[2] = -s.t[2]; }
    for (int e = 0; e < 9; ++e) s.E[e] = E0[e];
    tv_lo_derivatives(s);
}

// Rule 3 for one match (normalised coordinates): the signed Sampson distance in pixels and, for a pass that takes a step, its
// exact derivative by the five parameters (the denominator's included)
__host__ __device__ __forceinline__ double tv_lo_residual(const double *E, const double (*dE)[9], bool want, double f,
                                                          double x1, double y1, double x2, double y2, double *J)
{
    const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
    const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
    const double num = x2 * a0 + y2 * a1 + a2, den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
    const double is = 1.0 / sqrt(den);
    if (want) {
        const double hn = 0.5 * num / den;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const double *D = dE[j];
            const double c0 = D[0] * x1 + D[1] * y1 + D[2], c1 = D[3] * x1 + D[4] * y1 + D[5], c2 = D[6] * x1 + D[7] * y1 + D[8];
            const double d0 = D[0] * x2 + D[3] * y2 + D[6], d1 = D[1] * x2 + D[4] * y2 + D[7];
            const double dnum = x2 * c0 + y2 * c1 + c2, dden = 2.0 * (a0 * c0 + a1 * c1 + b0 * d0 + b1 * d1);
            J[j] = f * (dnum - hn * dden) * is;
        }
    }
    return f * num * is;
}

// Rule 4 for one match: acc[20] += loss; with `want`, H += w J J^T (upper triangle, row-major) and g += w J r.  A match beyond
// the gate (or with a residual that is not a number) has weight 0 and adds nothing to H and g.
__host__ __device__ __forceinline__ void tv_lo_accumulate(const Magsac &ms, double thr2, const double *E, const double (*dE)[9], bool want,
                                                          double f, double x1, double y1, double x2, double y2, double *acc)
{
    double J[5];
    const double r = tv_lo_residual(E, dE, want, f, x1, y1, x2, y2, J);
    double l1, wt;
    ms.terms(r * r, true, thr2, l1, wt);
    acc[20] += l1;
    if (want && wt > 0.0) {
        int e = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double wj = wt * J[i];
#pragma unroll
            for (int j = i; j < 5; ++j) acc[e++] += wj * J[j];
            acc[15 + i] += wj * r;
        }
    }
}

// delta = -H^-1 g by Cholesky of the 5 x 5 H, no damping; false when a pivot is not positive and finite
__host__ __device__ inline bool tv_lo_solve5(const double *acc, double *delta)
{
    double L[5][5];
    int e = 0;
    for (int i = 0; i < 5; ++i)
        for (int j = i; j < 5; ++j) L[j][i] = acc[e++];        // (lower triangle of H)
    for (int j = 0; j < 5; ++j) {
        double d = L[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !(d <= DBL_MAX)) return false;
        const double piv = sqrt(d), ip = 1.0 / piv;
        L[j][j] = piv;
        for (int i = j + 1; i < 5; ++i) {
            double v = L[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v * ip;
        }
    }
    double y[5];
    for (int i = 0; i < 5; ++i) {
        double v = -acc[15 + i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 4; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 5; ++k) v -= L[k][i] * delta[k];
        delta[i] = v / L[i][i];
    }
    return true;
}

// Rule 2: R <- exp([d omega]x) R (Rodrigues), t <- normalise(t + d tau_1 b1 + d tau_2 b2); then E = [t]x R and the derivatives
// at the new iterate.
__host__ __device__ inline void tv_lo_update(TvLoState &s, const double *delta)
{
    const double wx = delta[0], wy = delta[1], wz = delta[2], th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    const double A = th2 < 1e-8 ? 1.0 - th2 / 6.0 : sin(th) / th, B = th2 < 1e-8 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
    const double K[9] = { 0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0 };
    double X[9], Rn[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double k2 = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
            X[3 * i + j] = (i == j ? 1.0 : 0.0) + A * K[3 * i + j] + B * k2;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = X[3 * i] * s.R[j] + X[3 * i + 1] * s.R[3 + j] + X[3 * i + 2] * s.R[6 + j];
    for (int e = 0; e < 9; ++e) s.R[e] = Rn[e];
    // the tangent basis at the OLD t
    const double *t = s.t;
    double b1[3], b2[3];
    tv_lo_tangent(t, b1, b2);
    double tn[3];
    for (int i = 0; i < 3; ++i) tn[i] = t[i] + delta[3] * b1[i] + delta[4] * b2[i];
    const double it = 1.0 / sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
    for (int i = 0; i < 3; ++i) s.t[i] = tn[i] * it;
    tv_skew_mul(s.t, s.R, s.E);
    tv_lo_derivatives(s);
}

// Rules 4 and 5 between the passes, for the one thread that steers the refit: the winner, the kept iterate and the lowest loss so far
struct TvLoTrack {
    double E0[9], Ek[9], loss0, loss;
    int kept, steps;
};

__host__ __device__ inline void tv_lo_begin(const double *E0, TvLoState &st, TvLoTrack &tr)
{
    for (int e = 0; e < 9; ++e) { tr.E0[e] = E0[e]; tr.Ek[e] = E0[e]; }
    tr.loss0 = tr.loss = 0.0; tr.kept = tr.steps = 0;
    tv_lo_start(E0, st);
}

// after pass k (acc: its sums): keeps the iterate when its loss is the lowest so far (the lowest k wins a tie; a loss that is
// not a number is never kept), then steps when k < lo_iters.  false: the refit ends here.
__host__ __device__ inline bool tv_lo_advance(TvLoState &st, TvLoTrack &tr, const double *acc, int k, int lo_iters)
{
    const double L = acc[20];
    if (k == 0) {
        tr.loss0 = tr.loss = L;
    } else if (L < tr.loss) {
        tr.loss = L; tr.kept = k;
        for (int e = 0; e < 9; ++e) tr.Ek[e] = st.E[e];
    }
    double delta[5];
    if (k >= lo_iters || !tv_lo_solve5(acc, delta)) return false;
    tv_lo_update(st, delta);
    tr.steps = k + 1;
    return true;
}

// the E handed out: E0 itself for kept = 0, else the kept [t]x R with the sign that makes <E, E0> >= 0
__host__ __device__ inline void tv_lo_result(const TvLoTrack &tr, double *E)
{
    double dot = 0.0;
    for (int e = 0; e < 9; ++e) dot += tr.Ek[e] * tr.E0[e];
    const double sg = dot < 0.0 ? -1.0 : 1.0;
    for (int e = 0; e < 9; ++e) E[e] = tr.kept ? sg * tr.Ek[e] : tr.E0[e];
}

// rotation matrix (row-major) -> unit quaternion (x, y, z, w) (Eigen's conversion)
// (its own copy: host and device, compared bit for bit by the CPU drivers; device_math.h's R_to_quat and pose_kernels.hip's R2q round otherwise)
__host__ __device__ inline void tv_R2q(const double *m, double *q)
{
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else if (m[0] >= m[4] && m[0] >= m[8]) {
        t = sqrt(m[0] - m[4] - m[8] + 1.0); q[0] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t; q[1] = (m[3] + m[1]) * t; q[2] = (m[6] + m[2]) * t;
    } else if (m[4] > m[0] && m[4] >= m[8]) {
        t = sqrt(m[4] - m[8] - m[0] + 1.0); q[1] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t; q[2] = (m[7] + m[5]) * t; q[0] = (m[1] + m[3]) * t;
    } else {
        t = sqrt(m[8] - m[0] - m[4] + 1.0); q[2] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t; q[0] = (m[2] + m[6]) * t; q[1] = (m[5] + m[7]) * t;
    }
    const double n = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] *= n; q[1] *= n; q[2] *= n; q[3] *= n;
}

}  // namespace movba
