// The arithmetic of movba_triangulate (include/movba.h) for ONE match and its two views: the body of the loop at
// LocalMapping.cc:313-476 restated in fp64, quirks included.  Plain C++ over doubles, shared by the kernel (triangulate.hip)
// and by the host-only test build's fake device (tests/hipstub/fake_triangulate.cpp).  Every function is forced inline into
// its one caller, and the library is built with -ffp-contract=on, so a match rounds the same wherever it sits in a call.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "movba.h"

namespace movba {

// One view as the match arithmetic reads it: Rcw row-major [0..8], tcw [9..11], camera centre Ow = -Rcw^T tcw [12..14],
// fx fy cx cy [15..18], bf [19], b [20]; padded to 24 doubles.
constexpr int kTriViewDoubles = 24;
// sweeps of the one-sided Jacobi iteration at most (4 x 4, fp64: 4 - 7 until no pair is rotated)
constexpr int kTriMaxSweeps = 12;

__host__ __device__ __forceinline__ void tri_view(const double *pose, const double *cam, double bf, double b, double *v)
{
    double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
    const double n = sqrt(x * x + y * y + z * z + w * w);
    x = x / n; y = y / n; z = z / n; w = w / n;
    v[0] = 1.0 - 2.0 * (y * y + z * z); v[1] = 2.0 * (x * y - z * w);       v[2] = 2.0 * (x * z + y * w);
    v[3] = 2.0 * (x * y + z * w);       v[4] = 1.0 - 2.0 * (x * x + z * z); v[5] = 2.0 * (y * z - x * w);
    v[6] = 2.0 * (x * z - y * w);       v[7] = 2.0 * (y * z + x * w);       v[8] = 1.0 - 2.0 * (x * x + y * y);
    const double tx = pose[4], ty = pose[5], tz = pose[6];
    v[9] = tx; v[10] = ty; v[11] = tz;
    v[12] = -(v[0] * tx + v[3] * ty + v[6] * tz);
    v[13] = -(v[1] * tx + v[4] * ty + v[7] * tz);
    v[14] = -(v[2] * tx + v[5] * ty + v[8] * tz);
    v[15] = cam[0]; v[16] = cam[1]; v[17] = cam[2]; v[18] = cam[3];
    v[19] = bf; v[20] = b; v[21] = 0.0; v[22] = 0.0; v[23] = 0.0;
}

// cos(2 atan2(a, d)) (:346, :348) = (d^2 - a^2) / (d^2 + a^2): no transcendental call.  The corners as atan2 has them:
// a = d = 0 and infinite d give 1, a NaN stays a NaN (and fails every comparison, as in the reference).
__host__ __device__ __forceinline__ double tri_cos_stereo(double a, double d)
{
    const double dd = d * d, aa = a * a, den = dd + aa;
    if (den != den) return den;
    if (!(den > 0.0) || den > 1.7e308) return 1.0;
    return (dd - aa) / den;
}

// Null vector of the 4 x 4 system A (rows r, columns c: A[4 * r + c]) by the one-sided (Hestenes) Jacobi iteration: plane
// rotations from the right make the columns of A V orthogonal; the column of V that belongs to the shortest one is the
// right singular vector of the smallest singular value.  Works on A itself, not on A^T A: the condition number is not
// squared.  At most kTriMaxSweeps sweeps over the 6 column pairs in a fixed order; a sweep that rotates nothing ends it.
// Every index is a compile-time constant: A and V stay in registers.
__host__ __device__ __forceinline__ void tri_null4(double *A, double *x)
{
    double V[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kTriMaxSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    alpha += A[4 * r + p] * A[4 * r + p];
                    beta += A[4 * r + q] * A[4 * r + q];
                    gamma += A[4 * r + p] * A[4 * r + q];
                }
                if (fabs(gamma) > 2.2e-16 * sqrt(alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double az = fabs(zeta);
                    double t = 1.0 / (az + sqrt(1.0 + az * az));
                    if (zeta < 0.0) t = -t;
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ap = A[4 * r + p], aq = A[4 * r + q];
                        A[4 * r + p] = c * ap - s * aq;
                        A[4 * r + q] = s * ap + c * aq;
                        const double vp = V[4 * r + p], vq = V[4 * r + q];
                        V[4 * r + p] = c * vp - s * vq;
                        V[4 * r + q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double nn = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) nn += A[4 * r + c] * A[4 * r + c];
        if (c == 0 || nn < best) {
            best = nn;
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = V[4 * r + c];
        }
    }
}

// One match.  v1 / v2: the views of its pair (tri_view); (u1, w1), (u2, w2): the observations in pixels; ur* < 0: monocular
// observation; d*: stereo depth.  Returns MOVBA_TRI_*; X is the world point, NaN where none was reached.
__host__ __device__ __forceinline__ uint8_t tri_match(const double *v1, const double *v2, double u1, double w1, double u2, double w2,
                                                      double ur1, double d1, double ur2, double d2, double gate, double far_th, double *X)
{
    const double nan = __builtin_nan("");
    X[0] = nan; X[1] = nan; X[2] = nan;
    // unprojectEig, rays and their parallax (:334-339)
    const double a1 = (u1 - v1[17]) / v1[15], b1 = (w1 - v1[18]) / v1[16];
    const double a2 = (u2 - v2[17]) / v2[15], b2 = (w2 - v2[18]) / v2[16];
    const double r1x = v1[0] * a1 + v1[3] * b1 + v1[6], r1y = v1[1] * a1 + v1[4] * b1 + v1[7], r1z = v1[2] * a1 + v1[5] * b1 + v1[8];
    const double r2x = v2[0] * a2 + v2[3] * b2 + v2[6], r2y = v2[1] * a2 + v2[4] * b2 + v2[7], r2z = v2[2] * a2 + v2[5] * b2 + v2[8];
    const double cos_rays = (r1x * r2x + r1y * r2y + r1z * r2z) /
                            (sqrt(r1x * r1x + r1y * r1y + r1z * r1z) * sqrt(r2x * r2x + r2y * r2y + r2z * r2z));
    const bool st1 = ur1 >= 0.0, st2 = ur2 >= 0.0;
    // the stereo parallaxes as the if / else if leaves them (:341-348): view 2's only when view 1's observation is not stereo
    double c1 = cos_rays + 1.0, c2 = cos_rays + 1.0;
    if (st1) c1 = tri_cos_stereo(0.5 * v1[20], d1);
    else if (st2) c2 = tri_cos_stereo(0.5 * v2[20], d2);

    uint8_t accepted;
    if (!st1 && !st2) {
        // cv::triangulatePoints over the normalised coordinates with P = [Rcw | tcw] (:365-376)
        double A[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double p10 = c < 3 ? v1[c] : v1[9], p11 = c < 3 ? v1[3 + c] : v1[10], p12 = c < 3 ? v1[6 + c] : v1[11];
            const double p20 = c < 3 ? v2[c] : v2[9], p21 = c < 3 ? v2[3 + c] : v2[10], p22 = c < 3 ? v2[6 + c] : v2[11];
            A[c] = a1 * p12 - p10;
            A[4 + c] = b1 * p12 - p11;
            A[8 + c] = a2 * p22 - p20;
            A[12 + c] = b2 * p22 - p21;
        }
        double x[4];
        tri_null4(A, x);
        if (x[3] == 0.0) return MOVBA_TRI_REJ_W0;
        X[0] = x[0] / x[3]; X[1] = x[1] / x[3]; X[2] = x[2] / x[3];
        accepted = MOVBA_TRI_DLT;
    } else if (st1 && c1 < c2) {
        // KeyFrame::UnprojectStereo of view 1 (:382)
        if (!(d1 > 0.0)) return MOVBA_TRI_REJ_DEPTH;
        const double xc = (u1 - v1[17]) * d1 * (1.0 / v1[15]), yc = (w1 - v1[18]) * d1 * (1.0 / v1[16]);
        X[0] = v1[0] * xc + v1[3] * yc + v1[6] * d1 + v1[12];
        X[1] = v1[1] * xc + v1[4] * yc + v1[7] * d1 + v1[13];
        X[2] = v1[2] * xc + v1[5] * yc + v1[8] * d1 + v1[14];
        accepted = MOVBA_TRI_STEREO1;
    } else if (st2 && c2 < c1) {
        if (!(d2 > 0.0)) return MOVBA_TRI_REJ_DEPTH;
        const double xc = (u2 - v2[17]) * d2 * (1.0 / v2[15]), yc = (w2 - v2[18]) * d2 * (1.0 / v2[16]);
        X[0] = v2[0] * xc + v2[3] * yc + v2[6] * d2 + v2[12];
        X[1] = v2[1] * xc + v2[4] * yc + v2[7] * d2 + v2[13];
        X[2] = v2[2] * xc + v2[5] * yc + v2[8] * d2 + v2[14];
        accepted = MOVBA_TRI_STEREO2;
    } else {
        return MOVBA_TRI_REJ_PARALLAX;
    }

    // in front of both cameras (:399-409)
    const double z1 = v1[6] * X[0] + v1[7] * X[1] + v1[8] * X[2] + v1[11];
    if (z1 <= 0.0) return MOVBA_TRI_REJ_BEHIND1;
    const double z2 = v2[6] * X[0] + v2[7] * X[1] + v2[8] * X[2] + v2[11];
    if (z2 <= 0.0) return MOVBA_TRI_REJ_BEHIND2;

    // reprojection in view 1 (:412-437)
    const double x1 = v1[0] * X[0] + v1[1] * X[1] + v1[2] * X[2] + v1[9];
    const double y1 = v1[3] * X[0] + v1[4] * X[1] + v1[5] * X[2] + v1[10];
    const double invz1 = 1.0 / z1;
    if (!st1) {
        const double ex = v1[15] * x1 / z1 + v1[17] - u1, ey = v1[16] * y1 / z1 + v1[18] - w1;
        if (ex * ex + ey * ey > gate) return MOVBA_TRI_REJ_REPROJ1;
    } else {
        const double pu = v1[15] * x1 * invz1 + v1[17], pr = pu - v1[19] * invz1, pv = v1[16] * y1 * invz1 + v1[18];
        const double ex = pu - u1, ey = pv - w1, er = pr - ur1;
        if (ex * ex + ey * ey + er * er > gate) return MOVBA_TRI_REJ_REPROJ1;
    }
    // ... in view 2 (:440-463); its stereo residual subtracts VIEW 1's bf over z2, as the reference does (:456)
    const double x2 = v2[0] * X[0] + v2[1] * X[1] + v2[2] * X[2] + v2[9];
    const double y2 = v2[3] * X[0] + v2[4] * X[1] + v2[5] * X[2] + v2[10];
    const double invz2 = 1.0 / z2;
    if (!st2) {
        const double ex = v2[15] * x2 / z2 + v2[17] - u2, ey = v2[16] * y2 / z2 + v2[18] - w2;
        if (ex * ex + ey * ey > gate) return MOVBA_TRI_REJ_REPROJ2;
    } else {
        const double pu = v2[15] * x2 * invz2 + v2[17], pr = pu - v1[19] * invz2, pv = v2[16] * y2 * invz2 + v2[18];
        const double ex = pu - u2, ey = pv - w2, er = pr - ur2;
        if (ex * ex + ey * ey + er * er > gate) return MOVBA_TRI_REJ_REPROJ2;
    }

    // distances to the two camera centres (:466-480)
    const double e1x = X[0] - v1[12], e1y = X[1] - v1[13], e1z = X[2] - v1[14];
    const double e2x = X[0] - v2[12], e2y = X[1] - v2[13], e2z = X[2] - v2[14];
    const double dist1 = sqrt(e1x * e1x + e1y * e1y + e1z * e1z), dist2 = sqrt(e2x * e2x + e2y * e2y + e2z * e2z);
    if (dist1 == 0.0 || dist2 == 0.0) return MOVBA_TRI_REJ_ZERO_DIST;
    if (far_th > 0.0 && (dist1 >= far_th || dist2 >= far_th)) return MOVBA_TRI_REJ_FAR;
    return accepted;
}

}  // namespace movba
