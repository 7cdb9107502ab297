// Device view + launch wrapper of movba_init_map (init_map.hip; host side: init_map.cpp), and the per-point arithmetic of its
// two-keyframe bundle adjustment as plain C++ (what k_init_map inlines, and what a host build can run point by point).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace movba {

// One frame pair as the kernel reads it.  Every pointer is device memory or a device view of pinned host memory.
struct ImPair {
    int32_t n;                      // matches (0 for a pair without a used match: the kernel writes nothing for it)
    int32_t cap;                    // used matches as the host counted them in the staged mask: the stride of the pair's scratch
    int32_t m0;                     // first match of the pair in the call's concatenated input arrays
    int32_t max_iters, max_trials, min_tracked;
    int64_t s0;                     // first slot of the pair in the scratch arrays (sum of the earlier pairs' cap)
    double pose2[7];
    double fx, fy, cx, cy, huber;
    double *points, *chi2;          // n x 3 out; n x 2 out or nullptr
    double *out;                    // kImOutDoubles out
    double *trace;                  // kImTraceDoubles out or nullptr
};

struct ImDev {
    int32_t n_pairs;
    const ImPair *pairs;
    // all pairs' matches: observations x 2, start points x 3, information of the two edges (ones where the caller gave none),
    // mask bytes (ones where the caller gave none)
    const double *obs1, *obs2, *pts, *sig1, *sig2;
    const uint8_t *use;
    // scratch over all pairs' used matches (structure of arrays inside a pair: component c of point k at [c * cap + k])
    int32_t *idx;                   // the used matches of a pair, ascending
    double *X, *Xbk;                // 3 per point: estimate, and its backup for a rejected trial
    double *lin;                    // kImLin per point: Hll 6, b_l 3, Hpl 18 of the current linearisation
};

constexpr int kImThreads = 256;     // (k_pose_opt's)
constexpr int kImLin = 27;
// per pair: pose 7, median, outcome, n_used, iters_done, n_solves, last_rejected, n_chol_fail, lambda, cost0, cost
constexpr int kImOutDoubles = 24;
// per pair: n_trace, then lambda, f0, f1, rho, accept of MOVBA_MAX_TRACE trials each
constexpr int kImTraceDoubles = 1 + 5 * 128;

// k_init_map over all pairs on the stream
hipError_t launch_init_map(const ImDev &d, hipStream_t s);

// ---- the arithmetic of one map point ----

// RobustKernelHuber::robustify: rho0 and rho1 of chi2; delta <= 0: no kernel
__host__ __device__ inline void im_huber(double chi2, double delta, double &rho0, double &rho1)
{
    rho0 = chi2; rho1 = 1.0;
    if (delta > 0.0 && !(chi2 <= delta * delta)) {
        const double s = sqrt(chi2);
        rho0 = 2.0 * s * delta - delta * delta;
        rho1 = delta / s;
    }
}

// EdgeSE3ProjectXYZ::computeError over Pinhole::project: obs - (fx x / z + cx, fy y / z + cy), IEEE division (z = 0 gives inf)
__host__ __device__ inline void im_error(const double Xc[3], const double *obs, const double cam[4], double e[2])
{
    e[0] = obs[0] - (cam[0] * Xc[0] / Xc[2] + cam[2]);
    e[1] = obs[1] - (cam[1] * Xc[1] / Xc[2] + cam[3]);
}

// camera coordinates of world point X in keyframe 2 (R row-major, t)
__host__ __device__ inline void im_map(const double R[9], const double t[3], const double X[3], double Xc[3])
{
    Xc[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    Xc[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    Xc[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
}

// chi2 of the point's two edges (keyframe 1 at the identity, keyframe 2 at (R, t)) and their robust cost
__host__ __device__ inline double im_cost(const double R[9], const double t[3], const double cam[4], double huber, const double X[3],
                                          const double *o1, const double *o2, double s1, double s2, double chi2[2])
{
    double e[2], Xc[3], r0, r1, f;
    im_error(X, o1, cam, e);
    chi2[0] = s1 * (e[0] * e[0] + e[1] * e[1]);
    im_huber(chi2[0], huber, r0, r1);
    f = r0;
    im_map(R, t, X, Xc);
    im_error(Xc, o2, cam, e);
    chi2[1] = s2 * (e[0] * e[0] + e[1] * e[1]);
    im_huber(chi2[1], huber, r0, r1);
    return f + r0;
}

// EdgeSE3ProjectXYZ::linearizeOplus (OptimizableTypes.cpp:158-180): A = J_point (2 x 3), B = J_pose (2 x 6) at camera
// coordinates Xc under rotation R
__host__ __device__ inline void im_jacobians(const double R[9], const double Xc[3], const double cam[4], double A[6], double B[12])
{
    const double x = Xc[0], y = Xc[1], z = Xc[2];
    const double a00 = -(cam[0] / z), a02 = cam[0] * x / (z * z);
    const double a11 = -(cam[1] / z), a12 = cam[1] * y / (z * z);
    for (int j = 0; j < 3; ++j) {
        A[j] = a00 * R[j] + a02 * R[6 + j];
        A[3 + j] = a11 * R[3 + j] + a12 * R[6 + j];
    }
    B[0] = a02 * y;               B[1] = a00 * z + a02 * (-x); B[2] = a00 * (-y);
    B[3] = a00;                   B[4] = 0.0;                  B[5] = a02;
    B[6] = a11 * (-z) + a12 * y;  B[7] = a12 * (-x);           B[8] = a11 * x;
    B[9] = 0.0;                   B[10] = a11;                 B[11] = a12;
}

// buildSystem for one point: both edges linearised and robustified.  lin: Hll (xx xy xz yy yz zz), b_l, Hpl (6 x 3
// row-major, keyframe-2 edge).  acc += Hpp (upper triangle packed, 21), b_p (6), robust cost (1).
__host__ __device__ inline void im_linearize(const double R[9], const double t[3], const double cam[4], double huber, const double X[3],
                                             const double *o1, const double *o2, double s1, double s2, double lin[kImLin], double acc[28])
{
    const double I3[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
    double e[2], A[6], B[12], r0, r1, Xc[3];
    // keyframe 1: fixed, so the edge reaches Hll and b_l only
    im_error(X, o1, cam, e);
    im_huber(s1 * (e[0] * e[0] + e[1] * e[1]), huber, r0, r1);
    im_jacobians(I3, X, cam, A, B);
    double wo = r1 * s1, q0 = -s1 * e[0] * r1, q1 = -s1 * e[1] * r1;
    double F = r0;
    lin[0] = wo * (A[0] * A[0] + A[3] * A[3]); lin[1] = wo * (A[0] * A[1] + A[3] * A[4]); lin[2] = wo * (A[0] * A[2] + A[3] * A[5]);
    lin[3] = wo * (A[1] * A[1] + A[4] * A[4]); lin[4] = wo * (A[1] * A[2] + A[4] * A[5]); lin[5] = wo * (A[2] * A[2] + A[5] * A[5]);
    for (int a = 0; a < 3; ++a) lin[6 + a] = A[a] * q0 + A[3 + a] * q1;
    // keyframe 2
    im_map(R, t, X, Xc);
    im_error(Xc, o2, cam, e);
    im_huber(s2 * (e[0] * e[0] + e[1] * e[1]), huber, r0, r1);
    im_jacobians(R, Xc, cam, A, B);
    wo = r1 * s2; q0 = -s2 * e[0] * r1; q1 = -s2 * e[1] * r1;
    F += r0;
    lin[0] += wo * (A[0] * A[0] + A[3] * A[3]); lin[1] += wo * (A[0] * A[1] + A[3] * A[4]); lin[2] += wo * (A[0] * A[2] + A[3] * A[5]);
    lin[3] += wo * (A[1] * A[1] + A[4] * A[4]); lin[4] += wo * (A[1] * A[2] + A[4] * A[5]); lin[5] += wo * (A[2] * A[2] + A[5] * A[5]);
    for (int a = 0; a < 3; ++a) lin[6 + a] += A[a] * q0 + A[3 + a] * q1;
    int u = 0;
    for (int a = 0; a < 6; ++a) {
        for (int c = 0; c < 3; ++c) lin[9 + 3 * a + c] = wo * (B[a] * A[c] + B[6 + a] * A[3 + c]);
        for (int c = a; c < 6; ++c) acc[u++] += wo * (B[a] * B[c] + B[6 + a] * B[6 + c]);
        acc[21 + a] += B[a] * q0 + B[6 + a] * q1;
    }
    acc[27] += F;
}

// (Hll + lambda I)^-1 by cofactors (Eigen's fixed-size inverse, BlockSolver::solve's Dinv), symmetric storage
__host__ __device__ inline void im_dinv(const double lin[kImLin], double lambda, double Di[6])
{
    const double a = lin[0] + lambda, b = lin[1], c = lin[2], d = lin[3] + lambda, e = lin[4], f = lin[5] + lambda;
    const double c00 = d * f - e * e, c01 = e * c - b * f, c02 = b * e - d * c;
    const double id = 1.0 / (a * c00 + b * c01 + c * c02);
    Di[0] = c00 * id; Di[1] = c01 * id; Di[2] = c02 * id;
    Di[3] = (a * f - c * c) * id; Di[4] = (c * b - a * e) * id; Di[5] = (a * d - b * b) * id;
}

__host__ __device__ inline void im_sym3_mul(const double Di[6], const double v[3], double o[3])
{
    o[0] = Di[0] * v[0] + Di[1] * v[1] + Di[2] * v[2];
    o[1] = Di[1] * v[0] + Di[3] * v[1] + Di[4] * v[2];
    o[2] = Di[2] * v[0] + Di[4] * v[1] + Di[5] * v[2];
}

// The point's share of the Schur complement: acc[0..21) += Hpl Dinv Hpl^T (upper triangle), acc[21..27) += Hpl Dinv b_l
__host__ __device__ inline void im_schur(const double lin[kImLin], double lambda, double acc[27])
{
    double Di[6], db[3];
    im_dinv(lin, lambda, Di);
    im_sym3_mul(Di, lin + 6, db);
    const double *H = lin + 9;
    double BD[18];
    for (int a = 0; a < 6; ++a) {
        im_sym3_mul(Di, H + 3 * a, BD + 3 * a);         // (Dinv is symmetric: row a of Hpl Dinv)
        acc[21 + a] += H[3 * a] * db[0] + H[3 * a + 1] * db[1] + H[3 * a + 2] * db[2];
    }
    int u = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) acc[u++] += BD[3 * a] * H[3 * c] + BD[3 * a + 1] * H[3 * c + 1] + BD[3 * a + 2] * H[3 * c + 2];
}

// Back substitution of one point: x_l = Dinv (b_l - Hpl^T x_p); returns its share of computeScale, x_l . (lambda x_l + b_l)
__host__ __device__ inline double im_back(const double lin[kImLin], double lambda, const double xp[6], double xl[3])
{
    double Di[6], c[3] = { lin[6], lin[7], lin[8] };
    im_dinv(lin, lambda, Di);
    for (int a = 0; a < 6; ++a)
        for (int k = 0; k < 3; ++k) c[k] -= lin[9 + 3 * a + k] * xp[a];
    im_sym3_mul(Di, c, xl);
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s += xl[k] * (lambda * xl[k] + lin[6 + k]);
    return s;
}

// total order of doubles by bit pattern: a < b as numbers implies key(a) < key(b); -0 below +0, a positive NaN above +inf
__host__ __device__ inline uint64_t im_order_key(double v)
{
    union { double d; uint64_t u; } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : c.u | 0x8000000000000000ull;
}

}  // namespace movba
