// The pinhole edge of the reference as the kernels evaluate it: camera-frame point, reprojection residual and chi2, Huber
// kernel, Jacobian rows.
//   EdgeSE3ProjectXYZ::computeError   include/OptimizableTypes.h:103-109
//   EdgeSE3ProjectXYZ::linearizeOplus src/OptimizableTypes.cpp:158-180
//   Pinhole::project / projectJac     src/CameraModels/Pinhole.cpp:36-43, 77-88
// The library is built with -ffp-contract=on (a product fuses with the add of the same statement only), so these bodies keep
// the statements of the kernels they were taken from, in their order: a helper that re-associated would round otherwise.
// Spellings that round differently stay where they are (the sqrt form of pose_kernels.hip's cost, init_map.h's im_huber /
// im_error, which the host stand-in shares).
#pragma once
#include <cfloat>

#include "device_math.h"

namespace movba {

// The camera of an edge is its keyframe's (src/Optimizer.cc:664: e->pCamera = pKFi->mpCamera; :690-695: e->fx .. e->bf from
// pKFi): one set of intrinsics for the whole window in every shipped MoV-SLAM configuration (DevWindow::fx ..), a table by
// keyframe when the caller hands one (movba_lba_desc::cam_kf / bf_kf).
struct Cam { double fx, fy, cx, cy, bf; };

// Xc = R X + t: R row-major in Rt[0..8], t in Rt[9..11]
__device__ __forceinline__ void cam_point(const double *Rt, const double *X, double &x, double &y, double &z)
{
    x = Rt[0] * X[0] + Rt[1] * X[1] + Rt[2] * X[2] + Rt[9];
    y = Rt[3] * X[0] + Rt[4] * X[1] + Rt[5] * X[2] + Rt[10];
    z = Rt[6] * X[0] + Rt[7] * X[1] + Rt[8] * X[2] + Rt[11];
}

// chi2 = e^T (om I) e of the monocular rows by IEEE division, as Pinhole::project divides (z = 0 gives inf)
// (CAM: a Cam, or what else carries fx, fy, cx, cy - PoseDev: the intrinsics are read where the statements name them)
template <class CAM>
__device__ __forceinline__ double edge_chi2_div(const CAM &cm, double x, double y, double z, const double *ob, double om)
{
    const double e0 = ob[0] - (cm.fx * x / z + cm.cx), e1 = ob[1] - (cm.fy * y / z + cm.cy);
    return e0 * (om * e0) + e1 * (om * e1);
}

// The same by ONE reciprocal iz of z (fast_rcp / fast_rcp_zero_safe, the caller's choice) and multiplications: an fp64
// division is a ~25-instruction sequence, and the projection and its Jacobian would take six of them.  u, v: the projection
// before the principal point is added, which the Jacobian rows reuse.
template <class CAM>
__device__ __forceinline__ double edge_res_rcp(const CAM &cm, double x, double y, double iz, const double *ob, double om,
                                              double &u, double &v, double &e0, double &e1)
{
    u = cm.fx * x * iz; v = cm.fy * y * iz;
    e0 = ob[0] - (u + cm.cx);
    e1 = ob[1] - (v + cm.cy);
    return e0 * (om * e0) + e1 * (om * e1);
}
// the stereo row: adds its term to chi2 and returns its residual
__device__ __forceinline__ double edge_res_rcp_stereo(const Cam &cm, double u, double iz, double ur, double om, double &chi2)
{
    const double e2 = ur - (u + cm.cx - cm.bf * iz);
    chi2 += e2 * (om * e2);
    return e2;
}

// RobustKernelHuber::robustify in its rsqrt form: rho0 and rho1 of chi2 (delta <= 0: no kernel; dsqr = delta^2).
// sqrt(chi2) = chi2 / sqrt(chi2): for chi2 = inf - a point on the keyframe's z = 0 plane - the product is inf * 0; g2o takes
// sqrt(inf) = inf there, an infinite cost, not NaN.
__device__ __forceinline__ void huber_rs(double chi2, double delta, double dsqr, double &rho0, double &rho1)
{
    rho0 = chi2; rho1 = 1.0;
    if (delta > 0.0 && !(chi2 <= dsqr)) {
        const double rs = rsqrt(chi2), sq = chi2 > DBL_MAX ? chi2 : chi2 * rs;
        rho0 = 2.0 * sq * delta - dsqr;
        rho1 = delta * rs;
    }
}

// Jacobian rows of one edge from its cached camera-frame point: P = J_point rows (-Jpi R), C = J_pose rows
// (-Jpi [ -[Xc]x | I ]).  NR = 2: monocular edge (src/OptimizableTypes.cpp:158-180); NR = 3 adds the stereo row of
// g2o::EdgeStereoSE3ProjectXYZ (built at src/Optimizer.cc:673-705), zeroed for the monocular edges of a mixed window.
// (A division-free variant on normalised records (x / z, y / z, 1 / z) with the structural zeros of C skipped was 20 %
//  SLOWER, solo and batched: the kernel then needs all 256 registers and the compiler schedules its gathers worse.)
template <int NR>
__device__ __forceinline__ void edge_rows(const Cam &cm, double x, double y, double z, const double R[9], bool stereo,
                                          double (&P)[NR][3], double (&C)[NR][6])
{
    const double iz = fast_rcp(z);
    const double a00 = -cm.fx * iz, a02 = cm.fx * x * iz * iz, a11 = -cm.fy * iz, a12 = cm.fy * y * iz * iz;
#pragma unroll
    for (int q = 0; q < 3; ++q) { P[0][q] = a00 * R[q] + a02 * R[6 + q]; P[1][q] = a11 * R[3 + q] + a12 * R[6 + q]; }
    C[0][0] = a02 * y; C[0][1] = a00 * z - a02 * x; C[0][2] = -a00 * y; C[0][3] = a00; C[0][4] = 0.0; C[0][5] = a02;
    C[1][0] = -a11 * z + a12 * y; C[1][1] = -a12 * x; C[1][2] = a11 * x; C[1][3] = 0.0; C[1][4] = a11; C[1][5] = a12;
    if (NR == 3) {
        const double m = stereo ? 1.0 : 0.0;
        const double c00 = m * a00, c02 = m * (a02 - cm.bf * iz * iz);
#pragma unroll
        for (int q = 0; q < 3; ++q) P[NR - 1][q] = c00 * R[q] + c02 * R[6 + q];
        C[NR - 1][0] = c02 * y; C[NR - 1][1] = c00 * z - c02 * x; C[NR - 1][2] = -c00 * y;
        C[NR - 1][3] = c00; C[NR - 1][4] = 0.0; C[NR - 1][5] = c02;
    }
}

}  // namespace movba
