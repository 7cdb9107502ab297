// Marginal covariances of a solved window: the device pass behind movba_lba_marginals (marginals.cpp, include/movba.h).
//
// g2o's SparseOptimizer::computeMarginals, Ceres' Covariance and GTSAM's Marginals read the same thing out of a solved problem:
// blocks of the inverse of the normal matrix H at the estimate.  H here is the matrix the LM kernels build at the window's
// final state (every edge, weight rho'(chi2) inv_sigma2, stereo rows, cameras by keyframe) with `damping` on its diagonal.
// With the reduced system S = Hpp - Hpl Hll^-1 Hlp of the direct solver (at lambda = damping) and its factor S = L L^T:
//     pose block of free keyframe i  = (S^-1)_ii,    S^-1 = W^T W,  W = L^-1
//     point block of map point l     = D + D (sum over free observers i, j of l of B_il^T (S^-1)_ij B_jl) D,
//                                      D = (Hll_l + damping I)^-1,  B_il = the 6 x 3 block of Hpl of the edge (i, l)
// The chain, on the handle's stream:
//     k_marg_ctrl      the run's controller copied into a scratch one (lambda = damping, done = 0)
//     k_point<false>, k_schur, k_dense_assemble, k_chol_step
//                      the LM's own linearisation, schur pass, assembly and factorisation, unchanged, through the scratch
//                      controller (kernels.hip, dense_solve.hip)
//     k_marg_trinv     L(I, I)^-1 of every diagonal factor tile (one wave per tile)
//     k_marg_w         W = L^-1, one workgroup per tile column J: W(J, J) = L(J, J)^-1, then for I = J + 1, J + 2, ...
//                      W(I, J) = -L(I, I)^-1 sum_{K = J}^{I-1} L(I, K) W(K, J)
//     k_marg_sigma     the lower tiles of W^T W, one workgroup per tile: sigma(I, J) = sum_{K >= I} W(K, I)^T W(K, J)
//     k_marg_out       pose blocks from the diagonal tiles in caller order (hidx: the covisibility renumbering is undone
//                      there); point blocks, 8 lanes per map point, B_il rebuilt from the linearisation's edge records
// The tile products are 48 x 48 x 48 on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, as in dense_tile.h).  Every sum runs in
// a fixed order, so results are bit-reproducible; the inverse kernels leave at once after a failed factorisation.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dense_tile.h"
#include "device_math.h"
#include "device_types.h"
#include "kernels.h"
#include "marginals.h"

namespace movba {

using namespace dense;

namespace {

constexpr int kMargThreads = kStepThreads;      // 4 waves: the nine 16 x 16 MFMA tiles of a product dealt round-robin
constexpr int kPointLanes = 8;                  // lanes per map point in k_marg_out
constexpr int kPointsPerMargBlock = kMargThreads / kPointLanes;

// element r (0..3) of a wave's accumulator u: MFMA tile q = wave + 4 u of the 3 x 3 grid, C/D layout of the instruction
__device__ __forceinline__ int acc_row(int q, int lane, int r) { return (q / 3) * 16 + (lane >> 4) + 4 * r; }
__device__ __forceinline__ int acc_col(int q, int lane) { return (q % 3) * 16 + (lane & 15); }

// global tile (row-major) -> LDS image of its transpose
__device__ __forceinline__ void load_tile_t(const double *__restrict__ g, double *sm, int tid)
{
    for (int e = tid; e < NB * NB; e += kMargThreads) {
        const int r = e / NB, c = e - r * NB;
        sm[c * LD + r] = g[e];
    }
}

__device__ __forceinline__ dbl4 dzero() { return dbl4{ 0.0, 0.0, 0.0, 0.0 }; }

// element (r, c) of the symmetric S^-1 from its lower tiles
__device__ __forceinline__ double sig_at(const double *sig, int r, int c)
{
    if (r < c) { const int t = r; r = c; c = t; }
    const int I = r / NB, J = c / NB;
    return sig[tile_off(I, J) + (size_t)(r - I * NB) * NB + (c - J * NB)];
}

// B_il^T (3 x 6) of grouped edge g at the state the linearisation left (its edge record: camera-frame point and weight), the
// Jacobian rows of k_schur's edge_rows (edge_model.h) written out: through the call two v_mul_f64 of k_marg_out swap their
// operands, and movba_lba_marginals measured slower at cfg2; false for an edge of a keyframe outside the system (fixed)
__device__ __forceinline__ bool edge_g(const DevWindow &w, const DevState &S, int g, double (&G)[3][6], int &h)
{
    const int ip = w.g_pose[g];
    h = w.hidx[ip];
    if (h < 0) return false;
    const int sl = w.slot[g];
    const double4 rc = *reinterpret_cast<const double4 *>(S.erecA + 4 * (size_t)sl);
    const double *R = S.Rt + 12 * (size_t)ip;
    double fx = w.fx, fy = w.fy, bf = w.bf;
    if (w.kcam) { const double *k = w.kcam + 8 * (size_t)ip; fx = k[0]; fy = k[1]; bf = k[4]; }
    const bool st = w.stereo && w.obs_r[g] >= 0.0;
    const double x = rc.x, y = rc.y, z = rc.z, wg = rc.w;
    const double iz = fast_rcp(z);
    const double a00 = -fx * iz, a02 = fx * x * iz * iz, a11 = -fy * iz, a12 = fy * y * iz * iz;
    double P[3][3], C[3][6];
#pragma unroll
    for (int q = 0; q < 3; ++q) { P[0][q] = a00 * R[q] + a02 * R[6 + q]; P[1][q] = a11 * R[3 + q] + a12 * R[6 + q]; }
    C[0][0] = a02 * y; C[0][1] = a00 * z - a02 * x; C[0][2] = -a00 * y; C[0][3] = a00; C[0][4] = 0.0; C[0][5] = a02;
    C[1][0] = -a11 * z + a12 * y; C[1][1] = -a12 * x; C[1][2] = a11 * x; C[1][3] = 0.0; C[1][4] = a11; C[1][5] = a12;
    const double m = st ? 1.0 : 0.0;
    const double c00 = m * a00, c02 = m * (a02 - bf * iz * iz);
#pragma unroll
    for (int q = 0; q < 3; ++q) P[2][q] = c00 * R[q] + c02 * R[6 + q];
    C[2][0] = c02 * y; C[2][1] = c00 * z - c02 * x; C[2][2] = -c00 * y; C[2][3] = c00; C[2][4] = 0.0; C[2][5] = c02;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int a = 0; a < 6; ++a) G[q][a] = wg * ((P[0][q] * C[0][a] + P[1][q] * C[1][a]) + P[2][q] * C[2][a]);
    return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// k_marg_ctrl: the run's controller -> the scratch controller, with lambda = damping and done = 0 (k_dense_assemble and
// k_chol_step return at once on done == 1, which the run leaves behind); the flag words cleared
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMargThreads) void k_marg_ctrl(MargDev m)
{
    static_assert(sizeof(Ctrl) % 8 == 0, "the controller is copied in 8-byte words");
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(m.run_ctrl);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(m.ctrl);
    for (int k = threadIdx.x; k < (int)(sizeof(Ctrl) / 8); k += kMargThreads) dst[k] = src[k];
    __syncthreads();
    if (threadIdx.x == 0) { m.ctrl->lambda = m.damping; m.ctrl->done = 0; m.flags[0] = 0; m.flags[1] = 0; }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_marg_trinv: L(I, I)^-1 for tile I = blockIdx.x.  One wave; lane c solves L x = e_c by forward substitution with the
// factor's rows read from LDS as broadcasts (the zeros above the diagonal come out exact).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_marg_trinv(MargDev m)
{
    __shared__ double Ls[NB * LD], rd[NB];
    if (*m.w.dense.fail) return;
    const int I = blockIdx.x, lane = threadIdx.x;
    const double *g = m.w.dense.diagL + (size_t)I * NB * NB;
    for (int e = lane; e < NB * NB; e += 64) { const int r = e / NB, c = e - r * NB; Ls[r * LD + c] = g[e]; }
    __syncthreads();
    if (lane < NB) rd[lane] = 1.0 / Ls[lane * LD + lane];
    __syncthreads();
    const int c = lane < NB ? lane : NB - 1;        // lanes 48..63 shadow column 47 (never stored)
    double x[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        double s = r == c ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < r; ++k) s -= Ls[r * LD + k] * x[k];
        x[r] = s * rd[r];
    }
    if (lane < NB) {
        double *out = m.linv + (size_t)I * NB * NB;
#pragma unroll
        for (int r = 0; r < NB; ++r) out[r * NB + c] = x[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_marg_w: tile column J = blockIdx.x of W = L^-1, block row after block row (each needs the ones above it in its column;
// no column needs another, so the launch has no waits).  The column's tiles go to global memory as they are finished and
// come back through L2 as operands.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMargThreads) void k_marg_w(MargDev m)
{
    __shared__ double As[NB * LD], Bs[NB * LD];
    const DenseSys &ds = m.w.dense;
    if (*ds.fail) return;
    const int J = blockIdx.x, nt = ds.ntile, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const double2 *src = reinterpret_cast<const double2 *>(m.linv + (size_t)J * NB * NB);
        double2 *dst = reinterpret_cast<double2 *>(m.W + tile_off(J, J));
        for (int e = tid; e < NB * NB / 2; e += kMargThreads) dst[e] = src[e];
    }
    for (int I = J + 1; I < nt; ++I) {
        dbl4 acc[3] = { dzero(), dzero(), dzero() };
        for (int K = J; K < I; ++K) {
            __threadfence();                        // this workgroup's stores of W(K, J) are visible to all of its waves ...
            __syncthreads();                        // ... and every wave is done with the previous operands
            load_tile(ds.tiles + tile_off(I, K), As, tid);
            load_tile_t(m.W + tile_off(K, J), Bs, tid);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int q = wv + 4 * u;
                if (q < 9) acc[u] = tile_mfma<true>(As, Bs, q / 3, q % 3, lane, acc[u]);
            }
        }
        __syncthreads();
        // acc = -sum L(I, K) W(K, J): its transpose is the B operand of the product with L(I, I)^-1
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int q = wv + 4 * u;
            if (q < 9) {
                const int cc = acc_col(q, lane);
                Bs[cc * LD + acc_row(q, lane, 0)] = acc[u].x; Bs[cc * LD + acc_row(q, lane, 1)] = acc[u].y;
                Bs[cc * LD + acc_row(q, lane, 2)] = acc[u].z; Bs[cc * LD + acc_row(q, lane, 3)] = acc[u].w;
            }
        }
        load_tile(m.linv + (size_t)I * NB * NB, As, tid);
        __syncthreads();
        double *out = m.W + tile_off(I, J);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int q = wv + 4 * u;
            if (q < 9) {
                const dbl4 v = tile_mfma<false>(As, Bs, q / 3, q % 3, lane, dzero());
                const int cc = acc_col(q, lane);
                out[acc_row(q, lane, 0) * NB + cc] = v.x; out[acc_row(q, lane, 1) * NB + cc] = v.y;
                out[acc_row(q, lane, 2) * NB + cc] = v.z; out[acc_row(q, lane, 3) * NB + cc] = v.w;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_marg_sigma: lower tile (I, J) of S^-1 = W^T W, one workgroup per tile (linear index as k_dense_assemble's)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMargThreads) void k_marg_sigma(MargDev m)
{
    __shared__ double As[NB * LD], Bs[NB * LD];
    const DenseSys &ds = m.w.dense;
    if (*ds.fail) return;
    const int tid = threadIdx.x, lane = tid & 63, nt = ds.ntile;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    int I = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
    while (I * (I + 1) / 2 > (int)blockIdx.x) --I;
    const int J = (int)blockIdx.x - I * (I + 1) / 2;
    dbl4 acc[3] = { dzero(), dzero(), dzero() };
    for (int K = I; K < nt; ++K) {
        if (K > I) __syncthreads();
        load_tile_t(m.W + tile_off(K, I), As, tid);
        load_tile_t(m.W + tile_off(K, J), Bs, tid);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int q = wv + 4 * u;
            if (q < 9) acc[u] = tile_mfma<false>(As, Bs, q / 3, q % 3, lane, acc[u]);
        }
    }
    double *out = m.sig + tile_off(I, J);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int q = wv + 4 * u;
        if (q < 9) {
            const int cc = acc_col(q, lane);
            out[acc_row(q, lane, 0) * NB + cc] = acc[u].x; out[acc_row(q, lane, 1) * NB + cc] = acc[u].y;
            out[acc_row(q, lane, 2) * NB + cc] = acc[u].z; out[acc_row(q, lane, 3) * NB + cc] = acc[u].w;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_marg_out: workgroups [0, pose_blocks) gather the pose blocks (one caller keyframe per thread), the others take 32 map
// points each, 8 lanes per point: every point's damped Hll is checked for positive definiteness (flags[1]); with want_points
// lane s takes the point's edges a = s, s + 8, ... and, for each, the pairs (a, b >= a) of its free observers.  Every block is
// written from its lower triangle, so it is exactly symmetric.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMargThreads) void k_marg_out(MargDev m)
{
    const DevWindow &w = m.w;
    const int tid = threadIdx.x;
    const bool fail = *w.dense.fail != 0;
    const double nan = __builtin_nan("");
    if (blockIdx.x == 0 && tid == 0 && fail) m.flags[0] = 1;
    if ((int)blockIdx.x < m.pose_blocks) {
        const int i = blockIdx.x * kMargThreads + tid;
        if (fail || i >= w.NP) return;
        double *o = m.pose_out + 36 * (size_t)i;
        const int h = w.hidx[i];
        if (h < 0) {            // fixed (zeroed by the host) or without edges: not in the system
            for (int k = 0; k < 36; ++k) o[k] = nan;
            return;
        }
        const int r0 = 6 * h, T = r0 / NB, off = r0 - T * NB;
        const double *t = m.sig + tile_off(T, T);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                const double v = t[(size_t)(off + a) * NB + off + b];
                o[6 * a + b] = v; o[6 * b + a] = v;
            }
        return;
    }
    const int sub = tid & (kPointLanes - 1);
    const int l = ((int)blockIdx.x - m.pose_blocks) * kPointsPerMargBlock + tid / kPointLanes;
    if (l >= w.P) return;                           // (the 8 lanes of a point take every branch below together)
    const DevState &S = w.st[m.ctrl->cur];
    const int begin = w.pt_start[l], end = w.pt_start[l + 1];
    double *o = m.point_out + 9 * (size_t)l;
    if (end <= begin) {
        if (m.want_points && !fail && sub == 0) for (int k = 0; k < 9; ++k) o[k] = nan;
        return;
    }
    double H[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) H[k] = S.Hll[6 * (size_t)l + k];
    H[0] += m.damping; H[3] += m.damping; H[5] += m.damping;
    // leading minors (xx xy xz yy yz zz)
    const double m2 = H[0] * H[3] - H[1] * H[1];
    const double det = H[0] * (H[3] * H[5] - H[4] * H[4]) - H[1] * (H[1] * H[5] - H[4] * H[2]) + H[2] * (H[1] * H[4] - H[3] * H[2]);
    const bool pd = H[0] > 0.0 && m2 > 0.0 && det > 0.0 && isfinite(H[0]) && isfinite(m2) && isfinite(det);
    if (!pd) { if (sub == 0) m.flags[1] = 1; return; }
    if (!m.want_points || fail) return;
    double D[6];
    inv3sym(H, D);                                  // (the schur pass's own inverse: the point blocks see the D that S was built with)
    // T = sum_{a, b} G_a sigma_ab G_b^T, lower triangle: (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
    double t6[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int a = begin + sub; a < end; a += kPointLanes) {
        double Ga[3][6];
        int ha;
        if (!edge_g(w, S, a, Ga, ha)) continue;
        for (int b = a; b < end; ++b) {
            double Gb[3][6];
            int hb = ha;
            if (b == a) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int k = 0; k < 6; ++k) Gb[q][k] = Ga[q][k];
            } else if (!edge_g(w, S, b, Gb, hb)) continue;
            double U[3][6];
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int k = 0; k < 6; ++k) U[q][k] = 0.0;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double s = sig_at(m.sig, 6 * ha + p, 6 * hb + k);
#pragma unroll
                    for (int q = 0; q < 3; ++q) U[q][k] += Ga[q][p] * s;
                }
            double M[3][3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) s += U[q][k] * Gb[r][k];
                    M[q][r] = s;
                }
            const bool same = b == a;
            t6[0] += same ? M[0][0] : M[0][0] + M[0][0];
            t6[1] += same ? M[1][0] : M[1][0] + M[0][1];
            t6[2] += same ? M[1][1] : M[1][1] + M[1][1];
            t6[3] += same ? M[2][0] : M[2][0] + M[0][2];
            t6[4] += same ? M[2][1] : M[2][1] + M[1][2];
            t6[5] += same ? M[2][2] : M[2][2] + M[2][2];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) t6[k] = group_sum_dpp(t6[k], kPointLanes);
    if (sub != 0) return;
    // cov = D + D T D
    const double Dm[3][3] = { { D[0], D[1], D[2] }, { D[1], D[3], D[4] }, { D[2], D[4], D[5] } };
    const double Tm[3][3] = { { t6[0], t6[1], t6[3] }, { t6[1], t6[2], t6[4] }, { t6[3], t6[4], t6[5] } };
    double DT[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r < 3; ++r) DT[q][r] = (Dm[q][0] * Tm[0][r] + Dm[q][1] * Tm[1][r]) + Dm[q][2] * Tm[2][r];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r <= q; ++r) {
            const double v = Dm[q][r] + ((DT[q][0] * Dm[0][r] + DT[q][1] * Dm[1][r]) + DT[q][2] * Dm[2][r]);
            o[3 * q + r] = v; o[3 * r + q] = v;
        }
}

hipError_t launch_marginals(const MargDev &m, hipStream_t s)
{
    hipLaunchKernelGGL(k_marg_ctrl, dim3(1), dim3(kMargThreads), 0, s, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_linearize(m.w, s)) != hipSuccess) return e;
    if (m.w.nitems > 0 && (e = launch_schur(m.w, 0, s)) != hipSuccess) return e;
    if ((e = launch_dense_factor(m.w, s)) != hipSuccess) return e;
    const int nt = m.w.dense.ntile;
    hipLaunchKernelGGL(k_marg_trinv, dim3(nt), dim3(64), 0, s, m);
    hipLaunchKernelGGL(k_marg_w, dim3(nt), dim3(kMargThreads), 0, s, m);
    hipLaunchKernelGGL(k_marg_sigma, dim3(nt * (nt + 1) / 2), dim3(kMargThreads), 0, s, m);
    const int point_blocks = (m.w.P + kPointsPerMargBlock - 1) / kPointsPerMargBlock;
    hipLaunchKernelGGL(k_marg_out, dim3(m.pose_blocks + point_blocks), dim3(kMargThreads), 0, s, m);
    return hipGetLastError();
}

}  // namespace movba
