// movba_init_map (include/movba.h): the two-keyframe bundle adjustment, median depth and rescaling of
// Tracking::CreateInitialMapMonocular (Tracking.cc:688-717) for many frame pairs, one workgroup per pair and
// the whole Levenberg-Marquardt loop inside one launch (as k_pose_opt).  With keyframe 1 fixed the reduced system is one 6 x 6
// block: every thread owns the points k = thread, thread + 256, ... for the whole launch (their estimate, backup and
// linearisation live in device scratch that no other thread touches), the workgroup meets in one fixed-tree reduction per outer
// iteration (the build) plus two per trial (Schur complement; cost and scale), and every thread then solves the 6 x 6 system
// and takes the accept / reject decision redundantly from the same bits.
// Per-point arithmetic: init_map.h.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "device_math.h"
#include "init_map.h"
#include "lm_rule.h"
#include "movba.h"

namespace movba {

namespace {

constexpr int kT = kImThreads;
constexpr int kW = kT / 64;

__device__ __forceinline__ void load3(const double *a, size_t cap, int k, double v[3])
{
    v[0] = a[k]; v[1] = a[cap + k]; v[2] = a[2 * cap + k];
}
__device__ __forceinline__ void store3(double *a, size_t cap, int k, const double v[3])
{
    a[k] = v[0]; a[cap + k] = v[1]; a[2 * cap + k] = v[2];
}

}  // namespace

__global__ __launch_bounds__(kImThreads) void k_init_map(ImDev d)
{
    __shared__ __attribute__((aligned(16))) double red[kRedLds<kW>];      // reduce_all (device_math.h)
    __shared__ double s_med;
    __shared__ int s_cnt[kW];
    const ImPair p = d.pairs[blockIdx.x];
    const int n = p.n;
    if (n == 0) return;                                     // (no used match: the host fills the result in)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t m0 = (size_t)p.m0, cap = (size_t)p.cap;
    const uint8_t *use = d.use + m0;
    int32_t *idx = d.idx + p.s0;
    double *X = d.X + 3 * p.s0, *Xbk = d.Xbk + 3 * p.s0, *lin = d.lin + (size_t)kImLin * p.s0;
    const double cam[4] = { p.fx, p.fy, p.cx, p.cy };
    const double huber = p.huber;
    const double nan = __builtin_nan("");

    // 1. the used matches, compacted in ascending order (tiles of one workgroup; a tile's offsets from the waves' ballots)
    int nu = 0;
    for (int t0 = 0; t0 < n; t0 += kT) {
        const int i = t0 + tid;
        const bool f = i < n && use[i] != 0;
        const unsigned long long b = __ballot(f);
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < kW; ++q) { const int c = s_cnt[q]; before += q < wave ? c : 0; total += c; }
        const int at = nu + before + __popcll(b & ((1ull << lane) - 1ull));
        if (f && at < p.cap) idx[at] = i;                   // (at < cap always: the host counted the same bytes)
        nu += total;
        __syncthreads();
    }
    if (nu > p.cap) nu = p.cap;
    for (int k = tid; k < nu; k += kT) {
        const double *src = d.pts + 3 * (m0 + (size_t)idx[k]);
        const double v[3] = { src[0], src[1], src[2] };
        store3(X, cap, k, v);
    }

    // 2. Levenberg-Marquardt; every thread carries the same pose, lambda and counters
    double pose[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) pose[e] = p.pose2[e];
    quat_normalize_exact(pose);
    const int max_trials = p.max_trials > 0 ? p.max_trials : 10;
    double lambda = 0.0, ni = 2.0, cost0 = 0.0, R[9];
    int flip = 0, iters_done = 0, n_solves = 0, last_rejected = 0, n_chol_fail = 0, n_trace = 0;
    bool ok = true;
    double *trace = p.trace;
    for (int it = 0; it < p.max_iters && ok; ++it) {
        // buildSystem at the current estimate: per point Hll, b_l, Hpl to scratch; Hpp, b_p and F0 summed over the workgroup
        quat_to_R(pose, R);
        double acc[28];
#pragma unroll
        for (int e = 0; e < 28; ++e) acc[e] = 0.0;
        double md = 0.0;
        for (int k = tid; k < nu; k += kT) {
            const size_t m = m0 + (size_t)idx[k];
            double x[3], l[kImLin];
            load3(X, cap, k, x);
            im_linearize(R, pose + 4, cam, huber, x, d.obs1 + 2 * m, d.obs2 + 2 * m, d.sig1[m], d.sig2[m], l, acc);
#pragma unroll
            for (int e = 0; e < kImLin; ++e) lin[(size_t)e * cap + k] = l[e];
            md = fmax(fmax(fabs(l[0]), fabs(l[3])), fmax(fabs(l[5]), md));
        }
        reduce_all<kW>(acc, red, flip);
        double F0 = acc[27];
        if (it == 0) {
            // computeLambdaInit over the pose block and the point blocks
            md = block_reduce<kW, true>(md, red + 2 * kW * kRedMax);
#pragma unroll
            for (int a = 0; a < 6; ++a) md = fmax(fabs(acc[ut6(a, a)]), md);
            lambda = lm_lambda_init(md);
            ni = 2.0;
            cost0 = F0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            // Schur complement and reduced right-hand side
            double sc[27];
#pragma unroll
            for (int e = 0; e < 27; ++e) sc[e] = 0.0;
            for (int k = tid; k < nu; k += kT) {
                double l[kImLin];
#pragma unroll
                for (int e = 0; e < kImLin; ++e) l[e] = lin[(size_t)e * cap + k];
                im_schur(l, lambda, sc);
            }
            reduce_all<kW>(sc, red, flip);
            double Su[21], bS[6], xp[6];
#pragma unroll
            for (int e = 0; e < 21; ++e) Su[e] = acc[e] - sc[e];
#pragma unroll
            for (int a = 0; a < 6; ++a) bS[a] = acc[21 + a] - sc[21 + a];
            const bool ok2 = solve6(Su, lambda, bS, xp);
            double trial[7], Rt[9];
#pragma unroll
            for (int e = 0; e < 7; ++e) trial[e] = pose[e];
            if (ok2) se3_oplus(xp, pose, trial);
            quat_to_R(trial, Rt);
            // back substitution, update (the old estimate goes to the backup) and the cost at the trial estimate
            double fs[2] = { 0.0, 0.0 };
            for (int k = tid; k < nu; k += kT) {
                const size_t m = m0 + (size_t)idx[k];
                double x[3], c2[2];
                load3(X, cap, k, x);
                if (ok2) {
                    double l[kImLin], xl[3];
#pragma unroll
                    for (int e = 0; e < kImLin; ++e) l[e] = lin[(size_t)e * cap + k];
                    fs[1] += im_back(l, lambda, xp, xl);
                    store3(Xbk, cap, k, x);
                    x[0] += xl[0]; x[1] += xl[1]; x[2] += xl[2];
                    store3(X, cap, k, x);
                }
                fs[0] += im_cost(Rt, trial + 4, cam, huber, x, d.obs1 + 2 * m, d.obs2 + 2 * m, d.sig1[m], d.sig2[m], c2);
            }
            reduce_all<kW>(fs, red, flip);
            // (the rest of the step rule - lm_gain, lm_accept, lm_update and the two loop conditions of lm_rule.h - written out: through
            //  the calls the kernel's registers are numbered otherwise or its instructions change, and movba_init_map measured slower)
            double F1 = fs[0], scale = 0.0;
            if (ok2) {
#pragma unroll
                for (int a = 0; a < 6; ++a) scale += xp[a] * (lambda * xp[a] + acc[21 + a]);
                scale += fs[1];
            } else {
                F1 = DBL_MAX;
                ++n_chol_fail;
            }
            scale += 1e-3;
            rho = (F0 - F1) / scale;
            const double lambda_tried = lambda, F0_tried = F0;
            const bool accept = rho > 0.0 && isfinite(F1);
            bool lambda_ok = true;
            if (accept) {
                double alpha = 2.0 * rho - 1.0;
                alpha = 1.0 - alpha * alpha * alpha;
                alpha = fmin(alpha, 2.0 / 3.0);
                lambda *= fmax(1.0 / 3.0, alpha);
                ni = 2.0;
                F0 = F1;
#pragma unroll
                for (int e = 0; e < 7; ++e) pose[e] = trial[e];
            } else {
                lambda *= ni;
                ni *= 2.0;
                if (ok2)
                    for (int k = tid; k < nu; k += kT) {
                        double x[3];
                        load3(Xbk, cap, k, x);
                        store3(X, cap, k, x);
                    }
                lambda_ok = isfinite(lambda);
            }
            if (trace && tid == 0 && n_trace < MOVBA_MAX_TRACE) {
                trace[1 + n_trace] = lambda_tried; trace[1 + MOVBA_MAX_TRACE + n_trace] = F0_tried;
                trace[1 + 2 * MOVBA_MAX_TRACE + n_trace] = F1; trace[1 + 3 * MOVBA_MAX_TRACE + n_trace] = rho;
                trace[1 + 4 * MOVBA_MAX_TRACE + n_trace] = accept ? 1.0 : 0.0;
            }
            if (n_trace < MOVBA_MAX_TRACE) ++n_trace;
            last_rejected = accept ? 0 : 1;
            ++n_solves;
            ++qmax;
            if (!lambda_ok) break;
        } while (rho < 0.0 && qmax < max_trials);
        iters_done = it + 1;
        if (qmax == max_trials || rho == 0.0 || !isfinite(lambda)) ok = false;      // Terminate
    }

    // cost and chi2 at the returned estimate; the depths go to the (now free) backup array for the median
    quat_to_R(pose, R);
    double fc[1] = { 0.0 };
    double *z = Xbk;
    for (int k = tid; k < nu; k += kT) {
        const int i = idx[k];
        const size_t m = m0 + (size_t)i;
        double x[3], c2[2];
        load3(X, cap, k, x);
        fc[0] += im_cost(R, pose + 4, cam, huber, x, d.obs1 + 2 * m, d.obs2 + 2 * m, d.sig1[m], d.sig2[m], c2);
        if (p.chi2) { p.chi2[2 * (size_t)i] = c2[0]; p.chi2[2 * (size_t)i + 1] = c2[1]; }
        z[k] = x[2];
    }
    reduce_all<kW>(fc, red, flip);                               // (its barrier also publishes z to the workgroup)
    const double cost = fc[0];
    if (p.max_iters == 0) cost0 = cost;

    // 3. median depth: the element of rank (nu - 1) / 2 in the total order (key, match order); exactly one thread finds it
    const int kmed = (nu - 1) / 2;
    for (int k = tid; k < nu; k += kT) {
        const uint64_t mine = im_order_key(z[k]);
        int rank = 0;
        for (int j = 0; j < nu; ++j) {
            const uint64_t o = im_order_key(z[j]);
            rank += (o < mine || (o == mine && j < k)) ? 1 : 0;
        }
        if (rank == kmed) s_med = z[k];
    }
    __syncthreads();
    const double med = s_med;

    // 4. the test of Tracking.cc:694 and the rescaling
    const int outcome = med < 0.0 ? MOVBA_IM_NEG_DEPTH : (nu < p.min_tracked ? MOVBA_IM_FEW_TRACKED : MOVBA_IM_OK);
    const double inv = outcome == MOVBA_IM_OK ? 1.0 / med : 1.0;
    for (int k = tid; k < nu; k += kT) {
        double x[3];
        load3(X, cap, k, x);
        double *dst = p.points + 3 * (size_t)idx[k];
        dst[0] = x[0] * inv; dst[1] = x[1] * inv; dst[2] = x[2] * inv;
    }
    for (int i = tid; i < n; i += kT)
        if (use[i] == 0) {
            double *dst = p.points + 3 * (size_t)i;
            dst[0] = nan; dst[1] = nan; dst[2] = nan;
            if (p.chi2) { p.chi2[2 * (size_t)i] = nan; p.chi2[2 * (size_t)i + 1] = nan; }
        }
    if (tid == 0) {
        double *o = p.out;
        o[0] = pose[0]; o[1] = pose[1]; o[2] = pose[2]; o[3] = pose[3];
        o[4] = pose[4] * inv; o[5] = pose[5] * inv; o[6] = pose[6] * inv;
        o[7] = med; o[8] = outcome; o[9] = nu; o[10] = iters_done; o[11] = n_solves; o[12] = last_rejected; o[13] = n_chol_fail;
        o[14] = lambda; o[15] = cost0; o[16] = cost;
        if (trace) trace[0] = n_trace;
    }
}

hipError_t launch_init_map(const ImDev &d, hipStream_t s)
{
    if (d.n_pairs > 0) hipLaunchKernelGGL(k_init_map, dim3(d.n_pairs), dim3(kImThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
