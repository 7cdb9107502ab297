// The kernels of movba_two_view and movba_two_view_lo (include/movba.h); the arithmetic is two_view_math.h.
//   k_tv_hyp      one workgroup per (pair, sample), found by binary search over the prefix of the pairs' sample counts (as
//                 k_pose_hyp_b finds its frame).  The five-point solve runs over the whole workgroup with its tables in LDS
//                 (tv_five_point: the lanes own the columns of the 10 x 20 elimination, the intervals of the root search and
//                 the roots); then the four waves score the candidates over the pair's matches.
//   k_tv_lo       (movba_two_view_lo with lo_iters > 0 only) one workgroup per pair: the winner as k_tv_recover finds it
//                 (tv_select), then lo_iters + 1 passes over the pair's matches - threads stride the matches with the 21
//                 accumulators in registers, a butterfly per wave, the four waves combined in LDS in wave order - between
//                 which thread 0 factors the 5 x 5 system, steps and rebuilds E and its derivatives in LDS.  The kept E and
//                 the call's `info` go to the pair's slot of TvDev::lo.  The matches are read from global memory in every
//                 pass: a pair of MOVBA_MAX_TWO_VIEW_MATCHES matches is 1 MiB of coordinates, several times the LDS.
//   k_tv_recover  one workgroup per pair: best candidate per sample (one thread per sample), the stopping rule's walk
//                 (tv_select) - or the kept E of a marked slot -, the threshold mask, the decomposition of E, the four
//                 cheirality counts (one wave each), the final mask.
//   k_tv_check    one workgroup per pair: CheckRT for every match (thread-strided), then the order statistic of the accepted
//                 cosines by counting ranks, the outcome and the pose.
// No atomics on floating-point data: sums are per-lane partial sums combined by a butterfly in a fixed order; counts are integers.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "two_view.h"
#include "two_view_math.h"

namespace movba {

namespace {

struct TvSyncWg { __device__ void operator()() const { __syncthreads(); } };

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kTvThreads) void k_tv_hyp(const TvDev d)
{
    __shared__ TvWork w;
    __shared__ double q[20], E[9 * kTvMaxSol];
    __shared__ int nsol_s;
    const int tid = threadIdx.x;
    const int pi = prefix_find(d.hyp_first, d.n_pairs, blockIdx.x);
    const TvPair p = d.pairs[pi];
    const int h = blockIdx.x - d.hyp_first[pi];
    const size_t hg = (size_t)p.h0 + h;
    const double *o1 = d.obs1 + 2 * (size_t)p.m0, *o2 = d.obs2 + 2 * (size_t)p.m0;
    const double inv_f = 1.0 / p.f;
    if (tid < 5) {
        const int i = min(max(d.samples[5 * hg + tid], 0), p.n - 1);
        q[4 * tid] = (o1[2 * i] - p.cx) * inv_f; q[4 * tid + 1] = (o1[2 * i + 1] - p.cy) * inv_f;
        q[4 * tid + 2] = (o2[2 * i] - p.cx) * inv_f; q[4 * tid + 3] = (o2[2 * i + 1] - p.cy) * inv_f;
    }
    if (tid < 9 * kTvMaxSol) E[tid] = 0.0;
    __syncthreads();
    tv_five_point(w, q, E, &nsol_s, tid, kTvThreads, TvSyncWg{});
    const int ns = nsol_s;
    if (tid < 9 * kTvMaxSol) d.cand[90 * hg + tid] = tid < 9 * ns ? E[tid] : 0.0;
    if (tid == 0) d.nsol[hg] = ns;
    if (tid >= ns && tid < kTvMaxSol) { d.loss[10 * hg + tid] = __builtin_inf(); d.cnt[10 * hg + tid] = -1; }
    // score: wave wv takes candidates wv, wv + 4, wv + 8
    const int lane = tid & 63, wv = tid >> 6;
    const Magsac ms(p.thr2);
    const double f2 = p.f * p.f;
    for (int c = wv; c < ns; c += kTvThreads / 64) {
        double Ec[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Ec[e] = E[9 * c + e];
        double ls = 0.0;
        int cn = 0;
        for (int i = lane; i < p.n; i += 64) {
            const double2 a = reinterpret_cast<const double2 *>(o1)[i], b = reinterpret_cast<const double2 *>(o2)[i];
            const double s2 = f2 * tv_sampson2(Ec, (a.x - p.cx) * inv_f, (a.y - p.cy) * inv_f, (b.x - p.cx) * inv_f, (b.y - p.cy) * inv_f);
            double l1, wt;
            ms.terms(s2, true, p.thr2, l1, wt);
            ls += l1;
            cn += s2 <= p.thr2 ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ls += __shfl_xor(ls, o, 64);
        cn = wave_sum(cn);
        if (lane == 0) { d.loss[10 * hg + c] = ls; d.cnt[10 * hg + c] = cn; }
    }
}

// Best candidate per sample (one thread per sample), then the stopping rule's walk by thread 0: *best_s = the winner's candidate
// index 10 h + c (< 0: none), *used_s = the samples admitted.  sl / sc / sb: LDS, MOVBA_MAX_TWO_VIEW_ITERS each.  Ends behind a barrier.
__device__ __forceinline__ void tv_select(const TvDev &d, const TvPair &p, double *sl, int *sc, int *sb, int *best_s, int *used_s, int tid)
{
    for (int h = tid; h < p.n_hyp; h += kTvThreads) {
        const size_t hg = (size_t)p.h0 + h;
        const int ns = d.nsol[hg];
        double bl = 0.0;
        int bi = -1, bc = 0;
        for (int c = 0; c < ns; ++c) {
            const double l = d.loss[10 * hg + c];
            if (bi < 0 || l < bl) { bi = 10 * h + c; bl = l; bc = d.cnt[10 * hg + c]; }
        }
        sl[h] = bl; sc[h] = bc; sb[h] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        int b, u;
        tv_walk(sl, sc, sb, p.n_hyp, p.n, p.conf, &b, &u);
        *best_s = b; *used_s = u;
    }
    __syncthreads();
}

// One pass of the refit over the pair's matches at E (and, for a pass that takes a step, its five derivatives dE), both in LDS:
// thread-strided with the kTvLoAcc accumulators in registers, a butterfly per wave, then thread a adds the four waves' sums of
// accumulator a in wave order.  acc (LDS) holds the sums behind the closing barrier; cnt4 (nullptr: not counted) the waves'
// numbers of matches within the threshold by k_tv_recover's own test.
__device__ __forceinline__ void tv_lo_pass(const TvPair &p, const double *o1, const double *o2, const double *E, const double (*dE)[9], bool want,
                                           const Magsac &ms, double (*red)[kTvLoAcc], double *acc, int *cnt4, int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    const double inv_f = 1.0 / p.f, f2 = p.f * p.f;
    double Ec[9], dEc[5][9], a[kTvLoAcc];
#pragma unroll
    for (int e = 0; e < 9; ++e) Ec[e] = E[e];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int e = 0; e < 9; ++e) dEc[j][e] = want ? dE[j][e] : 0.0;
#pragma unroll
    for (int e = 0; e < kTvLoAcc; ++e) a[e] = 0.0;
    int cn = 0;
    for (int i = tid; i < p.n; i += kTvThreads) {
        const double2 u = reinterpret_cast<const double2 *>(o1)[i], v = reinterpret_cast<const double2 *>(o2)[i];
        const double x1 = (u.x - p.cx) * inv_f, y1 = (u.y - p.cy) * inv_f, x2 = (v.x - p.cx) * inv_f, y2 = (v.y - p.cy) * inv_f;
        tv_lo_accumulate(ms, p.thr2, Ec, dEc, want, p.f, x1, y1, x2, y2, a);
        if (cnt4) cn += f2 * tv_sampson2(Ec, x1, y1, x2, y2) <= p.thr2 ? 1 : 0;
    }
#pragma unroll
    for (int e = 0; e < kTvLoAcc; ++e) {
        double v = a[e];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wv][e] = v;
    }
    if (cnt4) {
        cn = wave_sum(cn);
        if (lane == 0) cnt4[wv] = cn;
    }
    __syncthreads();
    if (tid < kTvLoAcc) acc[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
}

__global__ __launch_bounds__(kTvThreads) void k_tv_lo(const TvDev d)
{
    __shared__ double sl[MOVBA_MAX_TWO_VIEW_ITERS];
    __shared__ int sc[MOVBA_MAX_TWO_VIEW_ITERS], sb[MOVBA_MAX_TWO_VIEW_ITERS];
    __shared__ int best_s, used_s, go_s, cnt4[kTvThreads / 64];
    __shared__ TvLoState st;
    __shared__ TvLoTrack trk;           // (thread 0's)
    __shared__ double red[kTvThreads / 64][kTvLoAcc], acc[kTvLoAcc];
    const int tid = threadIdx.x;
    const TvPair p = d.pairs[blockIdx.x];
    if (p.n_hyp <= 0) return;
    tv_select(d, p, sl, sc, sb, &best_s, &used_s, tid);
    const int best = best_s;
    if (best < 0) return;               // (the slot stays zero: k_tv_recover finds no winner either)
    const double *o1 = d.obs1 + 2 * (size_t)p.m0, *o2 = d.obs2 + 2 * (size_t)p.m0;
    const Magsac ms(p.thr2);
    if (tid == 0) tv_lo_begin(d.cand + 90 * (size_t)p.h0 + 9 * (size_t)best, st, trk);
    __syncthreads();
    for (int k = 0; k <= d.lo_iters; ++k) {
        tv_lo_pass(p, o1, o2, st.E, st.dE, k < d.lo_iters, ms, red, acc, k == 0 ? cnt4 : nullptr, tid);
        if (tid == 0) go_s = tv_lo_advance(st, trk, acc, k, d.lo_iters) ? 1 : 0;
        __syncthreads();
        if (!go_s) break;
    }
    if (tid == 0) {
        double *slot = d.lo + (size_t)kTvLoDoubles * blockIdx.x;
        tv_lo_result(trk, slot);
#pragma unroll
        for (int e = 0; e < 9; ++e) slot[9 + e] = trk.E0[e];
        slot[18] = trk.loss0; slot[19] = trk.loss; slot[20] = (double)trk.kept; slot[21] = (double)trk.steps;
        slot[22] = (double)(((cnt4[0] + cnt4[1]) + cnt4[2]) + cnt4[3]);
        slot[23] = 1.0;
    }
}

__global__ __launch_bounds__(kTvThreads) void k_tv_recover(const TvDev d)
{
    __shared__ double sl[MOVBA_MAX_TWO_VIEW_ITERS];
    __shared__ int sc[MOVBA_MAX_TWO_VIEW_ITERS], sb[MOVBA_MAX_TWO_VIEW_ITERS];
    __shared__ int best_s, used_s, n_in, cheir[4];
    __shared__ double Rt[2][9], tt[3], Ew[9];
    __shared__ double red[kTvThreads / 64][kTvLoAcc], acc[kTvLoAcc];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const TvPair p = d.pairs[blockIdx.x];
    double *rec = d.rec + (size_t)kTvRecDoubles * blockIdx.x;
    const double *o1 = d.obs1 + 2 * (size_t)p.m0, *o2 = d.obs2 + 2 * (size_t)p.m0;
    uint8_t *inl0 = d.inl0 + p.m0;
    if (tid == 0) { n_in = 0; cheir[0] = cheir[1] = cheir[2] = cheir[3] = 0; }
    tv_select(d, p, sl, sc, sb, &best_s, &used_s, tid);
    const int best = best_s;
    if (best < 0) {
        for (int i = tid; i < p.n; i += kTvThreads) { inl0[i] = 0; p.inlier[i] = 0; }
        if (tid < kTvRecDoubles) rec[tid] = tid == 23 ? (double)used_s : 0.0;
        return;
    }
    // the refit's kept E where k_tv_lo has marked the pair's slot, else the winner itself
    double *slot = d.lo ? d.lo + (size_t)kTvLoDoubles * blockIdx.x : nullptr;
    const bool refit = slot && slot[23] != 0.0;
    if (tid < 9) Ew[tid] = refit ? slot[tid] : d.cand[90 * (size_t)p.h0 + 9 * (size_t)best + tid];
    __syncthreads();
    // `info` without a refit: the winner's loss by the refit's own pass
    if (slot && !refit) tv_lo_pass(p, o1, o2, Ew, nullptr, false, Magsac(p.thr2), red, acc, nullptr, tid);
    const double inv_f = 1.0 / p.f, f2 = p.f * p.f;
    double Ec[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Ec[e] = Ew[e];
    int mine = 0;
    for (int i = tid; i < p.n; i += kTvThreads) {
        const double s2 = f2 * tv_sampson2(Ec, (o1[2 * i] - p.cx) * inv_f, (o1[2 * i + 1] - p.cy) * inv_f, (o2[2 * i] - p.cx) * inv_f,
                                           (o2[2 * i + 1] - p.cy) * inv_f);
        const bool in = s2 <= p.thr2;
        inl0[i] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    mine = wave_sum(mine);
    if (lane == 0) atomicAdd(&n_in, mine);
    if (tid == 0) tv_decompose(Ec, Rt[0], Rt[1], tt);
    __syncthreads();
    // wave wv counts combination wv: (R1, t), (R2, t), (R1, -t), (R2, -t)
    {
        double R[9], t[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = Rt[wv & 1][e];
#pragma unroll
        for (int e = 0; e < 3; ++e) t[e] = (wv & 2) ? -tt[e] : tt[e];
        int cn = 0;
        for (int i = lane; i < p.n; i += 64) {
            if (!inl0[i]) continue;
            cn += tv_cheirality(R, t, (o1[2 * i] - p.cx) * inv_f, (o1[2 * i + 1] - p.cy) * inv_f, (o2[2 * i] - p.cx) * inv_f,
                                (o2[2 * i + 1] - p.cy) * inv_f, p.max_depth) ? 1 : 0;
        }
        cn = wave_sum(cn);
        if (lane == 0) cheir[wv] = cn;
    }
    __syncthreads();
    int pick = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c) pick = cheir[c] > cheir[pick] ? c : pick;
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rt[pick & 1][e];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = (pick & 2) ? -tt[e] : tt[e];
    for (int i = tid; i < p.n; i += kTvThreads) {
        const bool ok = inl0[i] && tv_cheirality(R, t, (o1[2 * i] - p.cx) * inv_f, (o1[2 * i + 1] - p.cy) * inv_f, (o2[2 * i] - p.cx) * inv_f,
                                                 (o2[2 * i + 1] - p.cy) * inv_f, p.max_depth);
        p.inlier[i] = ok ? 1 : 0;
        inl0[i] = ok ? 1 : 0;           // (k_tv_check reads the final mask from device memory)
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) { rec[e] = Ec[e]; rec[9 + e] = R[e]; }
        rec[18] = t[0]; rec[19] = t[1]; rec[20] = t[2];
        rec[21] = (double)n_in; rec[22] = (double)cheir[pick]; rec[23] = (double)used_s; rec[24] = (double)best;
        rec[25] = n_in > 0 ? 1.0 : 0.0;
        for (int e = 26; e < kTvRecDoubles; ++e) rec[e] = 0.0;
        if (slot && !refit) {
#pragma unroll
            for (int e = 0; e < 9; ++e) slot[9 + e] = Ec[e];
            slot[18] = acc[20]; slot[19] = acc[20]; slot[22] = (double)n_in;
        }
        if (slot && n_in == 0)          // (MOVBA_TV_NO_MODEL: a zeroed `info`)
            for (int e = 0; e < kTvLoDoubles - 1; ++e) slot[e] = 0.0;
    }
}

__global__ __launch_bounds__(kTvThreads) void k_tv_check(const TvDev d)
{
    __shared__ int n_good_s;
    __shared__ double sel;
    const int tid = threadIdx.x, lane = tid & 63;
    const TvPair p = d.pairs[blockIdx.x];
    const double *rec = d.rec + (size_t)kTvRecDoubles * blockIdx.x;
    const double *o1 = d.obs1 + 2 * (size_t)p.m0, *o2 = d.obs2 + 2 * (size_t)p.m0;
    double *cosv = d.cosv + p.m0;
    const double nan = __builtin_nan("");
    const bool model = p.n_hyp > 0 && rec[25] != 0.0;
    if (!model) {
        for (int i = tid; i < p.n; i += kTvThreads) {
            p.points[3 * (size_t)i] = nan; p.points[3 * (size_t)i + 1] = nan; p.points[3 * (size_t)i + 2] = nan;
            p.good[i] = 0; p.code[i] = MOVBA_TV_CHK_NONE;
            if (p.n_hyp > 0 && rec[25] == 0.0) p.inlier[i] = 0;
        }
        if (tid < kTvOutDoubles) {
            double v = 0.0;
            if (tid == 3) v = 1.0;
            if (tid == 17) v = (double)MOVBA_TV_NO_MODEL;
            if (tid == 21 && p.n_hyp > 0) v = rec[23];
            if (tid == 22) v = -1.0;
            p.out[tid] = v;
        }
        return;
    }
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = rec[9 + e];
    t[0] = rec[18]; t[1] = rec[19]; t[2] = rec[20];
    if (tid == 0) n_good_s = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < p.n; i += kTvThreads) {
        double X[3] = { nan, nan, nan }, cp = __builtin_inf();
        uint8_t code = MOVBA_TV_CHK_REJ_NOT_INLIER;
        if (d.inl0[p.m0 + i]) code = tv_check(R, t, p.fx, p.fy, p.cx, p.cy, o1[2 * i], o1[2 * i + 1], o2[2 * i], o2[2 * i + 1], p.th2, X, &cp);
        const bool acc = code == MOVBA_TV_CHK_GOOD || code == MOVBA_TV_CHK_LOW_PARALLAX;
        cosv[i] = acc ? cp : __builtin_inf();
        p.points[3 * (size_t)i] = X[0]; p.points[3 * (size_t)i + 1] = X[1]; p.points[3 * (size_t)i + 2] = X[2];
        p.good[i] = code == MOVBA_TV_CHK_GOOD ? 1 : 0;
        p.code[i] = code;
        mine += acc ? 1 : 0;
    }
    mine = wave_sum(mine);
    if (lane == 0) atomicAdd(&n_good_s, mine);
    if (tid == 0) sel = nan;
    __syncthreads();
    const int n_good = n_good_s;
    // element min(50, nGood - 1) of the sorted accepted cosines (:236-239): the value whose rank is that index
    if (n_good > 0) {
        const int idx = min(50, n_good - 1);
        for (int i = tid; i < p.n; i += kTvThreads) {
            const double ci = cosv[i];
            if (!(ci < __builtin_inf())) continue;
            int rank = 0;
            for (int j = 0; j < p.n; ++j) {
                const double cj = cosv[j];
                rank += (cj < ci || (cj == ci && j < i)) ? 1 : 0;
            }
            if (rank == idx) sel = ci;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const double parallax = n_good > 0 ? acos(sel) * 180.0 / 3.14159265358979323846 : 0.0;
        const int n_in = (int)rec[21], n_pass = (int)rec[22];
        const int min_good = max((int)(0.75 * (double)n_in), p.min_tri);
        const int outcome = n_pass < min_good ? MOVBA_TV_FEW_GOOD : (parallax > p.min_par ? MOVBA_TV_OK : MOVBA_TV_LOW_PARALLAX);
        double qv[4];
        tv_R2q(R, qv);
        double *o = p.out;
        o[0] = qv[0]; o[1] = qv[1]; o[2] = qv[2]; o[3] = qv[3]; o[4] = t[0]; o[5] = t[1]; o[6] = t[2];
#pragma unroll
        for (int e = 0; e < 9; ++e) o[7 + e] = rec[e];
        o[16] = parallax; o[17] = (double)outcome; o[18] = (double)n_in; o[19] = (double)n_pass; o[20] = (double)n_good;
        o[21] = rec[23]; o[22] = rec[24];
        for (int e = 23; e < kTvOutDoubles; ++e) o[e] = 0.0;
    }
}

}  // namespace

hipError_t launch_two_view(const TvDev &d, hipStream_t s)
{
    if (d.n_pairs <= 0) return hipGetLastError();
    if (d.n_hyp_total > 0) hipLaunchKernelGGL(k_tv_hyp, dim3(d.n_hyp_total), dim3(kTvThreads), 0, s, d);
    if (d.n_hyp_total > 0 && d.lo && d.lo_iters > 0) hipLaunchKernelGGL(k_tv_lo, dim3(d.n_pairs), dim3(kTvThreads), 0, s, d);
    hipLaunchKernelGGL(k_tv_recover, dim3(d.n_pairs), dim3(kTvThreads), 0, s, d);
    hipLaunchKernelGGL(k_tv_check, dim3(d.n_pairs), dim3(kTvThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
