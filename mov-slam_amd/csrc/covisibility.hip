// The kernel of movba_covisibility (include/movba.h).
//
// k_covis: one workgroup of 256 threads per query, one launch over all queries of the call.  Everything a query needs lives in
// its workgroup's LDS, sized to the call's n_views (covisibility.h: cv_lds_bytes; 98 KB at MOVBA_MAX_COVIS_VIEWS, 6.2 KB at a
// 500-keyframe map): one int32 counter per view and the 64-bit sort keys of the counted views.
//   1. the counters are zeroed
//   2. count: each wave takes 64 items of the query at a time, one per lane.  A lane walks its item's list and adds to the
//      counters with LDS atomics (integer sums commute: the result does not depend on the order).  Items whose list has
//      kCvWaveList observers or more are left out of that walk and then taken one after the other by the whole wave, 64 entries a
//      step: a hub point seen by thousands of views does not serialise its wave - what point_normals.hip documents for its
//      one-lane walk, which has a sequential sum to keep; this count has none.
//   3. compact: thread t owns the views [t * per, (t + 1) * per), ascending; a scan over the threads' numbers of counted views
//      gives each its place, so the keys stand in ascending view order.  The query's own view and the views that are not eligible
//      drop out here (cv_weight).  The same pass finds n_counted, the views at or above min_weight and the best view.
//   4. sort: bitonic over pow2ceil(n_counted) keys, descending, the tail padded with 0.  The keys are distinct, so the method
//      does not show in the result.
//   5. thread 0 writes the four scalars, all threads the query's row of out_view / out_weight with its -1 / 0 padding.
// A workgroup reads its own query's items and the lists they name, and writes its own query's results: it waits for no other
// workgroup, and no result depends on which others ran.  Global memory is written with ordinary vector stores only.
#include <hip/hip_runtime.h>

#include "covisibility.h"

namespace movba {

namespace {

constexpr int kWaves = kCvThreads / 64;

// the head of the LDS (kCvLdsHead bytes): per-wave partial results of the compaction pass
struct CvHead {
    uint64_t best[kWaves];
    int32_t counted[kWaves], reaching[kWaves];
};
static_assert(sizeof(CvHead) <= kCvLdsHead, "the scratch of the scans outgrew the head of the LDS");

__device__ inline int32_t wave_sum(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline uint64_t wave_best(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = cv_best_max(v, (uint64_t)__shfl_xor((unsigned long long)v, o));
    return v;
}

__global__ __launch_bounds__(kCvThreads) void k_covis(const CvDev d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    CvHead *head = reinterpret_cast<CvHead *>(lds);
    const int32_t nv = d.n_views;
    uint64_t *keys = reinterpret_cast<uint64_t *>(lds + kCvLdsHead);
    int32_t *counters = reinterpret_cast<int32_t *>(lds + kCvLdsHead + 8 * (size_t)cv_pow2ceil(nv));

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t q = blockIdx.x;
    const int32_t qs = d.query_ptr[q], qe = d.query_ptr[q + 1];
    const int32_t self = d.query_self ? d.query_self[q] : -1;

    // 1.
    for (int32_t v = tid; v < nv; v += kCvThreads) counters[v] = 0;
    __syncthreads();

    // 2.  (base and qe are the same for every lane of a wave: the ballot and the shuffles below run with the whole wave)
    for (int32_t base = qs + wave * 64; base < qe; base += kCvThreads) {
        const int32_t i = base + lane;
        int32_t k0 = 0, k1 = 0;
        if (i < qe) {
            const int32_t p = d.query_point[i];
            k0 = d.obs_ptr[p]; k1 = d.obs_ptr[p + 1];
        }
        const bool hub = k1 - k0 >= kCvWaveList;
        if (!hub) cv_count_list(counters, d.obs_view, k0, k1, 0, 1);
        unsigned long long hubs = __ballot(hub);
        while (hubs) {
            const int src = __ffsll(hubs) - 1;
            hubs &= hubs - 1;
            cv_count_list(counters, d.obs_view, __shfl(k0, src), __shfl(k1, src), lane, 64);
        }
    }
    __syncthreads();

    // 3.
    const int32_t per = (nv + kCvThreads - 1) / kCvThreads;
    const int32_t v0 = min(tid * per, nv), v1 = min(v0 + per, nv);
    int32_t mine = 0, reaching = 0;
    uint64_t best = 0;
    for (int32_t v = v0; v < v1; ++v) {
        const int32_t w = cv_weight(counters, v, d.eligible, self);
        if (w <= 0) continue;
        ++mine;
        reaching += w >= d.min_weight;
        best = cv_best_max(best, cv_best_key(w, v));
    }
    // (inclusive scan of `mine` over the lanes of the wave, then over the waves)
    int32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    reaching = wave_sum(reaching);
    best = wave_best(best);
    if (lane == 63) head->counted[wave] = incl;
    if (lane == 0) { head->reaching[wave] = reaching; head->best[wave] = best; }
    __syncthreads();
    int32_t place = incl - mine, n_counted = 0, n_reaching = 0;
    uint64_t q_best = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) place += head->counted[w];
        n_counted += head->counted[w];
        n_reaching += head->reaching[w];
        q_best = cv_best_max(q_best, head->best[w]);
    }
    for (int32_t v = v0; v < v1; ++v) {
        const int32_t w = cv_weight(counters, v, d.eligible, self);
        if (w > 0) keys[place++] = cv_key(w, v);
    }
    const int32_t m = cv_pow2ceil(n_counted);
    for (int32_t k = n_counted + tid; k < m; k += kCvThreads) keys[k] = 0;
    __syncthreads();

    // 4.  (m <= pow2ceil(n_views): the keys' part of the LDS holds it)
    for (int32_t k = 2; k <= m; k <<= 1) {
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t t = tid; t < (m >> 1); t += kCvThreads) cv_sort_pair(keys, t, j, k);
            __syncthreads();
        }
    }

    // 5.
    if (tid == 0) {
        d.n_counted[q] = n_counted;
        d.n_connected[q] = cv_connected(n_counted, n_reaching);
        d.best_view[q] = cv_best_view(q_best);
        d.best_weight[q] = cv_best_weight(q_best);
    }
    const size_t row = (size_t)q * (size_t)d.max_out;
    for (int32_t k = tid; k < d.max_out; k += kCvThreads) {
        int32_t view, weight;
        cv_hand_out(keys, n_counted, k, &view, &weight);
        d.out_view[row + k] = view;
        d.out_weight[row + k] = weight;
    }
}

}  // namespace

hipError_t launch_covisibility(const CvDev &d, hipStream_t s)
{
    if (d.n_queries <= 0) return hipGetLastError();
    const size_t lds = cv_lds_bytes(d.n_views);
    // (above the 64 KB a kernel may ask for unannounced; per device, so said where it is needed rather than once per process)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_covis), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv_lds_bytes(MOVBA_MAX_COVIS_VIEWS));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_covis, dim3(d.n_queries), dim3(kCvThreads), lds, s, d);
    return hipGetLastError();
}

}  // namespace movba
