// Device view + launch wrapper of movba_covisibility (covisibility.hip; host side: covisibility.cpp), and the steps of one query
// that have a serial meaning - count, order, best, connected - as plain C++ (what k_covis calls from its lanes, and what a host
// build runs query by query: cv_query): the numeric body of KeyFrame::UpdateConnections (KeyFrame.cc:367-459) and of the voting
// loop of Tracking::UpdateLocalKeyFrames (Tracking.cc:1200-1280), as include/movba.h restates it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "movba.h"

namespace movba {

// Everything the kernel reads and writes.  Inputs lie in device memory, every index in them checked by the host; every out
// pointer is device memory or a device view of pinned host memory (the staging buffer, or the caller's movba_host_alloc arrays).
struct CvDev {
    int32_t n_views, n_queries, min_weight, max_out;
    const int32_t *obs_ptr, *obs_view;              // the observers of point p: obs_view[obs_ptr[p] .. obs_ptr[p + 1])
    const uint8_t *eligible;                        // n_views, or nullptr: all
    const int32_t *query_ptr, *query_point;         // the items of query q: query_point[query_ptr[q] .. query_ptr[q + 1])
    const int32_t *query_self;                      // n_queries, or nullptr: all -1
    int32_t *n_counted, *n_connected, *best_view, *best_weight;     // out: n_queries each
    int32_t *out_view, *out_weight;                 // out: n_queries x max_out (nullptr when max_out == 0)
};

constexpr int kCvThreads = 256;
// a list of this many observers or more is walked by a whole wave, a shorter one by the lane that owns its item
constexpr int kCvWaveList = 64;
// front of the workgroup's LDS: the scratch of its scans and reductions; the sort keys and the counters lie behind it
constexpr size_t kCvLdsHead = 128;

// the sort runs over a power of two of keys, the tail padded with 0 (a key no counted view has: its weight is 0)
__host__ __device__ inline int32_t cv_pow2ceil(int32_t n)
{
    int32_t m = 1;
    while (m < n) m <<= 1;
    return m;
}

// LDS of one workgroup: head | pow2ceil(n_views) 64-bit keys | n_views 32-bit counters.  98 432 bytes at MOVBA_MAX_COVIS_VIEWS.
inline size_t cv_lds_bytes(int32_t n_views) { return kCvLdsHead + 8 * (size_t)cv_pow2ceil(n_views) + 4 * (size_t)n_views; }

// k_covis over all queries, on the stream
hipError_t launch_covisibility(const CvDev &d, hipStream_t s);

// ---- the steps ----

// count: one occurrence of a view in a list of the query (KFcounter[mit->first]++, KeyFrame.cc:396; keyframeCounter[..]++,
// Tracking.cc:1217).  On the device the counter is in LDS and other lanes add to it at the same time.
__host__ __device__ inline void cv_bump(int32_t *counter)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(counter, 1);
#else
    ++*counter;
#endif
}

// count: entries first, first + stride, ... of one item's list [k0, k1).  Every view that is named is counted here; the ones the
// query must not count (KeyFrame.cc:394) are taken out by cv_weight, which gives the same weights as skipping them here and
// reads `eligible` once per view instead of once per observation.
__host__ __device__ inline void cv_count_list(int32_t *counters, const int32_t *obs_view, int32_t k0, int32_t k1, int32_t first, int32_t stride)
{
    for (int32_t k = k0 + first; k < k1; k += stride) cv_bump(counters + obs_view[k]);
}

// count: weight[q][v] from the raw counter: 0 for the query's own view and for a view that is not eligible
__host__ __device__ inline int32_t cv_weight(const int32_t *counters, int32_t v, const uint8_t *eligible, int32_t self)
{
    if (v == self || (eligible && !eligible[v])) return 0;
    return counters[v];
}

// order: by weight descending, ties by view index descending = by this key descending (sort(vPairs) ascending by (weight,
// pointer), then push_front: KeyFrame.cc:436-443).  Keys of one query are distinct, and none is 0.
__host__ __device__ inline uint64_t cv_key(int32_t weight, int32_t view) { return ((uint64_t)(uint32_t)weight << 32) | (uint32_t)view; }
__host__ __device__ inline int32_t cv_key_weight(uint64_t key) { return (int32_t)(key >> 32); }
__host__ __device__ inline int32_t cv_key_view(uint64_t key) { return (int32_t)(uint32_t)key; }

// best: `>` while walking the views in ascending order keeps the first maximum (KeyFrame.cc:418, Tracking.cc:1272) = the
// largest of these keys, which rank a lower view above a higher one of the same weight.  0: no view.
__host__ __device__ inline uint64_t cv_best_key(int32_t weight, int32_t view) { return ((uint64_t)(uint32_t)weight << 32) | (uint32_t)(0x7fffffff - view); }
__host__ __device__ inline uint64_t cv_best_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
__host__ __device__ inline int32_t cv_best_view(uint64_t best) { return best ? 0x7fffffff - (int32_t)(uint32_t)best : -1; }
__host__ __device__ inline int32_t cv_best_weight(uint64_t best) { return (int32_t)(best >> 32); }

// connected: the views at or above the threshold; none of them but something counted: the one best view (KeyFrame.cc:423-434)
__host__ __device__ inline int32_t cv_connected(int32_t n_counted, int32_t n_reaching)
{
    if (n_counted == 0) return 0;
    return n_reaching > 0 ? n_reaching : 1;
}

// hand-out: entry k of a query's row from its sorted keys
__host__ __device__ inline void cv_hand_out(const uint64_t *keys, int32_t n_counted, int32_t k, int32_t *view, int32_t *weight)
{
    *view = k < n_counted ? cv_key_view(keys[k]) : -1;
    *weight = k < n_counted ? cv_key_weight(keys[k]) : 0;
}

// order: one compare-exchange of the bitonic network over m keys, m a power of two: pair t of the m / 2 pairs at distance j of the
// stage that merges runs of k keys.  The pairs of one (k, j) touch disjoint keys; the result is descending.
__host__ __device__ inline void cv_sort_pair(uint64_t *keys, int32_t t, int32_t j, int32_t k)
{
    const int32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
    const uint64_t a = keys[lo], b = keys[hi];
    const bool descending = (lo & k) == 0;
    if ((a < b) == descending) { keys[lo] = b; keys[hi] = a; }
}

// order: the whole network on one thread over keys[0, n), padded to m = pow2ceil(n) with 0 as the kernel pads it
inline void cv_sort_serial(uint64_t *keys, int32_t n)
{
    const int32_t m = cv_pow2ceil(n);
    for (int32_t k = n; k < m; ++k) keys[k] = 0;
    for (int32_t k = 2; k <= m; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1)
            for (int32_t t = 0; t < (m >> 1); ++t) cv_sort_pair(keys, t, j, k);
}

// One query from front to back on one thread, the steps in the kernel's order.  Scratch: counters, n_views entries, and keys,
// pow2ceil(n_views) entries.
inline void cv_query(const CvDev &d, int32_t q, int32_t *counters, uint64_t *keys)
{
    const int32_t self = d.query_self ? d.query_self[q] : -1;
    for (int32_t v = 0; v < d.n_views; ++v) counters[v] = 0;
    for (int32_t i = d.query_ptr[q]; i < d.query_ptr[q + 1]; ++i) {
        const int32_t p = d.query_point[i];
        cv_count_list(counters, d.obs_view, d.obs_ptr[p], d.obs_ptr[p + 1], 0, 1);
    }
    int32_t n_counted = 0, n_reaching = 0;
    uint64_t best = 0;
    for (int32_t v = 0; v < d.n_views; ++v) {
        const int32_t w = cv_weight(counters, v, d.eligible, self);
        if (w <= 0) continue;
        keys[n_counted++] = cv_key(w, v);
        n_reaching += w >= d.min_weight;
        best = cv_best_max(best, cv_best_key(w, v));
    }
    cv_sort_serial(keys, n_counted);
    d.n_counted[q] = n_counted;
    d.n_connected[q] = cv_connected(n_counted, n_reaching);
    d.best_view[q] = cv_best_view(best);
    d.best_weight[q] = cv_best_weight(best);
    for (int32_t k = 0; k < d.max_out; ++k)
        cv_hand_out(keys, n_counted, k, d.out_view + (size_t)q * d.max_out + k, d.out_weight + (size_t)q * d.max_out + k);
}

}  // namespace movba
