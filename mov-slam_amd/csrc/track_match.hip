// The kernels of movba_track_match (include/movba.h).
//
// k_tm_match: one workgroup of 256 threads per query, one launch over all queries of the call.  The workgroup builds an
// open-addressing table in its LDS over the slots of the view that is searched (view 2; TRIANGULATION: the slots that are not
// taken, LOOKUP: all of them) and probes it with the free slots of view 1, or with the query's items.  The table holds slot
// indices, 2 x pow2ceil(slots) of them (track_match.h: tm_lds_bytes; 128 KB at MOVBA_MAX_TRACK_SLOTS, 16 KB at a keyframe of
// 2 000 features), so it is at most half full and no id value is reserved for "empty".
//   1. the table is emptied
//   2. insert: one slot per thread and step (tm_insert: compare-and-swap on an empty entry, atomic minimum on an entry whose
//      occupant carries the same id - the lowest slot wins whatever order the lanes arrive in)
//   3. LOOKUP: one item per thread and step, the hit or -1 to item_slot, the hits summed over the workgroup to n_found
//      TRIANGULATION: view 1's slots in chunks of 256, ascending; a scan over the workgroup's hit flags gives each hit of a chunk
//      its place behind the hits of the chunks before it, so the query's matches stand in ascending i in its scratch row
//   4. thread 0 writes the query's count
// k_tm_pack: one workgroup per query again.  It sums the counts in front of its query (the query's place in pair_ptr) and all
// of them, moves its row to its dense place with the payload of the matched slots (tm_place), and takes a share of the tail
// behind the last match (tm_pad).
// A workgroup reads its own query's views and items and writes its own query's results: no result depends on which others
// ran.  Global memory is written with ordinary vector stores only; floating point does not occur.
#include <hip/hip_runtime.h>

#include "track_match.h"

namespace movba {

namespace {

constexpr int kWaves = kTmThreads / 64;

// the head of the LDS (kTmLdsHead bytes): per-wave partial results of the scans
struct TmHead {
    int32_t hits[kWaves];
};
static_assert(sizeof(TmHead) <= kTmLdsHead, "the scratch of the scans outgrew the head of the LDS");

__device__ inline int32_t wave_sum(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kTmThreads) void k_tm_match(const TmDev d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    TmHead *head = reinterpret_cast<TmHead *>(lds);
    int32_t *table = reinterpret_cast<int32_t *>(lds + kTmLdsHead);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t q = blockIdx.x;
    const bool lookup = d.query_mode[q] == MOVBA_TM_LOOKUP;
    const int32_t v1 = d.query_view[2 * q], v2 = d.query_view[2 * q + 1];
    const int32_t b2 = d.view_ptr[v2], n2 = d.view_ptr[v2 + 1] - b2;
    const int32_t *track2 = d.slot_track + b2;
    const uint8_t *taken2 = d.slot_taken ? d.slot_taken + b2 : nullptr;
    const int32_t entries = tm_table_entries(n2);

    // 1.
    for (int32_t e = tid; e < entries; e += kTmThreads) table[e] = kTmEmpty;
    __syncthreads();

    // 2.
    for (int32_t j = tid; j < n2; j += kTmThreads)
        if (lookup || tm_free(taken2, j)) tm_insert(table, entries, track2, j);
    __syncthreads();

    // 3.
    if (lookup) {
        const int32_t qs = d.query_ptr[q], qe = d.query_ptr[q + 1];
        int32_t found = 0;
        for (int32_t i = qs + tid; i < qe; i += kTmThreads) {
            const int32_t j = tm_find(table, entries, track2, d.item_track[i]);
            d.item_slot[i] = j;
            found += j >= 0;
        }
        found = wave_sum(found);
        if (lane == 0) head->hits[wave] = found;
        __syncthreads();
        if (tid == 0) {
            int32_t all = 0;
            for (int w = 0; w < kWaves; ++w) all += head->hits[w];
            d.n_found[q] = all;
            d.count[q] = 0;
        }
        return;
    }

    // (the chunk's bounds are the same for every thread: the ballot and the barriers below run with the whole workgroup)
    const int32_t b1 = d.view_ptr[v1], n1 = d.view_ptr[v1 + 1] - b1;
    const uint8_t *taken1 = d.slot_taken ? d.slot_taken + b1 : nullptr;
    const int32_t row = d.row_base[q];
    int32_t base = 0;
    for (int32_t chunk = 0; chunk < n1; chunk += kTmThreads) {
        const int32_t i = chunk + tid;
        int32_t j = -1;
        if (i < n1 && tm_free(taken1, i)) j = tm_find(table, entries, track2, d.slot_track[b1 + i]);
        const unsigned long long hits = __ballot(j >= 0);
        if (lane == 0) head->hits[wave] = __popcll(hits);
        __syncthreads();
        int32_t place = base + __popcll(hits & ((1ull << lane) - 1ull)), all = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) place += head->hits[w];
            all += head->hits[w];
        }
        if (j >= 0) { d.row_slot1[row + place] = i; d.row_slot2[row + place] = j; }
        base += all;
        __syncthreads();            // (the next chunk's counts overwrite this one's)
    }

    // 4.
    if (tid == 0) { d.count[q] = base; d.n_found[q] = 0; }
}

__global__ __launch_bounds__(kTmThreads) void k_tm_pack(const TmDev d)
{
    __shared__ int32_t sum_front[kWaves], sum_all[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t q = blockIdx.x;

    int32_t front = 0, all = 0;
    for (int32_t k = tid; k < d.n_queries; k += kTmThreads) {
        const int32_t c = d.count[k];
        all += c;
        if (k < q) front += c;
    }
    front = wave_sum(front);
    all = wave_sum(all);
    if (lane == 0) { sum_front[wave] = front; sum_all[wave] = all; }
    __syncthreads();
    front = 0; all = 0;
    for (int w = 0; w < kWaves; ++w) { front += sum_front[w]; all += sum_all[w]; }

    if (tid == 0) {
        d.pair_ptr[q] = front;
        if (q == d.n_queries - 1) d.pair_ptr[d.n_queries] = all;
    }
    const int32_t mine = d.count[q];
    for (int32_t k = tid; k < mine; k += kTmThreads) tm_place(d, q, k, front + k);
    // (all <= match_cap <= 2^28 and the stride <= 2^20: k does not wrap)
    const int32_t stride = (int32_t)gridDim.x * kTmThreads;
    for (int32_t k = all + q * kTmThreads + tid; k < d.match_cap; k += stride) tm_pad(d, k);
}

}  // namespace

hipError_t launch_track_match(const TmDev &d, int32_t max_slots, hipStream_t s)
{
    if (d.n_queries <= 0) return hipGetLastError();
    const size_t lds = tm_lds_bytes(max_slots);
    // (above the 64 KB a kernel may ask for unannounced; per device, so said where it is needed rather than once per process)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_tm_match), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tm_lds_bytes(MOVBA_MAX_TRACK_SLOTS));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_tm_match, dim3(d.n_queries), dim3(kTmThreads), lds, s, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tm_pack, dim3(d.n_queries), dim3(kTmThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
