// Device view + launch wrapper of movba_track_match (track_match.hip; host side: track_match.cpp), and the steps of one query that
// have a serial meaning - the hash, the probe order, what "lowest slot" means, the order of a query's matches, the padding
// values - as plain C++ (what k_tm_match and k_tm_pack call from their lanes, and what a host build runs query by query:
// tm_query, tm_pack): the track-id joins of MOVMatcher (MOVMatcher.h:35-168 and the keypoint loop of Fuse, :249-273), as
// include/movba.h restates them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "movba.h"

namespace movba {

// Everything the kernels read and write.  Inputs lie in device memory, every index in them checked by the host; `row_*` and
// `count` are device scratch; every out pointer is device memory or a device view of pinned host memory (the staging buffer, or
// the caller's movba_host_alloc arrays).  The payload travels as 64-bit words: it is copied, never computed with.
struct TmDev {
    int32_t n_queries, match_cap;
    const int32_t *view_ptr, *slot_track;           // the slots of view v: [view_ptr[v], view_ptr[v + 1])
    const uint8_t *slot_taken;                      // n_slots, or nullptr: none
    const uint64_t *slot_obs, *slot_ur, *slot_depth;        // n_slots x 2, n_slots, n_slots, or nullptr
    const int32_t *query_mode, *query_view;         // n_queries, n_queries x 2
    const int32_t *query_ptr, *item_track;          // the items of query q: item_track[query_ptr[q] .. query_ptr[q + 1])
    const int32_t *row_base;                        // n_queries + 1: prefix of view 1's slot counts over the TRIANGULATION queries
    int32_t *row_slot1, *row_slot2, *count;         // scratch: match_cap, match_cap (query q's matches from row_base[q] on), n_queries
    int32_t *pair_ptr, *match_slot1, *match_slot2;  // out: n_queries + 1, match_cap, match_cap
    uint64_t *obs1, *obs2, *ur1, *ur2, *depth1, *depth2;    // out: match_cap (x 2 for obs), or nullptr
    int32_t *item_slot, *n_found;                   // out: n_items, n_queries
};

constexpr int kTmThreads = 256;
// front of k_tm_match's LDS: the scratch of its scans; the table lies behind it
constexpr size_t kTmLdsHead = 128;
// what stands behind the last match: a slot index no slot has, and one quiet NaN
constexpr int32_t kTmPadSlot = -1;
constexpr uint64_t kTmPadBits = 0x7ff8000000000000ull;
// an entry of the table that holds no slot.  The table holds slot indices, not ids: no id value is reserved.
constexpr int32_t kTmEmpty = -1;

__host__ __device__ inline int32_t tm_pow2ceil(int32_t n)
{
    int32_t m = 1;
    while (m < n) m <<= 1;
    return m;
}

// entries of the table over a view of n slots: at most half of them are ever occupied, so every probe sequence ends
__host__ __device__ inline int32_t tm_table_entries(int32_t n_slots) { return 2 * tm_pow2ceil(n_slots); }

// LDS of one workgroup of k_tm_match: head | the table.  131 200 bytes at MOVBA_MAX_TRACK_SLOTS.
inline size_t tm_lds_bytes(int32_t n_slots) { return kTmLdsHead + 4 * (size_t)tm_table_entries(n_slots); }

// k_tm_match over all queries, then k_tm_pack, on the stream; max_slots: the largest view any query builds its table over
hipError_t launch_track_match(const TmDev &d, int32_t max_slots, hipStream_t s);

// ---- the steps ----

// where the probe sequence of an id starts (any int32 is an id: the bits are mixed as they are)
__host__ __device__ inline uint32_t tm_hash(int32_t id)
{
    uint32_t x = (uint32_t)id;
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// insert slot j of a view (track: the view's ids, slot order) into its table of `entries` entries.  The sequence of an id is
// hash, hash + 1, ...; it takes the first empty entry it meets, or joins the entry whose occupant carries the same id, where the
// LOWER slot stays: the first insertion in slot order wins (std::map::insert into mvVFMap, the ascending scans with `break`).
// On the device other lanes insert at the same time: an empty entry is taken by compare-and-swap, a shared one by an atomic
// minimum, so an entry only ever changes to a slot of the same id and the lowest slot wins whatever the order of the lanes.
__host__ __device__ inline void tm_insert(int32_t *table, int32_t entries, const int32_t *track, int32_t j)
{
    const int32_t id = track[j];
    const uint32_t mask = (uint32_t)entries - 1;
    for (uint32_t e = tm_hash(id) & mask;; e = (e + 1) & mask) {
#if defined(__HIP_DEVICE_COMPILE__)
        int32_t cur = table[e];
        if (cur == kTmEmpty) {
            cur = atomicCAS(table + e, kTmEmpty, j);
            if (cur == kTmEmpty) return;
        }
        if (track[cur] == id) { atomicMin(table + e, j); return; }
#else
        const int32_t cur = table[e];
        if (cur == kTmEmpty) { table[e] = j; return; }
        if (track[cur] == id) { if (j < cur) table[e] = j; return; }
#endif
    }
}

// the lowest inserted slot that carries `id`, or -1: the same sequence, ended by the id or by an empty entry
__host__ __device__ inline int32_t tm_find(const int32_t *table, int32_t entries, const int32_t *track, int32_t id)
{
    const uint32_t mask = (uint32_t)entries - 1;
    for (uint32_t e = tm_hash(id) & mask;; e = (e + 1) & mask) {
        const int32_t cur = table[e];
        if (cur == kTmEmpty) return -1;
        if (track[cur] == id) return cur;
    }
}

// is slot j of a view part of a TRIANGULATION join (GetMapPointMatches()[j] == NULL, MOVMatcher.h:146, :152)
__host__ __device__ inline bool tm_free(const uint8_t *taken, int32_t j) { return !taken || !taken[j]; }

// One query's join on one thread, the steps in the kernel's order.  Scratch: table, tm_table_entries(slots of the view searched).
inline void tm_query(const TmDev &d, int32_t q, int32_t *table)
{
    const bool lookup = d.query_mode[q] == MOVBA_TM_LOOKUP;
    const int32_t v1 = d.query_view[2 * q], v2 = d.query_view[2 * q + 1];
    const int32_t b2 = d.view_ptr[v2], n2 = d.view_ptr[v2 + 1] - b2;
    const int32_t *track2 = d.slot_track + b2;
    const uint8_t *taken2 = d.slot_taken ? d.slot_taken + b2 : nullptr;
    const int32_t entries = tm_table_entries(n2);
    for (int32_t e = 0; e < entries; ++e) table[e] = kTmEmpty;
    for (int32_t j = 0; j < n2; ++j)
        if (lookup || tm_free(taken2, j)) tm_insert(table, entries, track2, j);
    if (lookup) {
        int32_t found = 0;
        for (int32_t i = d.query_ptr[q]; i < d.query_ptr[q + 1]; ++i) {
            const int32_t j = tm_find(table, entries, track2, d.item_track[i]);
            d.item_slot[i] = j;
            found += j >= 0;
        }
        d.n_found[q] = found;
        d.count[q] = 0;
        return;
    }
    const int32_t b1 = d.view_ptr[v1], n1 = d.view_ptr[v1 + 1] - b1;
    const uint8_t *taken1 = d.slot_taken ? d.slot_taken + b1 : nullptr;
    int32_t n = 0;
    for (int32_t i = 0; i < n1; ++i) {
        if (!tm_free(taken1, i)) continue;
        const int32_t j = tm_find(table, entries, track2, d.slot_track[b1 + i]);
        if (j < 0) continue;
        d.row_slot1[d.row_base[q] + n] = i;
        d.row_slot2[d.row_base[q] + n] = j;
        ++n;
    }
    d.count[q] = n;
    d.n_found[q] = 0;
}

// match k of query q to its dense place `dst`, with the payload of its two slots
__host__ __device__ inline void tm_place(const TmDev &d, int32_t q, int32_t k, int32_t dst)
{
    const int32_t s1 = d.row_slot1[d.row_base[q] + k], s2 = d.row_slot2[d.row_base[q] + k];
    const size_t g1 = (size_t)d.view_ptr[d.query_view[2 * q]] + (size_t)s1, g2 = (size_t)d.view_ptr[d.query_view[2 * q + 1]] + (size_t)s2;
    d.match_slot1[dst] = s1;
    d.match_slot2[dst] = s2;
    if (d.obs1) { d.obs1[2 * (size_t)dst] = d.slot_obs[2 * g1]; d.obs1[2 * (size_t)dst + 1] = d.slot_obs[2 * g1 + 1]; }
    if (d.obs2) { d.obs2[2 * (size_t)dst] = d.slot_obs[2 * g2]; d.obs2[2 * (size_t)dst + 1] = d.slot_obs[2 * g2 + 1]; }
    if (d.ur1) d.ur1[dst] = d.slot_ur[g1];
    if (d.ur2) d.ur2[dst] = d.slot_ur[g2];
    if (d.depth1) d.depth1[dst] = d.slot_depth[g1];
    if (d.depth2) d.depth2[dst] = d.slot_depth[g2];
}

// entry k behind the last match
__host__ __device__ inline void tm_pad(const TmDev &d, int32_t k)
{
    d.match_slot1[k] = kTmPadSlot;
    d.match_slot2[k] = kTmPadSlot;
    if (d.obs1) { d.obs1[2 * (size_t)k] = kTmPadBits; d.obs1[2 * (size_t)k + 1] = kTmPadBits; }
    if (d.obs2) { d.obs2[2 * (size_t)k] = kTmPadBits; d.obs2[2 * (size_t)k + 1] = kTmPadBits; }
    if (d.ur1) d.ur1[k] = kTmPadBits;
    if (d.ur2) d.ur2[k] = kTmPadBits;
    if (d.depth1) d.depth1[k] = kTmPadBits;
    if (d.depth2) d.depth2[k] = kTmPadBits;
}

// the second pass on one thread: the prefix of the counts, the rows to their dense places, the tail
inline void tm_pack(const TmDev &d)
{
    int32_t at = 0;
    for (int32_t q = 0; q < d.n_queries; ++q) {
        d.pair_ptr[q] = at;
        for (int32_t k = 0; k < d.count[q]; ++k) tm_place(d, q, k, at + k);
        at += d.count[q];
    }
    d.pair_ptr[d.n_queries] = at;
    for (int32_t k = at; k < d.match_cap; ++k) tm_pad(d, k);
}

}  // namespace movba
