// Device view + launch wrapper of movba_advance (advance.hip; host side: advance.cpp), and the steps of the walk that have a
// serial meaning - the sort key, the rect of a vector with its fp32 operations and its truncation, the candidate loop's
// comparison, the claim rule, the gate, the id arithmetic - as plain C++: what the kernels call, and what a host build runs
// frame by frame (adv_frames), as express.h does with ex_item.  MOVExtractor.cc:245-335, :380-451 as include/movba.h restates
// them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "express.h"
#include "movba.h"

namespace movba {

// Everything the kernels read and write.  Inputs and scratch lie in device memory; `claim` arrives filled with kAdvNoClaim with
// the inputs; every out pointer is device memory or a device view of pinned host memory.  A frame's wave items are its previous
// features (by input index), then its macroblocks, then its lattice rects: item_base(f) = prev_ptr[f] + kp_ptr[f] + g_ptr[f].
struct AdvDev {
    int32_t n_frames, n_items, max_prev;            // n_items = n_prev + n_kps + n_grid = the capacity of the feature list
    const uint8_t *pixels;                          // the frames that have items, rows tight
    const int32_t *img_off, *rows, *cols, *threshold, *force_grid, *first_id;      // n_frames
    const int32_t *prev_ptr, *mv_ptr, *kp_ptr, *g_ptr;                             // n_frames + 1 (g_ptr: the lattices' rects)
    const float *prev_pt, *mv_pt;                   // n_prev x 2, n_mv x 2
    const int32_t *prev_mb, *prev_age, *prev_track, *prev_cand;    // n_prev x 2, n_prev, n_prev, n_prev x 4
    const uint64_t *prev_desc;                      // n_prev x 4
    const uint8_t *prev_coverage, *covered;         // n_prev, n_grid (zeros where the caller gave none)
    const int32_t *mv_dindx, *kp_rect;              // n_mv, n_kps x 4
    // scratch
    int32_t *claim;                                 // n_kps: the lowest position that reached the macroblock
    int32_t *pos, *ord;                             // n_prev: the position of an input index; `order` again, where the kernels read it
                                                    // (the caller's may lie in pinned host memory)
    uint64_t *it_desc;                              // n_items x 4: the final / detected descriptor
    int32_t *it_code, *it_rank;                     // n_items: pre-fate, then fate, or MOVBA_EX_*; the place in its segment or -1
    float *pf_pt;                                   // n_prev x 2: the fp32 sum
    int32_t *pf_xy, *pf_d, *pf_dist;                // n_prev x 2, n_prev, n_prev: the final rect's corner, dindx of the chosen vector, the final distance
    int32_t *counts;                                // n_frames x 3: kept, new, grid features
    // out
    int32_t *order, *chosen_mv, *distance, *mov_cnt, *next_id, *seg_ptr;
    uint8_t *fate, *kp_found, *kp_code, *grid_ran;
    int32_t *feat_src, *feat_track, *feat_rect, *feat_age;
    float *feat_pt;
    uint64_t *feat_desc;
};

constexpr int kAdvThreads = 256;
constexpr int kAdvSortThreads = 1024;                // k_adv_sort: a pass of the network is m / 2 pairs between two barriers
constexpr int kAdvEmitChunks = 64;                  // k_adv_emit: at most that many workgroups share a frame's items
constexpr int kAdvWaves = kAdvThreads / 64;         // wave items of one workgroup of k_adv_blocks
constexpr int32_t kAdvNoClaim = 0x7f7f7f7f;         // (one byte value: the host fills `claim` with memset)
constexpr int kAdvArrives = 0;                      // it_code of a previous feature between k_adv_blocks and k_adv_resolve
constexpr int kAdvGate = 40, kAdvMinMoves = 60;

// k_adv_sort, k_adv_blocks, k_adv_resolve, k_adv_emit on the stream
hipError_t launch_advance(const AdvDev &d, hipStream_t s);

// ---- the steps ----

__host__ __device__ inline int32_t adv_pow2ceil(int32_t n) { int32_t m = 1; while (m < n) m <<= 1; return m; }

// The sort key of input index `idx`: ascending keys are age descending, then desc.count() descending, then idx ascending (the
// tie rule).  31 + 9 + 14 bits; the padding of the bitonic sort, all ones, is above every key.
__host__ __device__ inline uint64_t adv_key(int32_t age, int count, int32_t idx)
{
    return ((uint64_t)(uint32_t)(INT32_MAX - age) << 23) | ((uint64_t)(256 - count) << 14) | (uint64_t)idx;
}
__host__ __device__ inline int32_t adv_key_index(uint64_t key) { return (int32_t)(key & 16383u); }

// pt = prev_pt + mv_pt: one fp32 add (no product stands beside it, so nothing can be contracted into it; the device build names
// the rounding all the same)
__host__ __device__ inline float adv_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    volatile float s = a + b;
    return s;
#endif
}
// (int)(pt - (float)(extent / 2)): the integer quotient, one fp32 subtract, truncation toward zero.  |pt| <= 2^21 by the call's
// checks, so the conversion is defined.
__host__ __device__ inline int32_t adv_corner(float pt, int32_t extent)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int32_t)__fsub_rn(pt, (float)(extent / 2));
#else
    volatile float s = pt - (float)(extent / 2);
    return (int32_t)s;
#endif
}

__host__ __device__ inline int adv_distance(const uint64_t a[4], const uint64_t b[4])
{
    return ex_popc(a[0] ^ b[0]) + ex_popc(a[1] ^ b[1]) + ex_popc(a[2] ^ b[2]) + ex_popc(a[3] ^ b[3]);
}
// the candidate loop's comparison: strict, so ties keep the earlier j
__host__ __device__ inline bool adv_better(int dist, int best) { return dist < best; }
// lbFound: the lowest position wins
__host__ __device__ inline int32_t adv_claim(int32_t held, int32_t position) { return position < held ? position : held; }
// the fate of a feature that arrived: d = dindx of its vector, holder = claim[d] (unused when d < 0)
__host__ __device__ inline int adv_fate(int32_t d, int32_t holder, int32_t position, int dist)
{
    if (d >= 0 && holder != position) return MOVBA_ADV_LOST_CLAIM;
    return dist <= kAdvGate ? MOVBA_ADV_KEPT : MOVBA_ADV_FAR;
}
__host__ __device__ inline bool adv_grid_runs(int force_grid, int32_t mov_cnt) { return force_grid || mov_cnt < kAdvMinMoves; }
// trackId = ++mCurrentId: the r-th new feature, then the r-th grid feature behind the n_new new ones
__host__ __device__ inline int32_t adv_new_id(int32_t first_id, int32_t r) { return first_id + 1 + r; }
__host__ __device__ inline int32_t adv_grid_id(int32_t first_id, int32_t n_new, int32_t r) { return first_id + 1 + n_new + r; }

// the lattice of extract_moves (movba_express_grid): its rects per row, its size, rect g
__host__ __device__ inline int32_t adv_lattice_nx(int32_t cols) { return cols <= 16 ? 0 : (cols - 17) / 16 + 1; }
__host__ __device__ inline int64_t adv_lattice(int32_t rows, int32_t cols) { return (int64_t)adv_lattice_nx(rows) * adv_lattice_nx(cols); }

__host__ __device__ inline int32_t adv_item_base(const AdvDev &d, int32_t f) { return d.prev_ptr[f] + d.kp_ptr[f] + d.g_ptr[f]; }
// the frame of wave item k (the bases ascend)
__host__ __device__ inline int32_t adv_frame_of(const AdvDev &d, int32_t k)
{
    int32_t lo = 0, hi = d.n_frames - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (adv_item_base(d, mid) <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One wave item: a previous feature (up to five descriptors, the choice, the final distance, the claim), a macroblock or a
// lattice rect (DETECT).  block(f, x, y, w, h, mode, desc) -> MOVBA_EX_*: ex_reject, then the block's steps - the wavefront's routine
// in k_adv_blocks, where every lane runs this with the same values and `writer` is lane 0, or ex_block on one thread.
template <typename Block> __host__ __device__ inline void adv_item(const AdvDev &d, int32_t k, bool writer, Block block)
{
    const int32_t f = adv_frame_of(d, k), j = k - adv_item_base(d, f);
    const int32_t np = d.prev_ptr[f + 1] - d.prev_ptr[f], nk = d.kp_ptr[f + 1] - d.kp_ptr[f];
    uint64_t desc[4] = { 0, 0, 0, 0 };
    if (j >= np) {
        // a macroblock (:380-416) or a lattice rect (:418-451): whether it is emitted is k_adv_resolve's
        int32_t x, y, w, h;
        if (j < np + nk) {
            const int32_t *r = d.kp_rect + 4 * (size_t)(d.kp_ptr[f] + j - np);
            x = r[0]; y = r[1]; w = r[2]; h = r[3];
        } else {
            const int32_t g = j - np - nk, nx = adv_lattice_nx(d.cols[f]);
            x = (g % nx) * 16; y = (g / nx) * 16; w = 16; h = 16;
        }
        const int code = block(f, x, y, w, h, MOVBA_EX_DETECT, desc);
        if (writer) {
            d.it_code[k] = code;
            for (int q = 0; q < 4; ++q) d.it_desc[4 * (size_t)k + q] = desc[q];
        }
        return;
    }
    const size_t g = (size_t)d.prev_ptr[f] + j;
    const int32_t *cand = d.prev_cand + 4 * g;
    if (d.prev_coverage[g] || cand[0] == -1) {
        if (writer) {
            d.it_code[k] = d.prev_coverage[g] ? MOVBA_ADV_COVERAGE : MOVBA_ADV_NO_MV;
            d.chosen_mv[g] = -1; d.distance[g] = -1;
        }
        return;
    }
    const int32_t w = d.prev_mb[2 * g], h = d.prev_mb[2 * g + 1];
    const float px = d.prev_pt[2 * g], py = d.prev_pt[2 * g + 1];
    const uint64_t *ref = d.prev_desc + 4 * g;
    const float *mv = d.mv_pt + 2 * (size_t)d.mv_ptr[f];
    int32_t indx = cand[0];
    if (cand[1] >= 0) {
        int best = 256;
        for (int c = 0; c < 4 && cand[c] != -1; ++c) {
            const float qx = adv_add(px, mv[2 * (size_t)cand[c]]), qy = adv_add(py, mv[2 * (size_t)cand[c] + 1]);
            if (block(f, adv_corner(qx, w), adv_corner(qy, h), w, h, MOVBA_EX_DESCRIBE, desc) != MOVBA_EX_DESCRIBED) continue;
            const int dist = adv_distance(ref, desc);
            if (adv_better(dist, best)) { best = dist; indx = cand[c]; }
        }
    }
    const float qx = adv_add(px, mv[2 * (size_t)indx]), qy = adv_add(py, mv[2 * (size_t)indx + 1]);
    const int32_t x = adv_corner(qx, w), y = adv_corner(qy, h);
    const bool inside = block(f, x, y, w, h, MOVBA_EX_DESCRIBE, desc) == MOVBA_EX_DESCRIBED;
    if (!writer) return;
    d.chosen_mv[g] = indx;
    if (!inside) { d.it_code[k] = MOVBA_ADV_REJ_BOUNDS; d.distance[g] = -1; return; }
    const int32_t dst = d.mv_dindx[d.mv_ptr[f] + indx];
    const int dist = adv_distance(ref, desc);
    d.distance[g] = dist; d.pf_dist[g] = dist;
    d.it_code[k] = kAdvArrives;
    for (int q = 0; q < 4; ++q) d.it_desc[4 * (size_t)k + q] = desc[q];
    d.pf_pt[2 * g] = qx; d.pf_pt[2 * g + 1] = qy;
    d.pf_xy[2 * g] = x; d.pf_xy[2 * g + 1] = y;
    d.pf_d[g] = dst;
    if (dst >= 0) {
        int32_t *held = d.claim + d.kp_ptr[f] + dst;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicMin(held, d.pos[g]);                  // (a minimum: the result does not depend on who comes first)
#else
        *held = adv_claim(*held, d.pos[g]);
#endif
    }
}

// ---- per element, what k_adv_resolve and k_adv_emit decide (and adv_frames, serially) ----

// the fate of the feature with input index g (frame f), from what adv_item left; also left in it_code
__host__ __device__ inline int adv_settle(const AdvDev &d, int32_t f, size_t g)
{
    const int32_t k = adv_item_base(d, f) + (int32_t)(g - (size_t)d.prev_ptr[f]);
    int fate = d.it_code[k];
    if (fate == kAdvArrives) {
        const int32_t dst = d.pf_d[g];
        fate = adv_fate(dst, dst >= 0 ? d.claim[d.kp_ptr[f] + dst] : 0, d.pos[g], d.pf_dist[g]);
        d.it_code[k] = fate;
    }
    d.fate[g] = (uint8_t)fate;
    return fate;
}
// macroblock m of frame f: whether it is a feature of the new segment (nobody claimed it and DETECT passed) ...
__host__ __device__ inline bool adv_kp_new(const AdvDev &d, int32_t f, int32_t m)
{
    const int32_t k = adv_item_base(d, f) + (d.prev_ptr[f + 1] - d.prev_ptr[f]) + m;
    return d.claim[d.kp_ptr[f] + m] == kAdvNoClaim && d.it_code[k] == MOVBA_EX_FEATURE;
}
// ... and its kp_found and kp_code
__host__ __device__ inline void adv_write_kp(const AdvDev &d, int32_t f, int32_t m)
{
    const int32_t k = adv_item_base(d, f) + (d.prev_ptr[f + 1] - d.prev_ptr[f]) + m;
    const bool found = d.claim[d.kp_ptr[f] + m] != kAdvNoClaim;
    d.kp_found[d.kp_ptr[f] + m] = found;
    d.kp_code[d.kp_ptr[f] + m] = found ? 0 : (uint8_t)d.it_code[k];
}
__host__ __device__ inline bool adv_grid_feature(const AdvDev &d, int32_t f, int32_t g)
{
    const int32_t k = adv_item_base(d, f) + (d.prev_ptr[f + 1] - d.prev_ptr[f]) + (d.kp_ptr[f + 1] - d.kp_ptr[f]) + g;
    return d.it_code[k] == MOVBA_EX_FEATURE && !d.covered[d.g_ptr[f] + g];
}
// what is written for a frame once its three counts are known
__host__ __device__ inline void adv_write_counts(const AdvDev &d, int32_t f, int32_t kept, int32_t fresh, int32_t grid)
{
    d.counts[3 * f] = kept; d.counts[3 * f + 1] = fresh; d.counts[3 * f + 2] = grid;
    d.mov_cnt[f] = fresh;
    d.grid_ran[f] = adv_grid_runs(d.force_grid[f], fresh);
    d.next_id[f] = d.first_id[f] + fresh + grid;
}
__host__ __device__ inline void adv_write_segments(const AdvDev &d, int32_t f, int32_t base, int32_t total)
{
    d.seg_ptr[4 * f] = base;
    d.seg_ptr[4 * f + 1] = base + d.counts[3 * f];
    d.seg_ptr[4 * f + 2] = base + d.counts[3 * f] + d.counts[3 * f + 1];
    d.seg_ptr[4 * f + 3] = base + d.counts[3 * f] + d.counts[3 * f + 1] + d.counts[3 * f + 2];
    if (f == d.n_frames - 1) d.seg_ptr[4 * d.n_frames] = total;
}
// the row of wave item k of frame f in the feature list, if it has one (it_rank >= 0); base = where the frame starts
__host__ __device__ inline void adv_emit_item(const AdvDev &d, int32_t f, int32_t k, int32_t base)
{
    const int32_t r = d.it_rank[k];
    if (r < 0) return;
    const int32_t j = k - adv_item_base(d, f), np = d.prev_ptr[f + 1] - d.prev_ptr[f], nk = d.kp_ptr[f + 1] - d.kp_ptr[f];
    const int32_t kept = d.counts[3 * f], fresh = d.counts[3 * f + 1];
    size_t o;
    int32_t src, track, age, x, y, w, h;
    float px, py;
    if (j < np) {
        const size_t g = (size_t)d.prev_ptr[f] + j;
        o = (size_t)base + r;
        src = d.pos[g]; track = d.prev_track[g]; age = d.prev_age[g] + 1;
        x = d.pf_xy[2 * g]; y = d.pf_xy[2 * g + 1]; w = d.prev_mb[2 * g]; h = d.prev_mb[2 * g + 1];
        px = d.pf_pt[2 * g]; py = d.pf_pt[2 * g + 1];
    } else if (j < np + nk) {
        const int32_t *rc = d.kp_rect + 4 * (size_t)(d.kp_ptr[f] + j - np);
        o = (size_t)base + kept + r;
        src = j - np; track = adv_new_id(d.first_id[f], r); age = 0;
        x = rc[0]; y = rc[1]; w = rc[2]; h = rc[3];
        px = (float)(x + w / 2); py = (float)(y + h / 2);
    } else {
        const int32_t g = j - np - nk, nx = adv_lattice_nx(d.cols[f]);
        o = (size_t)base + kept + fresh + r;
        src = g; track = adv_grid_id(d.first_id[f], fresh, r); age = 0;
        x = (g % nx) * 16; y = (g / nx) * 16; w = 16; h = 16;
        px = (float)(x + 8); py = (float)(y + 8);
    }
    d.feat_src[o] = src; d.feat_track[o] = track; d.feat_age[o] = age;
    d.feat_pt[2 * o] = px; d.feat_pt[2 * o + 1] = py;
    d.feat_rect[4 * o] = x; d.feat_rect[4 * o + 1] = y; d.feat_rect[4 * o + 2] = w; d.feat_rect[4 * o + 3] = h;
    for (int q = 0; q < 4; ++q) d.feat_desc[4 * o + q] = d.it_desc[4 * (size_t)k + q];
}
// entry o of the feature list behind the total
__host__ __device__ inline void adv_pad(const AdvDev &d, size_t o)
{
    d.feat_src[o] = -1; d.feat_track[o] = -1; d.feat_age[o] = -1;
    d.feat_pt[2 * o] = d.feat_pt[2 * o + 1] = __builtin_nanf("");
    for (int q = 0; q < 4; ++q) { d.feat_rect[4 * o + q] = -1; d.feat_desc[4 * o + q] = 0; }
}

// ---- the whole call on one thread, in the kernels' order ----

inline void adv_frames(const AdvDev &d)
{
    auto block = [&](int32_t f, int32_t x, int32_t y, int32_t w, int32_t h, int mode, uint64_t desc[4]) {
        int pass, code = ex_reject(x, y, w, h, d.rows[f], d.cols[f]);
        desc[0] = desc[1] = desc[2] = desc[3] = 0;
        if (!code) code = ex_block(d.pixels + d.img_off[f] + (size_t)y * d.cols[f] + x, d.cols[f], w, h, d.threshold[f], mode, desc, &pass);
        return code;
    };
    // k_adv_sort
    for (int32_t f = 0; f < d.n_frames; ++f) {
        const int32_t p0 = d.prev_ptr[f], n = d.prev_ptr[f + 1] - p0;
        std::vector<uint64_t> keys((size_t)n);
        for (int32_t i = 0; i < n; ++i) keys[(size_t)i] = adv_key(d.prev_age[p0 + i], ex_popc256(d.prev_desc + 4 * (size_t)(p0 + i)), i);
        std::sort(keys.begin(), keys.end());
        for (int32_t i = 0; i < n; ++i) { d.order[p0 + i] = d.ord[p0 + i] = adv_key_index(keys[(size_t)i]); d.pos[p0 + adv_key_index(keys[(size_t)i])] = i; }
    }
    // k_adv_blocks
    for (int32_t k = 0; k < d.n_items; ++k) adv_item(d, k, true, block);
    // k_adv_resolve
    for (int32_t f = 0; f < d.n_frames; ++f) {
        const int32_t p0 = d.prev_ptr[f], np = d.prev_ptr[f + 1] - p0, nk = d.kp_ptr[f + 1] - d.kp_ptr[f], ng = d.g_ptr[f + 1] - d.g_ptr[f];
        const int32_t base = adv_item_base(d, f);
        int32_t kept = 0, fresh = 0, grid = 0;
        for (int32_t i = 0; i < np; ++i) {
            const int32_t idx = d.ord[p0 + i];
            d.it_rank[base + idx] = adv_settle(d, f, (size_t)p0 + idx) == MOVBA_ADV_KEPT ? kept++ : -1;
        }
        for (int32_t m = 0; m < nk; ++m) { adv_write_kp(d, f, m); d.it_rank[base + np + m] = adv_kp_new(d, f, m) ? fresh++ : -1; }
        const bool runs = adv_grid_runs(d.force_grid[f], fresh);
        for (int32_t g = 0; g < ng; ++g) d.it_rank[base + np + nk + g] = runs && adv_grid_feature(d, f, g) ? grid++ : -1;
        adv_write_counts(d, f, kept, fresh, grid);
    }
    // k_adv_emit
    int32_t total = 0, at = 0;
    for (int32_t f = 0; f < d.n_frames; ++f) total += d.counts[3 * f] + d.counts[3 * f + 1] + d.counts[3 * f + 2];
    for (int32_t f = 0; f < d.n_frames; ++f) {
        adv_write_segments(d, f, at, total);
        for (int32_t k = adv_item_base(d, f); k < adv_item_base(d, f + 1); ++k) adv_emit_item(d, f, k, at);
        at += d.counts[3 * f] + d.counts[3 * f + 1] + d.counts[3 * f + 2];
    }
    for (int32_t o = total; o < d.n_items; ++o) adv_pad(d, (size_t)o);
}

}  // namespace movba
