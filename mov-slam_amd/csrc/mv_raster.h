// Device view + launch wrapper of movba_mv_raster (mv_raster.hip; host side: mv_raster.cpp), and the steps of the decoder's loop
// that have a serial meaning - the keep test, the rect of the destination block, the extent of the source block with its clamps,
// the slots of a pixel, the coverage ratio - as plain C++: what the kernels call, and what a host build runs record by record
// (mvr_frames), as advance.h does with adv_frames.  VideoDecoder.cc:198-351 as include/movba.h restates it.  Everything is
// integer arithmetic except the conversions of mv_pt and of the query points and the one fp64 division of the coverage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "advance.h"
#include "movba.h"

namespace movba {

// Everything the kernels read and write.  Inputs and scratch lie in device memory; `cover` and `tile_off` arrive cleared (one
// block of scratch, cover first); every out pointer is device memory or a device view of pinned host memory.  A frame is cut
// into tiles of 16 x 16 pixels, row-major, the tiles of frame f at tile_ptr[f]; a source extent spans at most 17 pixels per axis
// and so at most 2 x 2 tiles.
struct MvrDev {
    int32_t n_frames, n_records, n_q, n_grid, n_tiles, max_records;     // max_records: of one frame
    const int32_t *rows, *cols;                     // n_frames
    const int32_t *rec_ptr, *q_ptr, *g_ptr, *tile_ptr;      // n_frames + 1 (g_ptr: the lattices' rects; tile_ptr: the frames' tiles)
    const double *threshold;                        // n_frames
    const uint8_t *want_grid;                       // n_frames
    const int16_t *src_x, *src_y, *dst_x, *dst_y;   // n_records
    const uint8_t *w, *h;                           // n_records
    const float *q_pt;                              // n_q x 2
    // scratch
    int32_t *kept_rec;                              // n_records: [rec_ptr[f] + m] = the record that is the frame's kept record m
    int32_t *chunk_cnt;                             // kept records per chunk of kMvrKeepThreads records, the chunks of frame f at mvr_chunk_base
    int32_t *kept_cnt, *cover;                      // n_frames: kept records, the sum of their w * h
    int32_t *kept_base;                             // n_frames + 1: kept_ptr again, where the kernels read it
    int32_t *tile_off;                              // n_tiles + 1: records per tile, then where the tile's list starts
    int32_t *tile_cur;                              // n_tiles: where the next record of the tile goes
    int32_t *list_m;                                // 4 x n_records: the tiles' lists, the kept index m ...
    uint64_t *list_ext;                             // ... and its packed extent
    // out
    int32_t *kept_ptr, *kp_rect, *mv_dindx, *rec_kept, *cand, *grid_ptr, *cover_px;
    float *mv_pt;
    double *coverage_area;
    uint8_t *grid_covered, *force_grid;
};

constexpr int kMvrKeepThreads = 1024;               // k_mvr_count, k_mvr_keep: one chunk of records per workgroup; k_mvr_offsets: one workgroup
constexpr int kMvrKeepWaves = kMvrKeepThreads / 64;
constexpr int kMvrThreads = 256;                    // k_mvr_fill, k_mvr_query
constexpr int kMvrTile = 16, kMvrTileShift = 4;
constexpr int32_t kMvrMaxFrameRecords = 1 << 20;    // keeps cover_px <= 2^28

// the clearing of cover and tile_off, then k_mvr_count, k_mvr_keep, k_mvr_offsets, k_mvr_fill, k_mvr_query on the stream
hipError_t launch_mv_raster(const MvrDev &d, hipStream_t s);

// ---- the steps ----

struct MvrRec { int32_t sx, sy, dx, dy, w, h; };
struct MvrExtent { int32_t x0, y0, x1, y1; };       // both ends inclusive; empty when x0 > x1 or y0 > y1

__host__ __device__ inline MvrRec mvr_record(const MvrDev &d, size_t i)
{
    return MvrRec{ d.src_x[i], d.src_y[i], d.dst_x[i], d.dst_y[i], d.w[i], d.h[i] };
}
// where the chunk counts of frame f start: a frame of n records has ceil(n / kMvrKeepThreads) chunks, at most one more than the
// quotient, so the ranges do not meet; mvr_chunk_slots words hold them all
__host__ __device__ inline int32_t mvr_chunk_base(const int32_t *rec_ptr, int32_t f) { return rec_ptr[f] / kMvrKeepThreads + f; }
__host__ __device__ inline size_t mvr_chunk_slots(size_t n_records, size_t n_frames) { return n_records / kMvrKeepThreads + n_frames + 1; }
__host__ __device__ inline bool mvr_size_ok(int v) { return v == 4 || v == 8 || v == 16; }
// :236-241: only the high side is tested
__host__ __device__ inline bool mvr_keep(const MvrRec &r, int32_t W, int32_t H) { return !(r.dx + r.w / 2 >= W || r.dy + r.h / 2 >= H); }
// :230-235, :244: the corner is clamped, the size is not
__host__ __device__ inline void mvr_rect(const MvrRec &r, int32_t out[4])
{
    const int32_t x = r.dx - r.w / 2, y = r.dy - r.h / 2;
    out[0] = x < 0 ? 0 : x; out[1] = y < 0 ? 0 : y; out[2] = r.w; out[3] = r.h;
}
// :295-306 with ref == 0: src = dst - (dst - src)
__host__ __device__ inline MvrExtent mvr_extent(const MvrRec &r, int32_t W, int32_t H)
{
    MvrExtent e{ r.sx - r.w / 2, r.sy - r.h / 2, r.sx + r.w / 2, r.sy + r.h / 2 };
    if (e.x0 < 0) e.x0 = 0;
    if (e.y0 < 0) e.y0 = 0;
    if (e.x1 >= W) e.x1 = W - 1;
    if (e.y1 >= H) e.y1 = H - 1;
    return e;
}
__host__ __device__ inline bool mvr_empty(const MvrExtent &e) { return e.x0 > e.x1 || e.y0 > e.y1; }
// four int16: x0, y0 <= 32765, x1, y1 >= -32766 by the ranges of the record's fields
__host__ __device__ inline uint64_t mvr_pack(const MvrExtent &e)
{
    return (uint64_t)(uint16_t)e.x0 | ((uint64_t)(uint16_t)e.y0 << 16) | ((uint64_t)(uint16_t)e.x1 << 32) | ((uint64_t)(uint16_t)e.y1 << 48);
}
__host__ __device__ inline bool mvr_contains(uint64_t p, int32_t x, int32_t y)
{
    return x >= (int16_t)(uint16_t)p && y >= (int16_t)(uint16_t)(p >> 16) && x <= (int16_t)(uint16_t)(p >> 32) && y <= (int16_t)(uint16_t)(p >> 48);
}
__host__ __device__ inline int32_t mvr_tiles_across(int32_t extent) { return (extent + kMvrTile - 1) >> kMvrTileShift; }
__host__ __device__ inline int64_t mvr_tiles(int32_t rows, int32_t cols) { return (int64_t)mvr_tiles_across(rows) * mvr_tiles_across(cols); }
// visit(tile) for every tile of frame f that a non-empty extent touches (it lies inside the frame, so the tiles exist)
template <typename Visit> __host__ __device__ inline void mvr_for_tiles(const MvrDev &d, int32_t f, const MvrExtent &e, Visit visit)
{
    const int32_t across = mvr_tiles_across(d.cols[f]);
    for (int32_t ty = e.y0 >> kMvrTileShift; ty <= (e.y1 >> kMvrTileShift); ++ty)
        for (int32_t tx = e.x0 >> kMvrTileShift; tx <= (e.x1 >> kMvrTileShift); ++tx) visit(d.tile_ptr[f] + ty * across + tx);
}

// The slots of a pixel from the SET of kept records that contain it: the three smallest and, from four on, the largest - what
// the fill order of :336-343 leaves behind.
struct MvrSlots { int32_t low[3], high, k; };
__host__ __device__ inline MvrSlots mvr_no_slots() { return MvrSlots{ { INT32_MAX, INT32_MAX, INT32_MAX }, -1, 0 }; }
__host__ __device__ inline void mvr_add(MvrSlots &s, int32_t m)
{
    ++s.k;
    if (m > s.high) s.high = m;
    if (m < s.low[0]) { s.low[2] = s.low[1]; s.low[1] = s.low[0]; s.low[0] = m; }
    else if (m < s.low[1]) { s.low[2] = s.low[1]; s.low[1] = m; }
    else if (m < s.low[2]) s.low[2] = m;
}
__host__ __device__ inline int32_t mvr_slot(const MvrSlots &s, int c) { return c < 3 ? (c < s.k ? s.low[c] : -1) : (s.k >= 4 ? s.high : -1); }

// (int)pt: truncation toward zero; |pt| <= 2^20 by the call's checks, so the conversion is defined
__host__ __device__ inline int32_t mvr_pixel(float v) { return (int32_t)v; }
// :350 and MOVExtractor.cc:418; the sum is an integer below 2^28 here and in the reference's fp32
__host__ __device__ inline double mvr_area(int32_t cover, int32_t W, int32_t H) { return (double)cover / (double)((int64_t)W * H); }
__host__ __device__ inline bool mvr_force(double area, double threshold) { return area < threshold; }

// the largest f with ptr[f] <= k, f < n_frames (ptr ascends; k < ptr[n_frames])
__host__ __device__ inline int32_t mvr_frame_of(const int32_t *ptr, int32_t n_frames, int32_t k)
{
    int32_t lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- per element, what the kernels do (and mvr_frames, serially) ----

// k_mvr_keep, record i of frame f that is kept as the frame's m-th: rec_kept and kept_rec, and `count(tile)` for its tiles
// -> its area
template <typename Count> __host__ __device__ inline int32_t mvr_keep_record(const MvrDev &d, int32_t f, size_t i, int32_t m, Count count)
{
    const MvrRec r = mvr_record(d, i);
    d.rec_kept[i] = m;
    d.kept_rec[(size_t)d.rec_ptr[f] + m] = (int32_t)i;
    const MvrExtent e = mvr_extent(r, d.cols[f], d.rows[f]);
    if (!mvr_empty(e)) mvr_for_tiles(d, f, e, count);
    return r.w * r.h;
}
// k_mvr_offsets, per frame, once kept_base is known
__host__ __device__ inline void mvr_write_frame(const MvrDev &d, int32_t f)
{
    const double area = mvr_area(d.cover[f], d.cols[f], d.rows[f]);
    d.kept_ptr[f] = d.kept_base[f];
    d.grid_ptr[f] = d.g_ptr[f];
    d.cover_px[f] = d.cover[f];
    d.coverage_area[f] = area;
    d.force_grid[f] = mvr_force(area, d.threshold[f]);
    if (f == d.n_frames - 1) { d.kept_ptr[d.n_frames] = d.kept_base[d.n_frames]; d.grid_ptr[d.n_frames] = d.g_ptr[d.n_frames]; }
}
// k_mvr_fill, slot i of the records' range: the row of a kept record and its place in its tiles' lists (place(tile) -> where),
// and the padding row i behind the total
template <typename Place> __host__ __device__ inline void mvr_fill_slot(const MvrDev &d, int32_t i, Place place)
{
    const int32_t f = mvr_frame_of(d.rec_ptr, d.n_frames, i), m = i - d.rec_ptr[f];
    if (m < d.kept_cnt[f]) {
        const MvrRec r = mvr_record(d, (size_t)d.kept_rec[i]);
        const size_t o = (size_t)d.kept_base[f] + m;
        mvr_rect(r, d.kp_rect + 4 * o);
        d.mv_pt[2 * o] = (float)(r.dx - r.sx); d.mv_pt[2 * o + 1] = (float)(r.dy - r.sy);
        d.mv_dindx[o] = m;
        const MvrExtent e = mvr_extent(r, d.cols[f], d.rows[f]);
        if (!mvr_empty(e)) {
            const uint64_t packed = mvr_pack(e);
            mvr_for_tiles(d, f, e, [&](int32_t tile) {
                const int32_t at = place(tile);
                d.list_m[at] = m; d.list_ext[at] = packed;
            });
        }
    }
    if (i >= d.kept_base[d.n_frames]) {
        const size_t o = (size_t)i;
        for (int q = 0; q < 4; ++q) d.kp_rect[4 * o + q] = -1;
        d.mv_pt[2 * o] = d.mv_pt[2 * o + 1] = __builtin_nanf("");
        d.mv_dindx[o] = -1;
    }
}
// the slots of pixel (x, y) of frame f; four -1 outside the image
__host__ __device__ inline MvrSlots mvr_slots_at(const MvrDev &d, int32_t f, int32_t x, int32_t y)
{
    MvrSlots s = mvr_no_slots();
    if (x < 0 || y < 0 || x >= d.cols[f] || y >= d.rows[f]) return s;
    const int32_t tile = d.tile_ptr[f] + (y >> kMvrTileShift) * mvr_tiles_across(d.cols[f]) + (x >> kMvrTileShift);
    for (int32_t at = d.tile_off[tile]; at < d.tile_off[tile + 1]; ++at)
        if (mvr_contains(d.list_ext[at], x, y)) mvr_add(s, d.list_m[at]);
    return s;
}
// k_mvr_query, query j: a point query (j < n_q) or a lattice rect
__host__ __device__ inline void mvr_query(const MvrDev &d, int32_t j)
{
    if (j < d.n_q) {
        const int32_t f = mvr_frame_of(d.q_ptr, d.n_frames, j);
        const MvrSlots s = mvr_slots_at(d, f, mvr_pixel(d.q_pt[2 * (size_t)j]), mvr_pixel(d.q_pt[2 * (size_t)j + 1]));
        for (int c = 0; c < 4; ++c) d.cand[4 * (size_t)j + c] = mvr_slot(s, c);
        return;
    }
    const int32_t g = j - d.n_q, f = mvr_frame_of(d.g_ptr, d.n_frames, g);
    if (!d.want_grid[f]) { d.grid_covered[g] = 0; return; }
    const int32_t k = g - d.g_ptr[f], nx = adv_lattice_nx(d.cols[f]);
    d.grid_covered[g] = mvr_slots_at(d, f, (k % nx) * 16 + 8, (k / nx) * 16 + 8).k > 0;
}

// ---- the whole call on one thread, in the kernels' order ----

inline void mvr_frames(const MvrDev &d)
{
    // k_mvr_count, k_mvr_keep (cover and tile_off arrive cleared)
    for (int32_t f = 0; f < d.n_frames; ++f) {
        int32_t m = 0, cover = 0;
        for (size_t i = (size_t)d.rec_ptr[f]; i < (size_t)d.rec_ptr[f + 1]; ++i) {
            if (!mvr_keep(mvr_record(d, i), d.cols[f], d.rows[f])) { d.rec_kept[i] = -1; continue; }
            cover += mvr_keep_record(d, f, i, m, [&](int32_t tile) { ++d.tile_off[tile]; });
            ++m;
        }
        d.kept_cnt[f] = m; d.cover[f] = cover;
    }
    // k_mvr_offsets
    d.kept_base[0] = 0;
    for (int32_t f = 0; f < d.n_frames; ++f) d.kept_base[f + 1] = d.kept_base[f] + d.kept_cnt[f];
    for (int32_t f = 0; f < d.n_frames; ++f) mvr_write_frame(d, f);
    int32_t at = 0;
    for (int32_t t = 0; t < d.n_tiles; ++t) { const int32_t c = d.tile_off[t]; d.tile_off[t] = d.tile_cur[t] = at; at += c; }
    d.tile_off[d.n_tiles] = at;
    // k_mvr_fill
    for (int32_t i = 0; i < d.n_records; ++i) mvr_fill_slot(d, i, [&](int32_t tile) { return d.tile_cur[tile]++; });
    // k_mvr_query
    for (int32_t j = 0; j < d.n_q + d.n_grid; ++j) mvr_query(d, j);
}

}  // namespace movba
