// The kernels of movba_mv_raster (include/movba.h): the clearing of the coverage sums and the tile counts and five launches on
// one stream.  The 4-channel image of the reference is never formed: a frame is cut into tiles of 16 x 16 pixels, every kept
// record is listed in the at most 2 x 2 tiles its source extent touches, and a query reads the one list of its pixel's tile.
//
// k_mvr_count: one workgroup of 1024 threads per chunk of 1024 records of a frame: the keep test, a ballot per wavefront, the
//   chunk's number of kept records.
// k_mvr_keep: the same grid.  The carry of a chunk is the sum of the counts of the frame's chunks before it (at most 1024, one
//   per thread); the dense index of a kept record is the carry, the counts of the wavefronts before its own and its rank in
//   the ballot, so it ascends with the record.  rec_kept, the inverse kept_rec, one integer atomic add per touched tile, and
//   one integer atomic add of the chunk's area on the frame's sum.  Integer sums: scheduling cannot change them.  (One
//   workgroup per FRAME walking its chunks with a running count took 4.5 us per chunk - each round waits for its loads, its
//   stores and its atomics before the barrier - 36 us for 8 000 records and 149 us for 32 000: DESIGN.md 4k.)
// k_mvr_offsets: one workgroup.  The exclusive sum of the kept counts over the frames (kept_ptr), what follows from it per
//   frame (cover_px, coverage_area - one fp64 division, correctly rounded - force_grid, grid_ptr), and the exclusive sum of
//   the tile counts over the call, thread t taking a contiguous share; the cursors start at the offsets.
// k_mvr_fill: one thread per slot of the records' range.  A slot below its frame's kept count is a kept record: its kp_rect,
//   mv_pt, mv_dindx row, and an entry (m, packed extent) in each tile's list at the place an integer atomic add on the tile's
//   cursor hands out - the order inside a list is free, the slots are the three minima and the maximum of a set.  A slot at or
//   behind the total writes the padding row of its own number.
// k_mvr_query: one thread per point query and per lattice rect.  It walks its tile's list, tests containment against the
//   packed extent and keeps the three smallest indices, the largest and the count in registers.  A tile of a 1080p frame with
//   8 000 records of 16 x 16 holds about four entries, so a thread per query is enough.
// Global memory is written with ordinary vector stores and the integer atomics named above.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mv_raster.h"

namespace movba {

namespace {

static_assert(MOVBA_MAX_EXPRESS_IMAGES <= kMvrKeepThreads, "k_mvr_offsets takes one frame per thread");

// Exclusive prefix sum of one value per thread over the workgroup of kMvrKeepThreads; *total = the sum.  `part` is
// kMvrKeepWaves words of LDS; every thread calls it.
__device__ inline int32_t mvr_block_scan(int32_t mine, int32_t *part, int32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();                        // (part may still be read from the call before)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int32_t at = incl - mine, all = 0;
    for (int w = 0; w < kMvrKeepWaves; ++w) {
        if (w < wave) at += part[w];
        all += part[w];
    }
    *total = all;
    return at;
}

// The chunk of the workgroup: records [r0 + c * 1024, ...) of frame f = blockIdx.y, this thread's record i of the frame, and its
// keep flag.  -> false when the frame has no chunk c (the whole workgroup).
__device__ inline bool mvr_chunk(const MvrDev &d, int32_t *f, int32_t *r0, int32_t *n, int32_t *i, bool *keep)
{
    *f = blockIdx.y; *r0 = d.rec_ptr[*f]; *n = d.rec_ptr[*f + 1] - *r0;
    if ((int32_t)blockIdx.x * kMvrKeepThreads >= *n) return false;
    *i = (int32_t)blockIdx.x * kMvrKeepThreads + (int32_t)threadIdx.x;
    *keep = *i < *n && mvr_keep(mvr_record(d, (size_t)*r0 + *i), d.cols[*f], d.rows[*f]);
    return true;
}

__global__ __launch_bounds__(kMvrKeepThreads) void k_mvr_count(const MvrDev d)
{
    __shared__ int32_t part[kMvrKeepWaves];
    int32_t f, r0, n, i;
    bool keep;
    if (!mvr_chunk(d, &f, &r0, &n, &i, &keep)) return;
    const unsigned long long votes = __ballot(keep);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = __popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t all = 0;
        for (int w = 0; w < kMvrKeepWaves; ++w) all += part[w];
        d.chunk_cnt[mvr_chunk_base(d.rec_ptr, f) + blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kMvrKeepThreads) void k_mvr_keep(const MvrDev d)
{
    __shared__ int32_t part[kMvrKeepWaves], voted[kMvrKeepWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t c = blockIdx.x;
    int32_t f, r0, n, i;
    bool keep;
    if (!mvr_chunk(d, &f, &r0, &n, &i, &keep)) {
        if (c == 0 && tid == 0) d.kept_cnt[f] = 0;      // (a frame without records; its cover arrives cleared)
        return;
    }
    // (a frame has at most 2^20 records = 1024 chunks: one earlier chunk per thread)
    int32_t carry, area;
    mvr_block_scan(tid < c ? d.chunk_cnt[mvr_chunk_base(d.rec_ptr, f) + tid] : 0, part, &carry);
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) voted[wave] = __popcll(votes);
    __syncthreads();
    int32_t before = carry, all = 0;
    for (int w = 0; w < kMvrKeepWaves; ++w) {
        if (w < wave) before += voted[w];
        all += voted[w];
    }
    int32_t mine = 0;
    if (keep) mine = mvr_keep_record(d, f, (size_t)r0 + i, before + __popcll(votes & ((1ull << lane) - 1)), [&](int32_t tile) { atomicAdd(d.tile_off + tile, 1); });
    else if (i < n) d.rec_kept[(size_t)r0 + i] = -1;
    mvr_block_scan(mine, part, &area);
    if (tid == 0) {
        atomicAdd(d.cover + f, area);
        if ((c + 1) * kMvrKeepThreads >= n) d.kept_cnt[f] = carry + all;
    }
}

__global__ __launch_bounds__(kMvrKeepThreads) void k_mvr_offsets(const MvrDev d)
{
    __shared__ int32_t part[kMvrKeepWaves];
    const int tid = threadIdx.x;
    int32_t total;
    // (n_frames <= MOVBA_MAX_EXPRESS_IMAGES = the workgroup's size: one frame per thread)
    const int32_t mine = tid < d.n_frames ? d.kept_cnt[tid] : 0, at = mvr_block_scan(mine, part, &total);
    if (tid < d.n_frames) d.kept_base[tid] = at;
    if (tid == 0) d.kept_base[d.n_frames] = total;
    __syncthreads();
    if (tid < d.n_frames) mvr_write_frame(d, tid);
    const int32_t per = (d.n_tiles + kMvrKeepThreads - 1) / kMvrKeepThreads, t0 = min(tid * per, d.n_tiles), t1 = min(t0 + per, d.n_tiles);
    int32_t sum = 0;
    for (int32_t t = t0; t < t1; ++t) sum += d.tile_off[t];
    int32_t off = mvr_block_scan(sum, part, &total);
    for (int32_t t = t0; t < t1; ++t) {
        const int32_t c = d.tile_off[t];
        d.tile_off[t] = d.tile_cur[t] = off;
        off += c;
    }
    if (tid == 0) d.tile_off[d.n_tiles] = total;
}

__global__ __launch_bounds__(kMvrThreads) void k_mvr_fill(const MvrDev d)
{
    const int32_t i = (int32_t)(blockIdx.x * kMvrThreads + threadIdx.x);
    if (i >= d.n_records) return;
    mvr_fill_slot(d, i, [&](int32_t tile) { return atomicAdd(d.tile_cur + tile, 1); });
}

__global__ __launch_bounds__(kMvrThreads) void k_mvr_query(const MvrDev d)
{
    const int32_t j = (int32_t)(blockIdx.x * kMvrThreads + threadIdx.x);
    if (j >= d.n_q + d.n_grid) return;
    mvr_query(d, j);
}

}  // namespace

hipError_t launch_mv_raster(const MvrDev &d, hipStream_t s)
{
    if (d.n_frames <= 0) return hipGetLastError();
    // (cover and tile_off are one block: mv_raster.h)
    hipError_t e = hipMemsetAsync(d.cover, 0, sizeof(int32_t) * ((size_t)d.n_frames + (size_t)d.n_tiles + 1), s);
    if (e != hipSuccess) return e;
    const dim3 chunks((unsigned)std::max(1, (d.max_records + kMvrKeepThreads - 1) / kMvrKeepThreads), (unsigned)d.n_frames);
    if (d.n_records > 0) {
        hipLaunchKernelGGL(k_mvr_count, chunks, dim3(kMvrKeepThreads), 0, s, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_mvr_keep, chunks, dim3(kMvrKeepThreads), 0, s, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_mvr_offsets, dim3(1), dim3(kMvrKeepThreads), 0, s, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (d.n_records > 0) {
        hipLaunchKernelGGL(k_mvr_fill, dim3((d.n_records + kMvrThreads - 1) / kMvrThreads), dim3(kMvrThreads), 0, s, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (d.n_q + d.n_grid > 0) {
        hipLaunchKernelGGL(k_mvr_query, dim3((d.n_q + d.n_grid + kMvrThreads - 1) / kMvrThreads), dim3(kMvrThreads), 0, s, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace movba
