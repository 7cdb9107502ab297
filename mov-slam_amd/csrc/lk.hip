// The kernels of movba_lk_track (include/movba.h): the clearing of the frames' kept counts and up to five launches on one stream.
//
// k_lk_pyr: one launch per level 1 .. 3 that some frame uses.  A thread per output pixel of that level, for both images of every
//   frame: it finds its frame in the level's prefix over the frames (at most ten steps) and writes lk_pyr_pixel of the level
//   below.  A level is complete before the next launch reads it.
// k_lk_track: a wavefront per point, four per workgroup.  The wavefront walks lk_point (lk.h) together, levels top-down inside
//   the kernel: lane t owns the window entries t, t + 64, ... (at most 16: 31 x 31 = 961), keeps their I, Ix, Iy as int16 in
//   registers across the iterations of a level, and the five sums - a11, a12, a22 once per level, b1, b2 per iteration - are
//   int32 per lane and int64 through a butterfly over the wavefront, which leaves the total in every lane.  Every lane then
//   runs the same fp32 tail on the same values, so every branch of the walk is uniform and lane 0 writes the point.  The Scharr
//   pair is formed from the 4 x 4 neighbourhood of an entry as it is read: no derivative image is stored.  Pixels are read from
//   global memory through the caches: the window of a level is at most 34 x 34 bytes of each image, which the lanes of the
//   wavefront re-read from L1 for every iteration (DESIGN.md 4l has the reasoning and the times).  The point's keep flag is one
//   integer atomic add on its frame's count: scheduling cannot change the sum.
// k_lk_keep: a workgroup of 1024 threads per frame, and one more per 1024 points for the padding.  Each sums the frames'
//   counts before its own (at most 1024, one per thread) - kept_ptr - and walks its frame's keep flags in chunks of 1024 with a
//   running count: kept_src in input order.  The padding workgroups write -1 behind the total.
// Global memory is written with ordinary vector stores and the integer atomic named above.
#include <hip/hip_runtime.h>

#include "lk.h"

namespace movba {

namespace {

static_assert(MOVBA_MAX_EXPRESS_IMAGES <= kLkKeepThreads, "k_lk_keep takes one frame per thread");
static_assert(kLkThreads == 64 * kLkTrackWaves, "k_lk_track: four wavefronts per workgroup");

struct LkWave {
    static constexpr int kEntries = kLkWaveEntries, kStride = 64, kUnroll = kLkWaveEntries;
    typedef int32_t Acc;
    int first;
    __device__ int64_t sum(int64_t v) const
    {
        for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o);
        return v;
    }
};

__global__ __launch_bounds__(kLkThreads) void k_lk_pyr(const LkDev d, const int32_t level)
{
    const int64_t j = (int64_t)blockIdx.x * kLkThreads + threadIdx.x;
    if (j >= 2 * (int64_t)d.level_pixels[level - 1]) return;
    lk_pyr_item(d, level, (int32_t)j);
}

__global__ __launch_bounds__(kLkThreads) void k_lk_track(const LkDev d)
{
    const int lane = threadIdx.x & 63;
    const int64_t at = (int64_t)blockIdx.x * kLkTrackWaves + (threadIdx.x >> 6);
    if (at >= d.n_pt) return;                       // (the whole wavefront)
    const int32_t i = (int32_t)at, f = lk_frame_of(d.pt_ptr, d.n_frames, i);
    const LkFrame &fr = d.frame[f];
    const LkPoint p = lk_point(d, fr, d.pt[2 * (size_t)i], d.pt[2 * (size_t)i + 1], LkWave{ lane });
    if (lane != 0) return;
    const bool keep = lk_keep(p, fr.rows[0], fr.cols[0]);
    lk_write_point(d, i, p, keep);
    if (keep) atomicAdd(d.kept_cnt + f, 1);
}

// Exclusive prefix sum of one value per thread over the workgroup of kLkKeepThreads; *total = the sum.  `part` is kLkKeepWaves
// words of LDS; every thread calls it.
__device__ inline int32_t lk_block_scan(int32_t mine, int32_t *part, int32_t *total)
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
    for (int w = 0; w < kLkKeepWaves; ++w) {
        if (w < wave) at += part[w];
        all += part[w];
    }
    *total = all;
    return at;
}

__global__ __launch_bounds__(kLkKeepThreads) void k_lk_keep(const LkDev d)
{
    __shared__ int32_t part[kLkKeepWaves], base_of;
    const int tid = threadIdx.x;
    const int32_t b = blockIdx.x;
    int32_t total;
    // (n_frames <= MOVBA_MAX_EXPRESS_IMAGES = the workgroup's size: one frame per thread)
    const int32_t before = lk_block_scan(tid < d.n_frames ? d.kept_cnt[tid] : 0, part, &total);
    if (b >= d.n_frames) {                  // the padding behind the total
        const int64_t i = (int64_t)(b - d.n_frames) * kLkKeepThreads + tid;
        if (i >= total && i < d.n_pt) d.kept_src[i] = -1;
        return;
    }
    if (tid == b) base_of = before;
    __syncthreads();
    const int32_t base = base_of, p0 = d.pt_ptr[b], n = d.pt_ptr[b + 1] - p0;
    if (tid == 0) {
        d.kept_ptr[b] = base;
        if (b == d.n_frames - 1) d.kept_ptr[d.n_frames] = total;
    }
    int32_t run = 0;
    for (int32_t c = 0; c < n; c += kLkKeepThreads) {
        const int32_t i = c + tid;
        const bool keep = i < n && d.keep[(size_t)p0 + i] != 0;
        int32_t chunk;
        const int32_t rank = lk_block_scan(keep ? 1 : 0, part, &chunk);
        if (keep) d.kept_src[(size_t)base + run + rank] = i;
        run += chunk;
    }
}

}  // namespace

hipError_t launch_lk(const LkDev &d, hipStream_t s)
{
    if (d.n_frames <= 0) return hipGetLastError();
    hipError_t e = hipMemsetAsync(d.kept_cnt, 0, sizeof(int32_t) * (size_t)d.n_frames, s);
    if (e != hipSuccess) return e;
    if (d.n_pt > 0) {
        for (int32_t l = 1; l < kLkLevels; ++l) {
            const int64_t items = 2 * (int64_t)d.level_pixels[l - 1];
            if (items == 0) break;
            hipLaunchKernelGGL(k_lk_pyr, dim3((unsigned)((items + kLkThreads - 1) / kLkThreads)), dim3(kLkThreads), 0, s, d, l);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_lk_track, dim3((unsigned)((d.n_pt + kLkTrackWaves - 1) / kLkTrackWaves)), dim3(kLkThreads), 0, s, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const unsigned pad_groups = (unsigned)((d.n_pt + kLkKeepThreads - 1) / kLkKeepThreads);
    hipLaunchKernelGGL(k_lk_keep, dim3((unsigned)d.n_frames + pad_groups), dim3(kLkKeepThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
