// The kernels of movba_advance (include/movba.h), four launches on one stream.
//
// k_adv_sort: one workgroup of 1024 threads per frame.  The keys (adv_key: age, popcount, input index - distinct, so the method
//   cannot change the outcome) go into LDS, padded with all-ones to a power of two, and a bitonic network sorts them ascending;
//   `order` (to the caller and to scratch) and each feature's position come out.  LDS: 8 bytes x pow2ceil(the call's largest frame), 128 KiB at the bound.
// k_adv_blocks: one wavefront per wave item, 4 per workgroup, over the previous features, macroblocks and lattice rects of all
//   frames (adv_item).  The item, its frame and its rects are the same in every lane, so the tests and loops run uniformly; the
//   per-block routine is the one k_express calls (express_wave.h).  Lane 0 writes.  A previous feature that arrives claims its
//   macroblock with an integer atomic minimum of its position on a word of device scratch that arrives as kAdvNoClaim: a
//   minimum, so the outcome does not depend on which wave comes first.  DETECT of a macroblock or a lattice rect does not
//   depend on the claims - only whether it is emitted does - so the three kinds run side by side.
// k_adv_resolve: one workgroup per frame.  Fates (adv_settle), kp_found and kp_code (adv_write_kp), then three exclusive
//   prefix sums - kept features over the positions, new features over the macroblocks, and, once mov_cnt is known, grid
//   features over the lattice - leave each wave item's place in its segment (it_rank), and the frame's counts, mov_cnt,
//   grid_ran and next_id.  The lattice is always computed and only emitted when the gate says so.
// k_adv_emit: up to 64 workgroups per frame.  The frame's start in the dense list is the sum of the earlier frames' counts (at most
//   1024 x 3 words, which every workgroup adds up itself); seg_ptr, the rows of a share of the frame's items (adv_emit_item) and
//   a share of the padding behind the total.
// Global memory is written with ordinary vector stores and the one integer atomic; the only floating-point operations are the
// add and the subtract of adv_add / adv_corner.
#include <hip/hip_runtime.h>

#include "advance.h"
#include "express_wave.h"

namespace movba {

namespace {

__global__ __launch_bounds__(kAdvSortThreads) void k_adv_sort(const AdvDev d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char adv_lds[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(adv_lds);
    const int tid = threadIdx.x;
    const int32_t f = blockIdx.x, p0 = d.prev_ptr[f], n = d.prev_ptr[f + 1] - p0, m = adv_pow2ceil(n);
    if (n <= 0) return;                     // (the whole workgroup)
    for (int32_t i = tid; i < m; i += kAdvSortThreads)
        keys[i] = i < n ? adv_key(d.prev_age[p0 + i], ex_popc256(d.prev_desc + 4 * (size_t)(p0 + i)), i) : ~0ull;
    __syncthreads();
    for (int32_t k = 2; k <= m; k <<= 1) {
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t t = tid; t < (m >> 1); t += kAdvSortThreads) {
                const int32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const uint64_t ka = keys[a], kb = keys[b];
                if ((ka > kb) == ((a & k) == 0)) { keys[a] = kb; keys[b] = ka; }
            }
            __syncthreads();
        }
    }
    for (int32_t i = tid; i < n; i += kAdvSortThreads) {
        const int32_t idx = adv_key_index(keys[i]);
        d.order[p0 + i] = idx;
        d.ord[p0 + i] = idx;
        d.pos[p0 + idx] = i;
    }
}

__global__ __launch_bounds__(kAdvThreads) void k_adv_blocks(const AdvDev d)
{
    const int lane = threadIdx.x & 63;
    const int32_t k = __builtin_amdgcn_readfirstlane((int32_t)(blockIdx.x * kAdvWaves + (threadIdx.x >> 6)));
    if (k >= d.n_items) return;             // (the whole wave; there is no barrier in this kernel)
    adv_item(d, k, lane == 0, [&](int32_t f, int32_t x, int32_t y, int32_t w, int32_t h, int mode, uint64_t desc[4]) {
        const int32_t cols = d.cols[f];
        const int code = ex_reject(x, y, w, h, d.rows[f], cols);
        if (code) { desc[0] = desc[1] = desc[2] = desc[3] = 0; return code; }
        return ex_wave_block(d.pixels + d.img_off[f] + (size_t)y * cols + x, cols, w, h, d.threshold[f], mode, lane, desc);
    });
}

// Exclusive prefix sum of a flag over 0 .. n - 1 by the workgroup: thread t takes the contiguous chunk [t * per, (t + 1) * per),
// so places ascend with the index.  place(i, r) is called with r = the number of flagged indices below i for a flagged i and
// with -1 otherwise.  -> the number of flagged indices.  Every thread calls it; `part` is kAdvWaves + 1 words of LDS.
template <typename Flag, typename Place> __device__ inline int32_t adv_scan(int32_t n, int32_t *part, Flag flag, Place place)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t per = (n + kAdvThreads - 1) / kAdvThreads, i0 = min(tid * per, n), i1 = min(i0 + per, n);
    int32_t mine = 0;
    for (int32_t i = i0; i < i1; ++i) mine += flag(i) ? 1 : 0;
    int32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();                        // (part may still be read from the scan before)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int32_t at = incl - mine, total = 0;
    for (int w = 0; w < kAdvWaves; ++w) {
        if (w < wave) at += part[w];
        total += part[w];
    }
    for (int32_t i = i0; i < i1; ++i) place(i, flag(i) ? at++ : -1);
    return total;
}

__global__ __launch_bounds__(kAdvThreads) void k_adv_resolve(const AdvDev d)
{
    __shared__ int32_t part[kAdvWaves + 1];
    const int tid = threadIdx.x;
    const int32_t f = blockIdx.x, p0 = d.prev_ptr[f], np = d.prev_ptr[f + 1] - p0, nk = d.kp_ptr[f + 1] - d.kp_ptr[f], ng = d.g_ptr[f + 1] - d.g_ptr[f];
    const int32_t base = adv_item_base(d, f);
    for (int32_t i = tid; i < np; i += kAdvThreads) adv_settle(d, f, (size_t)p0 + i);
    __syncthreads();
    const int32_t kept = adv_scan(np, part, [&](int32_t i) { return d.it_code[base + d.ord[p0 + i]] == MOVBA_ADV_KEPT; },
                                  [&](int32_t i, int32_t r) { d.it_rank[base + d.ord[p0 + i]] = r; });
    const int32_t fresh = adv_scan(nk, part, [&](int32_t m) { return adv_kp_new(d, f, m); },
                                   [&](int32_t m, int32_t r) { adv_write_kp(d, f, m); d.it_rank[base + np + m] = r; });
    const bool runs = adv_grid_runs(d.force_grid[f], fresh);
    const int32_t grid = adv_scan(ng, part, [&](int32_t g) { return runs && adv_grid_feature(d, f, g); },
                                  [&](int32_t g, int32_t r) { d.it_rank[base + np + nk + g] = r; });
    if (tid == 0) adv_write_counts(d, f, kept, fresh, grid);
}

__global__ __launch_bounds__(kAdvThreads) void k_adv_emit(const AdvDev d)
{
    __shared__ int32_t sums[2][kAdvWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t f = blockIdx.x;
    int32_t before = 0, all = 0;
    for (int32_t i = tid; i < 3 * d.n_frames; i += kAdvThreads) {
        const int32_t c = d.counts[i];
        all += c;
        if (i < 3 * f) before += c;
    }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
    if (lane == 0) { sums[0][wave] = before; sums[1][wave] = all; }
    __syncthreads();
    before = all = 0;
    for (int w = 0; w < kAdvWaves; ++w) { before += sums[0][w]; all += sums[1][w]; }
    const int32_t chunk = blockIdx.y, n_chunks = gridDim.y;
    if (tid == 0 && chunk == 0) adv_write_segments(d, f, before, all);
    for (int32_t k = adv_item_base(d, f) + chunk * kAdvThreads + tid; k < adv_item_base(d, f + 1); k += n_chunks * kAdvThreads) adv_emit_item(d, f, k, before);
    const int64_t group = (int64_t)f * n_chunks + chunk, groups = (int64_t)d.n_frames * n_chunks;
    for (int64_t o = (int64_t)all + group * kAdvThreads + tid; o < d.n_items; o += groups * kAdvThreads) adv_pad(d, (size_t)o);
}

}  // namespace

hipError_t launch_advance(const AdvDev &d, hipStream_t s)
{
    if (d.n_frames <= 0) return hipGetLastError();
    if (d.max_prev > 0) {
        const size_t lds = 8 * (size_t)adv_pow2ceil(d.max_prev);
        // (above the 64 KB a kernel may ask for unannounced; per device, so said where it is needed rather than once per process)
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_adv_sort), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * MOVBA_MAX_ADVANCE_PREV);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_adv_sort, dim3(d.n_frames), dim3(kAdvSortThreads), lds, s, d);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (d.n_items > 0) {
        hipLaunchKernelGGL(k_adv_blocks, dim3((d.n_items + kAdvWaves - 1) / kAdvWaves), dim3(kAdvThreads), 0, s, d);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_adv_resolve, dim3(d.n_frames), dim3(kAdvThreads), 0, s, d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (workgroups per frame: by the average frame, so that a call of one frame is not one workgroup's work)
    const int chunks = std::min(kAdvEmitChunks, std::max(1, (d.n_items / d.n_frames + kAdvThreads - 1) / kAdvThreads));
    hipLaunchKernelGGL(k_adv_emit, dim3(d.n_frames, chunks), dim3(kAdvThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
