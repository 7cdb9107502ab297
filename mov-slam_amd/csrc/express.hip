// The kernels of movba_express (include/movba.h).
//
// k_express: one wavefront per item, kExWaves items per workgroup of 256 threads, one launch over all items of the call.  The
// wave's item, its rect and its image are the same in every lane (read through the first lane), so the tests and the vote loop
// run uniformly.
//   1. the two tests that keep a rectangle from being read (ex_reject); a rejected item writes its code, zeros and -1 and ends
//   2. - 5. ex_wave_block (express_wave.h, the routine k_adv_blocks of advance.hip calls too): the centre and the wrapped bounds;
//      the two 256-bit outside-masks of the TRUE and the SHIFTED pixels by ballots, lane l taking the pixels l, l + 64, l + 128,
//      l + 192 of the block; DESCRIBE ends the tests there, DETECT goes on to the precheck (a popcount) and the diagonal votes
//      (popcounts under the diagonals' masks, fetched lane by lane by the state machine ex_votes); the descriptor's bit order
//      (ex_descriptor)
//   6. lanes 0 .. 3 store one word each, lane 0 the code, count and distance and adds a feature to its image's counter (an
//      integer atomic on device memory)
// k_express_counts: the counters to n_features, which may lie in pinned host memory, where no atomic is sent.
// A wave reads its own item's rect, image and reference and writes its own item's results: no result depends on which others
// ran.  Global memory is written with ordinary vector stores and one integer atomic add per feature; floating point does not
// occur.
#include <hip/hip_runtime.h>

#include "express.h"
#include "express_wave.h"

namespace movba {

namespace {

__global__ __launch_bounds__(kExThreads) void k_express(const ExDev d)
{
    const int lane = threadIdx.x & 63;
    const int32_t k = __builtin_amdgcn_readfirstlane((int32_t)(blockIdx.x * kExWaves + (threadIdx.x >> 6)));
    if (k >= d.n_items) return;             // (the whole wave; there is no barrier in this kernel)

    const int32_t x0 = d.item_rect[4 * (size_t)k], y0 = d.item_rect[4 * (size_t)k + 1], w = d.item_rect[4 * (size_t)k + 2], h = d.item_rect[4 * (size_t)k + 3];
    const int32_t im = d.item_image[k], cols = d.cols[im];
    uint64_t desc[4] = { 0, 0, 0, 0 };
    uint64_t *out = d.desc + 4 * (size_t)k;

    // 1.
    int code = ex_reject(x0, y0, w, h, d.rows[im], cols);
    if (code) {
        if (lane < 4) out[lane] = 0;
        if (lane == 0) ex_write(d, k, code, desc, false);
        return;
    }

    // 2. - 5.  (express_wave.h: the routine k_adv_blocks calls too)
    code = ex_wave_block(d.pixels + d.img_off[im] + (size_t)y0 * cols + x0, cols, w, h, d.threshold[im], d.item_mode[k], lane, desc);
    const bool have = code == MOVBA_EX_FEATURE || code == MOVBA_EX_DESCRIBED;
    if (lane < 4) out[lane] = lane == 0 ? desc[0] : lane == 1 ? desc[1] : lane == 2 ? desc[2] : desc[3];
    if (lane == 0) {
        ex_write(d, k, code, desc, have);
        if (code == MOVBA_EX_FEATURE) atomicAdd(d.features + im, 1);
    }
}

__global__ __launch_bounds__(kExThreads) void k_express_counts(const ExDev d)
{
    const int32_t i = blockIdx.x * kExThreads + threadIdx.x;
    if (i < d.n_images) d.n_features[i] = d.features[i];
}

}  // namespace

hipError_t launch_express(const ExDev &d, hipStream_t s)
{
    if (d.n_items <= 0 || d.n_images <= 0) return hipGetLastError();
    hipLaunchKernelGGL(k_express, dim3((d.n_items + kExWaves - 1) / kExWaves), dim3(kExThreads), 0, s, d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_express_counts, dim3((d.n_images + kExThreads - 1) / kExThreads), dim3(kExThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
