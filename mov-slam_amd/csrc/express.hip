// The kernels of movba_express (include/movba.h).
//
// k_express: one wavefront per item, kExWaves items per workgroup of 256 threads, one launch over all items of the call.  The
// wave's item, its rect and its image are the same in every lane (read through the first lane), so the tests and the vote loop
// run uniformly.
//   1. the two tests that keep a rectangle from being read (ex_reject); a rejected item writes its code, zeros and -1 and ends
//   2. the centre (four pixels, every lane the same), the wrapped bounds
//   3. lane l takes the pixels l, l + 64, l + 128, l + 192 of the block (pixel (y, x) is number y * w + x): one byte load of the
//      TRUE pixel and one of the SHIFTED pixel one column to its right - x0 is arbitrary, so bytes - and one ballot each per
//      round: two 256-bit outside-masks, the same in every lane.  A lane whose number is past the block forms no address.
//   4. DESCRIBE ends the tests here.  DETECT: the precheck is a popcount of the shifted mask; lane i of the lower half builds the
//      mask of diagonal i of pass 0, lane 32 + i that of pass 1 (ex_diagonal), and counts the true mask under it; the 2 x slices
//      steps of the state machine (ex_votes) fetch these counts lane by lane, the same in every lane
//   5. the descriptor's bit order (ex_descriptor); lanes 0 .. 3 store one word each, lane 0 the code, count and distance and adds
//      a feature to its image's counter (an integer atomic on device memory)
// k_express_counts: the counters to n_features, which may lie in pinned host memory, where no atomic is sent.
// A wave reads its own item's rect, image and reference and writes its own item's results: no result depends on which others
// ran.  Global memory is written with ordinary vector stores and one integer atomic add per feature; floating point does not
// occur.
#include <hip/hip_runtime.h>

#include "express.h"

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

    // 2.
    const uint8_t *blk = d.pixels + d.img_off[im] + (size_t)y0 * cols + x0;
    const int center = ex_center(blk, cols, w, h), low = ex_low(center, d.threshold[im]), high = ex_high(center, d.threshold[im]);

    // 3.
    const int n = w * h, wl = w == 16 ? 4 : 3;
    uint64_t t[4], s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = r * 64 + lane;
        bool ot = false, os = false;
        if (p < n) {
            const uint8_t *q = blk + (size_t)(p >> wl) * cols + (p & (w - 1));
            ot = ex_outside(low, high, q[0]);
            os = ex_outside(low, high, q[1]);
        }
        t[r] = __ballot(ot);
        s[r] = __ballot(os);
    }

    // 4.
    if (d.item_mode[k] == MOVBA_EX_DESCRIBE) code = MOVBA_EX_DESCRIBED;
    else if (ex_popc256(s) < ex_precheck(w, h)) code = MOVBA_EX_REJ_FLAT;
    else {
        int my_win = 0, my_len = 0;
        if ((lane & 31) < h + w - 1) {
            uint64_t m[4];
            ex_diagonal(w, h, lane >> 5, lane & 31, m);
            my_len = ex_popc256(m);
            m[0] &= t[0]; m[1] &= t[1]; m[2] &= t[2]; m[3] &= t[3];
            my_win = ex_popc256(m);
        }
        const int pass = ex_votes(w, h, [&](int ps, int i, int *win, int *len) {
            *win = __shfl(my_win, ps * 32 + i);
            *len = __shfl(my_len, ps * 32 + i);
        });
        code = pass ? MOVBA_EX_FEATURE : MOVBA_EX_REJ_NO_EDGE;
    }

    // 5.
    const bool have = code == MOVBA_EX_FEATURE || code == MOVBA_EX_DESCRIBED;
    if (have) ex_descriptor(s, w, h, desc);
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
