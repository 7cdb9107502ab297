// One block on one wavefront: steps 2 - 5 of k_express (express.hip) as the device routines that k_express and k_adv_blocks
// (advance.hip) both call - the centre and the wrapped bounds, the two outside-masks by ballots, DETECT's precheck and diagonal
// votes by popcounts.  Every argument but `lane` is the same in every lane, the whole wave calls together, and what comes back
// is the same in every lane.  Device code only; the plain-C++ steps are express.h's.
#pragma once
#include "express.h"

namespace movba {

// Steps 2 and 3: blk = the block's first pixel (it passed ex_reject), `cols` bytes from row to row.  Lane l takes the pixels l,
// l + 64, l + 128, l + 192 of the block (pixel (y, x) is number y * w + x): one byte load of the TRUE pixel and one of the
// SHIFTED pixel one column to its right, one ballot each per round.  A lane whose number is past the block forms no address.
__device__ inline void ex_wave_masks(const uint8_t *blk, int32_t cols, int32_t w, int32_t h, int threshold, int lane, uint64_t t[4], uint64_t s[4])
{
    const int center = ex_center(blk, cols, w, h), low = ex_low(center, threshold), high = ex_high(center, threshold);
    const int n = w * h, wl = w == 16 ? 4 : 3;
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
}

// Step 4 of a DETECT item -> its code.  The precheck is a popcount of the shifted mask; lane i of the lower half builds the mask
// of diagonal i of pass 0, lane 32 + i that of pass 1 (ex_diagonal), and counts the true mask under it; the 2 x slices steps of
// the state machine (ex_votes) fetch these counts lane by lane.
__device__ inline int ex_wave_detect(const uint64_t t[4], const uint64_t s[4], int32_t w, int32_t h, int lane)
{
    if (ex_popc256(s) < ex_precheck(w, h)) return MOVBA_EX_REJ_FLAT;
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
    return pass ? MOVBA_EX_FEATURE : MOVBA_EX_REJ_NO_EDGE;
}

// Steps 2 - 5 for a block that passed ex_reject -> the code; `desc` holds the descriptor where the code has one, else zeros.
__device__ inline int ex_wave_block(const uint8_t *blk, int32_t cols, int32_t w, int32_t h, int threshold, int mode, int lane, uint64_t desc[4])
{
    uint64_t t[4], s[4];
    ex_wave_masks(blk, cols, w, h, threshold, lane, t, s);
    const int code = mode == MOVBA_EX_DESCRIBE ? MOVBA_EX_DESCRIBED : ex_wave_detect(t, s, w, h, lane);
    desc[0] = desc[1] = desc[2] = desc[3] = 0;
    if (code == MOVBA_EX_FEATURE || code == MOVBA_EX_DESCRIBED) ex_descriptor(s, w, h, desc);
    return code;
}

}  // namespace movba
