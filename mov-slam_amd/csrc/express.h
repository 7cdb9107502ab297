// Device view + launch wrapper of movba_express (express.hip; host side: express.cpp), and the steps of one item that have a
// serial meaning - the two tests that keep a rectangle from being read, the centre with its swapped offsets, the wrapped
// bounds, the diagonals, the descriptor's bit order, the vote state machine - as plain C++ (what k_express calls from its lanes,
// and what a host build runs item by item: ex_block, ex_item, ex_counts): the EXPRESS code of EXPRESS.h:79-192 as include/movba.h
// restates it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "movba.h"

namespace movba {

// Everything the kernels read and write.  Inputs lie in device memory; `features` is device scratch that arrives zeroed with the
// inputs; every out pointer is device memory or a device view of pinned host memory (the staging buffer, or the caller's
// movba_host_alloc arrays).
struct ExDev {
    int32_t n_images, n_items;
    const uint8_t *pixels;                          // the images that have items, rows tight (no stride padding)
    const int32_t *img_off, *rows, *cols, *threshold;       // n_images: image i starts at pixels + img_off[i] (0 without items)
    const int32_t *item_rect, *item_mode, *item_image;      // n_items x 4, n_items, n_items (the image of an item)
    const uint64_t *item_ref;                       // n_items x 4, or nullptr
    int32_t *features;                              // scratch: n_images, zero before k_express
    uint8_t *code;                                  // out: n_items
    uint64_t *desc;                                 // out: n_items x 4
    int32_t *count, *distance, *n_features;         // out: n_items, n_items or nullptr, n_images
};

constexpr int kExThreads = 256;
constexpr int kExWaves = kExThreads / 64;           // items of one workgroup

// k_express over all items, then k_express_counts, on the stream
hipError_t launch_express(const ExDev &d, hipStream_t s);

// ---- the steps ----

// 0 for a rectangle that is read, else the code that keeps it from being read, in the order the reference tests: its `if`
// (strict as written; the sums in 64 bits: any int32 is a coordinate), then the four shapes diagonal() knows
__host__ __device__ inline int ex_reject(int32_t x, int32_t y, int32_t w, int32_t h, int32_t rows, int32_t cols)
{
    if (!(x >= 0 && y >= 0 && (int64_t)x + w < cols && (int64_t)y + h < rows)) return MOVBA_EX_REJ_BOUNDS;
    if ((w != 8 && w != 16) || (h != 8 && h != 16)) return MOVBA_EX_REJ_SHAPE;
    return 0;
}

// compute_center: blk = the block's first pixel, `cols` bytes from row to row.  r, from the WIDTH, is the row offset and c, from
// the HEIGHT, the column offset (at<>() is handed its arguments swapped)
__host__ __device__ inline int ex_center(const uint8_t *blk, int32_t cols, int32_t w, int32_t h)
{
    const int r = w / 2, c = h / 2;
    const uint8_t *a = blk + (size_t)r * cols, *b = blk + (size_t)(r - 1) * cols;
    return ((int)a[c] + (int)b[c - 1] + (int)a[c - 1] + (int)b[c]) / 4;
}

// low_bounds / high_bounds: uint8 arithmetic, wrap-around included
__host__ __device__ inline int ex_low(int center, int threshold) { return (center - threshold) & 255; }
__host__ __device__ inline int ex_high(int center, int threshold) { return (center + threshold) & 255; }
__host__ __device__ inline bool ex_outside(int low, int high, int p) { return low > p || high < p; }

// (uint8_t)(img.rows * img.cols * .125)
__host__ __device__ inline int ex_precheck(int32_t w, int32_t h) { return ((h * w) >> 3) & 255; }
// round(slices * .25)
__host__ __device__ inline int ex_rounds(int slices) { return (slices + 2) >> 2; }

// A block's pixels as 256 bits: pixel (y, x) is bit y * w + x, bit k in bit k & 63 of word k >> 6.
__host__ __device__ inline int ex_popc(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
__host__ __device__ inline int ex_popc256(const uint64_t m[4]) { return ex_popc(m[0]) + ex_popc(m[1]) + ex_popc(m[2]) + ex_popc(m[3]); }

// diagonal i of a pass over a w x h block as such a mask: pass 0 {(y, x): x - y = i - (h - 1)}, pass 1 {(y, x): (w - 1 - x) -
// y = i - (h - 1)}
__host__ __device__ inline void ex_diagonal(int32_t w, int32_t h, int pass, int i, uint64_t m[4])
{
    m[0] = m[1] = m[2] = m[3] = 0;
    for (int y = 0; y < 16; ++y) {
        const int a = y + i - (h - 1), x = pass ? w - 1 - a : a;
        if (y >= h || a < 0 || a >= w) continue;
        const int k = y * w + x;
        const uint64_t bit = 1ull << (k & 63);
        m[0] |= (k >> 6) == 0 ? bit : 0; m[1] |= (k >> 6) == 1 ? bit : 0; m[2] |= (k >> 6) == 2 ? bit : 0; m[3] |= (k >> 6) == 3 ? bit : 0;
    }
}

// v (16 bits at the most) OR-ed into 256 bits from bit `at` on
__host__ __device__ inline void ex_or_bits(uint64_t d[4], uint64_t v, int at)
{
    const int k = at >> 6, s = at & 63;
    d[k] |= v << s;
    if (s > 48 && k < 3) d[k + 1] |= v >> (64 - s);
}

// compute_descriptor's bit order: the outside-mask of the SHIFTED pixels (bit y * w + x) to bit y * h + x - img.rows, not
// img.cols; where w = 16 and h = 8 the rows overlap and are OR-ed
__host__ __device__ inline void ex_descriptor(const uint64_t s[4], int32_t w, int32_t h, uint64_t d[4])
{
    if (w == h) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3]; return; }
    d[0] = d[1] = d[2] = d[3] = 0;
    if (w == 16) {
        for (int y = 0; y < 8; ++y) ex_or_bits(d, (s[y >> 2] >> ((y & 3) * 16)) & 0xffffull, y * 8);
    } else {
        for (int y = 0; y < 16; ++y) ex_or_bits(d, (s[y >> 3] >> ((y & 7) * 8)) & 0xffull, y * 16);
    }
}

// The diagonal votes of compute_express.  win_len(pass, i, &win, &len): the outside pixels on diagonal i of the pass and its
// length.  -> 0: neither pass succeeded, 1: pass 0 did, 2: pass 1 did (it runs only if pass 0 failed)
template <typename F> __host__ __device__ inline int ex_votes(int32_t w, int32_t h, F win_len)
{
    const int slices = h + w - 1, rounds = ex_rounds(slices), u_rounds = slices - rounds;
    for (int pass = 0; pass < 2; ++pass) {
        int wins = 0, losses = 0;
        for (int i = 0; i < slices; ++i) {
            int win, len;
            win_len(pass, i, &win, &len);
            const int loss = len - win;
            if (wins < rounds) wins = win >= loss ? wins + 1 : 0;
            if (losses < rounds) losses = loss > win ? losses + 1 : 0;
            if (i > u_rounds && (wins == 0 || losses == 0)) break;
        }
        if (wins >= rounds && losses >= rounds) return pass + 1;
    }
    return 0;
}

// what is written for an item: lane 0 of the item's wave, or the host
__host__ __device__ inline void ex_write(const ExDev &d, int32_t k, int code, const uint64_t desc[4], bool have)
{
    d.code[k] = (uint8_t)code;
    d.count[k] = have ? ex_popc256(desc) : -1;
    if (d.distance) {
        int dist = -1;
        if (have && d.item_ref) {
            const uint64_t *r = d.item_ref + 4 * (size_t)k;
            dist = ex_popc(r[0] ^ desc[0]) + ex_popc(r[1] ^ desc[1]) + ex_popc(r[2] ^ desc[2]) + ex_popc(r[3] ^ desc[3]);
        }
        d.distance[k] = dist;
    }
}

// One block that passed ex_reject on one thread, the steps in the kernel's order: blk = its first pixel, `cols` bytes from row to
// row.  -> the code, the descriptor where the code has one (else zeros), *pass = the pass that succeeded (ex_votes) or 0
inline int ex_block(const uint8_t *blk, int32_t cols, int32_t w, int32_t h, int threshold, int mode, uint64_t desc[4], int *pass)
{
    const int center = ex_center(blk, cols, w, h), low = ex_low(center, threshold), high = ex_high(center, threshold);
    uint64_t t[4] = { 0, 0, 0, 0 }, s[4] = { 0, 0, 0, 0 };
    int code;
    desc[0] = desc[1] = desc[2] = desc[3] = 0;
    *pass = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int p = y * w + x;
            if (ex_outside(low, high, blk[(size_t)y * cols + x])) t[p >> 6] |= 1ull << (p & 63);
            if (ex_outside(low, high, blk[(size_t)y * cols + x + 1])) s[p >> 6] |= 1ull << (p & 63);
        }
    if (mode == MOVBA_EX_DESCRIBE) code = MOVBA_EX_DESCRIBED;
    else if (ex_popc256(s) < ex_precheck(w, h)) code = MOVBA_EX_REJ_FLAT;
    else {
        *pass = ex_votes(w, h, [&](int ps, int i, int *win, int *len) {
            uint64_t m[4];
            ex_diagonal(w, h, ps, i, m);
            *len = ex_popc256(m);
            m[0] &= t[0]; m[1] &= t[1]; m[2] &= t[2]; m[3] &= t[3];
            *win = ex_popc256(m);
        });
        code = *pass ? MOVBA_EX_FEATURE : MOVBA_EX_REJ_NO_EDGE;
    }
    if (code == MOVBA_EX_FEATURE || code == MOVBA_EX_DESCRIBED) ex_descriptor(s, w, h, desc);
    return code;
}

// One item on one thread.  -> the pass that succeeded (ex_votes) for a feature, else 0
inline int ex_item(const ExDev &d, int32_t k)
{
    const int32_t x0 = d.item_rect[4 * (size_t)k], y0 = d.item_rect[4 * (size_t)k + 1], w = d.item_rect[4 * (size_t)k + 2], h = d.item_rect[4 * (size_t)k + 3];
    const int32_t im = d.item_image[k], cols = d.cols[im];
    uint64_t desc[4] = { 0, 0, 0, 0 };
    uint64_t *out = d.desc + 4 * (size_t)k;
    int code = ex_reject(x0, y0, w, h, d.rows[im], cols), pass = 0;
    if (!code) code = ex_block(d.pixels + d.img_off[im] + (size_t)y0 * cols + x0, cols, w, h, d.threshold[im], d.item_mode[k], desc, &pass);
    const bool have = code == MOVBA_EX_FEATURE || code == MOVBA_EX_DESCRIBED;
    out[0] = desc[0]; out[1] = desc[1]; out[2] = desc[2]; out[3] = desc[3];
    ex_write(d, k, code, desc, have);
    if (code == MOVBA_EX_FEATURE) d.features[im] += 1;
    return pass;
}

// the second pass on one thread
inline void ex_counts(const ExDev &d)
{
    for (int32_t i = 0; i < d.n_images; ++i) d.n_features[i] = d.features[i];
}

}  // namespace movba
