// Device view + launch wrapper of movba_lk_track (lk.hip; host side: lk.cpp), and the steps of sparse pyramidal Lucas-Kanade that
// have a serial meaning - the pyramid's pixel, the reflected read, the Scharr pair, the bilinear weights, a window entry, the
// matrix test, the iteration with its three exits, the keep gate - as plain C++: what the kernels call, and what a host build
// runs point by point (lk_frames), as mv_raster.h does with mvr_frames.  cv::calcOpticalFlowPyrLK as include/movba.h restates it
// [opencv-upstream].  This file is the single statement of the arithmetic: lk_point is ONE body, walked by one thread on the
// host (LkSerial: every window entry, sums passed through) and by the 64 lanes of a wavefront on the device (LkWave in lk.hip:
// entry lane, lane + 64, ..., sums through an integer wave reduction).  The five sums are integers, so their order is free; the
// fp32 tail is the same statements on both sides, one operation per statement, and contraction is off for all of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "movba.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace movba {

constexpr int kLkLevels = 4;                        // levels 0 .. 3
constexpr int kLkMaxWin = 31;
constexpr int kLkWaveEntries = (kLkMaxWin * kLkMaxWin + 63) / 64;      // 16: the window entries of one lane
constexpr int kLkTrackWaves = 4;                    // k_lk_track: a wavefront per point, four per workgroup
constexpr int kLkThreads = 256;                     // k_lk_pyr, k_lk_track
constexpr int kLkKeepThreads = 1024;                // k_lk_keep
constexpr int kLkKeepWaves = kLkKeepThreads / 64;

// One frame's pyramids.  Level l of image i (0: prev, 1: next) is rows[l] x cols[l] bytes, tightly packed, at pix + off[i][l];
// levels above `levels` have no pixels.  Filled by lk_frame_levels and the host's layout.
struct LkFrame {
    int64_t off[2][kLkLevels];
    int32_t rows[kLkLevels], cols[kLkLevels];
    int32_t levels, win;                            // levels: L of the header, the top level that is used
};

// Everything the kernels read and write.  Inputs and scratch lie in device memory; kept_cnt arrives cleared; every out pointer
// is device memory or a device view of pinned host memory.
struct LkDev {
    int32_t n_frames, n_pt, max_iter;
    int32_t level_pixels[kLkLevels - 1];            // the pixels of level 1, 2, 3 of ONE image over the call: lvl_ptr's last entries
    double eps_sq, min_eig;                         // eps * eps in fp64, as TermCriteria's epsilon is squared; the threshold
    const LkFrame *frame;                           // n_frames
    const int32_t *pt_ptr;                          // n_frames + 1
    const int32_t *lvl_ptr;                         // 3 x (n_frames + 1): the pixels of level l + 1 of ONE image, prefix over the frames
    const float *pt;                                // n_pt x 2
    uint8_t *pix;                                   // what LkFrame::off counts from: level 0 arrives, levels 1 .. 3 are built
    int32_t *kept_cnt;                              // n_frames: the frame's points with keep != 0
    // out
    float *next_pt, *err;
    uint8_t *pt_status, *exit_code, *keep;
    int32_t *kept_ptr, *kept_src;
};

// the clearing of kept_cnt, then k_lk_pyr per level, k_lk_track and k_lk_keep on the stream
hipError_t launch_lk(const LkDev &d, hipStream_t s);

// ---- the steps ----

// rows, cols and L of a frame's pyramid: level l + 1 is ((w + 1) / 2, (h + 1) / 2), and the top level is the largest L <= max_level
// such that every level 1 .. L has both sides > win
__host__ __device__ inline void lk_frame_levels(int32_t rows, int32_t cols, int32_t win, int32_t max_level, LkFrame *fr)
{
    for (int l = 0; l < kLkLevels; ++l) fr->rows[l] = fr->cols[l] = 0;
    fr->rows[0] = rows; fr->cols[0] = cols; fr->levels = 0; fr->win = win;
    for (int l = 1; l <= max_level && l < kLkLevels; ++l) {
        const int32_t r = (fr->rows[l - 1] + 1) / 2, c = (fr->cols[l - 1] + 1) / 2;
        if (r <= win || c <= win) break;
        fr->rows[l] = r; fr->cols[l] = c; fr->levels = l;
    }
}

// BORDER_REFLECT_101 with one reflection, which is all the rules ever ask for (sides > win, reads at most win + 1 outside).  The
// clamp behind it is never the result for an index whose pixel takes part in a result: it keeps the neighbourhood of a corner
// OUTSIDE the image - whose derivative is the constant 0 - inside the buffer.
__host__ __device__ inline int32_t lk_reflect(int32_t i, int32_t n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// pyrDown's pixel (x, y) of the level above `src` (sr x sc): [1 4 6 4 1] in both directions around (2x, 2y), all integer
__host__ __device__ inline uint8_t lk_pyr_pixel(const uint8_t *src, int32_t sr, int32_t sc, int32_t x, int32_t y)
{
    const int32_t k[5] = { 1, 4, 6, 4, 1 };
    int32_t sum = 0;
    for (int j = 0; j < 5; ++j) {
        const uint8_t *row = src + (size_t)lk_reflect(2 * y + j - 2, sr) * sc;
        int32_t line = 0;
        for (int i = 0; i < 5; ++i) line += k[i] * row[lk_reflect(2 * x + i - 2, sc)];
        sum += k[j] * line;
    }
    return (uint8_t)((sum + 128) >> 8);
}

__host__ __device__ inline int32_t lk_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// floor(p) must satisfy -win <= . < side on both axes, tested on the floats (a float beyond the integers fails it like any other)
__host__ __device__ inline bool lk_inside(float fx, float fy, int32_t win, int32_t cols, int32_t rows)
{
    return fx >= (float)-win && fx < (float)cols && fy >= (float)-win && fy < (float)rows;
}

struct LkWeights { int32_t w00, w01, w10, w11; };
// a, b: the fractions of the window's corner; rint is to nearest, ties to even
__host__ __device__ inline LkWeights lk_weights(float a, float b)
{
    const float one_a = 1.f - a, one_b = 1.f - b;
    const float f00 = one_a * one_b, f01 = a * one_b, f10 = one_a * b;
    const float s00 = f00 * 16384.f, s01 = f01 * 16384.f, s10 = f10 * 16384.f;
    LkWeights w;
    w.w00 = (int32_t)rintf(s00); w.w01 = (int32_t)rintf(s01); w.w10 = (int32_t)rintf(s10);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

// J at the bilinear cell whose corner is (x, y): REFLECT_101 pixels, descaled to 5 fractional bits
__host__ __device__ inline int32_t lk_pixel(const uint8_t *img, int32_t rows, int32_t cols, int32_t x, int32_t y, const LkWeights &w)
{
    const uint8_t *r0 = img + (size_t)lk_reflect(y, rows) * cols, *r1 = img + (size_t)lk_reflect(y + 1, rows) * cols;
    const int32_t x0 = lk_reflect(x, cols), x1 = lk_reflect(x + 1, cols);
    return lk_descale(r0[x0] * w.w00 + r0[x1] * w.w01 + r1[x0] * w.w10 + r1[x1] * w.w11, 9);
}

struct LkTaps { int32_t I, Ix, Iy; };
// I, Ix, Iy at the same cell of the previous image.  q is the 4 x 4 neighbourhood around the cell; a corner inside the image has
// the unscaled Scharr pair over REFLECT_101 neighbours, a corner outside has 0 - the constant border of the derivative buffer.
__host__ __device__ inline LkTaps lk_patch(const uint8_t *img, int32_t rows, int32_t cols, int32_t x, int32_t y, const LkWeights &w)
{
    int32_t q[4][4];
    for (int j = 0; j < 4; ++j) {
        const uint8_t *row = img + (size_t)lk_reflect(y - 1 + j, rows) * cols;
        for (int i = 0; i < 4; ++i) q[j][i] = row[lk_reflect(x - 1 + i, cols)];
    }
    const int32_t wt[2][2] = { { w.w00, w.w01 }, { w.w10, w.w11 } };
    int32_t sx = 0, sy = 0;
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 2; ++cx) {
            const int32_t px = x + cx, py = y + cy;
            if (px < 0 || px >= cols || py < 0 || py >= rows) continue;
            const int j = cy + 1, i = cx + 1;
            const int32_t dx = 3 * (q[j - 1][i + 1] - q[j - 1][i - 1]) + 10 * (q[j][i + 1] - q[j][i - 1]) + 3 * (q[j + 1][i + 1] - q[j + 1][i - 1]);
            const int32_t dy = 3 * (q[j + 1][i - 1] - q[j - 1][i - 1]) + 10 * (q[j + 1][i] - q[j - 1][i]) + 3 * (q[j + 1][i + 1] - q[j - 1][i + 1]);
            sx += dx * wt[cy][cx]; sy += dy * wt[cy][cx];
        }
    LkTaps t;
    t.I = lk_descale(q[1][1] * w.w00 + q[1][2] * w.w01 + q[2][1] * w.w10 + q[2][2] * w.w11, 9);
    t.Ix = lk_descale(sx, 14); t.Iy = lk_descale(sy, 14);
    return t;
}

// an exact integer sum (below 2^36 in magnitude) as the fp32 the matrix takes: converted ONCE, times 2^-20
__host__ __device__ inline float lk_scaled(int64_t s) { return (float)((double)s * (1.0 / 1048576.0)); }

struct LkMatrix { float A11, A12, A22, D, min_eig; };
__host__ __device__ inline LkMatrix lk_matrix(int64_t a11, int64_t a12, int64_t a22, int32_t win)
{
    LkMatrix m;
    m.A11 = lk_scaled(a11); m.A12 = lk_scaled(a12); m.A22 = lk_scaled(a22);
    const float p = m.A11 * m.A22, q = m.A12 * m.A12;
    m.D = p - q;
    const float diff = m.A11 - m.A22, diff2 = diff * diff, four = 4.f * q, rad = diff2 + four, root = sqrtf(rad);
    const float trace = m.A22 + m.A11, num = trace - root, den = (float)(2 * win * win);
    m.min_eig = num / den;
    return m;
}

struct LkPoint { float x, y, err; uint8_t status, exit_code; };

// how the window is walked: the host takes every entry itself ...
struct LkSerial {
    static constexpr int kEntries = kLkMaxWin * kLkMaxWin, kStride = 1, kUnroll = 1;
    typedef int64_t Acc;
    int first = 0;
    __host__ __device__ int64_t sum(int64_t v) const { return v; }
};
// ... and LkWave (lk.hip) gives lane `first` the entries first, first + 64, ...: at most 16 of them, whose partial sums fit int32

// One point of frame `fr`, levels L .. 0.  Every lane of a wavefront that walks it together ends with the same LkPoint.
template <typename Ex> __host__ __device__ inline LkPoint lk_point(const LkDev &d, const LkFrame &fr, float ptx, float pty, const Ex &ex)
{
    const int32_t win = fr.win, n = win * win;
    const float half = (float)(win - 1) * 0.5f;
    LkPoint out{ 0.f, 0.f, 0.f, 1, 0 };
    int16_t pI[Ex::kEntries], pIx[Ex::kEntries], pIy[Ex::kEntries], pos[Ex::kEntries];     // pos: y * 32 + x of the entry
#pragma unroll Ex::kUnroll
    for (int t = 0; t < Ex::kEntries; ++t) {
        const int32_t k = ex.first + t * Ex::kStride, y = k < n ? k / win : 0;
        pos[t] = (int16_t)(k < n ? y * 32 + (k - y * win) : -1);
    }
    float nx = 0.f, ny = 0.f;                       // nextPts[ptidx], as stored
    for (int32_t l = fr.levels; l >= 0; --l) {
        const int32_t cols = fr.cols[l], rows = fr.rows[l];
        const uint8_t *I = d.pix + fr.off[0][l], *J = d.pix + fr.off[1][l];
        const float scale = 1.f / (float)(1 << l);
        const float qx = ptx * scale, qy = pty * scale;
        if (l == fr.levels) { nx = qx; ny = qy; }
        else { nx = nx * 2.f; ny = ny * 2.f; }
        const float ux = qx - half, uy = qy - half, fx = floorf(ux), fy = floorf(uy);
        if (!lk_inside(fx, fy, win, cols, rows)) {
            if (l == 0) { out.status = 0; out.err = 0.f; out.exit_code = MOVBA_LK_REJ_START; }
            continue;
        }
        const int32_t ix = (int32_t)fx, iy = (int32_t)fy;
        const float a = ux - fx, b = uy - fy;
        const LkWeights w = lk_weights(a, b);
        typename Ex::Acc a11 = 0, a12 = 0, a22 = 0;
#pragma unroll Ex::kUnroll
        for (int t = 0; t < Ex::kEntries; ++t) {
            if (pos[t] < 0) continue;
            const LkTaps e = lk_patch(I, rows, cols, ix + (pos[t] & 31), iy + (pos[t] >> 5), w);
            pI[t] = (int16_t)e.I; pIx[t] = (int16_t)e.Ix; pIy[t] = (int16_t)e.Iy;
            a11 += e.Ix * e.Ix; a12 += e.Ix * e.Iy; a22 += e.Iy * e.Iy;
        }
        const LkMatrix m = lk_matrix(ex.sum(a11), ex.sum(a12), ex.sum(a22), win);
        out.err = m.min_eig;
        if ((double)m.min_eig < d.min_eig || m.D < FLT_EPSILON) {
            if (l == 0) { out.status = 0; out.exit_code = MOVBA_LK_REJ_MIN_EIG; }
            continue;
        }
        const float D = 1.f / m.D;
        float cx = nx - half, cy = ny - half, prev_dx = 0.f, prev_dy = 0.f;
        uint8_t why = MOVBA_LK_MAX_ITER_RAN;
        for (int32_t j = 0; j < d.max_iter; ++j) {
            const float gx = floorf(cx), gy = floorf(cy);
            if (!lk_inside(gx, gy, win, cols, rows)) {
                if (l == 0) out.status = 0;
                why = MOVBA_LK_REJ_LOOP;
                break;
            }
            const int32_t jx = (int32_t)gx, jy = (int32_t)gy;
            const float ja = cx - gx, jb = cy - gy;
            const LkWeights v = lk_weights(ja, jb);
            typename Ex::Acc b1 = 0, b2 = 0;
#pragma unroll Ex::kUnroll
            for (int t = 0; t < Ex::kEntries; ++t) {
                if (pos[t] < 0) continue;
                const int32_t diff = lk_pixel(J, rows, cols, jx + (pos[t] & 31), jy + (pos[t] >> 5), v) - pI[t];
                b1 += diff * pIx[t]; b2 += diff * pIy[t];
            }
            const float B1 = lk_scaled(ex.sum(b1)), B2 = lk_scaled(ex.sum(b2));
            const float t1 = m.A12 * B2, t2 = m.A22 * B1, t3 = m.A12 * B1, t4 = m.A11 * B2;
            const float e1 = t1 - t2, e2 = t3 - t4;
            const float dx = e1 * D, dy = e2 * D;
            cx = cx + dx; cy = cy + dy;
            nx = cx + half; ny = cy + half;
            const double dx2 = (double)dx * (double)dx, dy2 = (double)dy * (double)dy, len2 = dx2 + dy2;
            if (len2 <= d.eps_sq) { why = MOVBA_LK_EPS; break; }
            const float ox = dx + prev_dx, oy = dy + prev_dy;
            if (j > 0 && fabs((double)ox) < 0.01 && fabs((double)oy) < 0.01) {
                const float hx = dx * 0.5f, hy = dy * 0.5f;
                nx = nx - hx; ny = ny - hy;
                why = MOVBA_LK_OSCILLATION;
                break;
            }
            prev_dx = dx; prev_dy = dy;
        }
        if (l == 0) out.exit_code = why;
    }
    out.x = nx; out.y = ny;
    return out;
}

// the gate of MOVExtractor.cc:98 and :354
__host__ __device__ inline bool lk_keep(const LkPoint &p, int32_t rows, int32_t cols)
{
    return p.status && p.x >= 0.f && p.x < (float)cols && p.y >= 0.f && p.y < (float)rows;
}

// the frame of item i of a prefix array: the f with ptr[f] <= i < ptr[f + 1] (i < ptr[n])
__host__ __device__ inline int32_t lk_frame_of(const int32_t *ptr, int32_t n, int32_t i)
{
    int32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) / 2;
        if (ptr[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// pixel j of level l (1 .. 3) over the call: [0, lvl_ptr[l-1][n_frames]) are the previous images', the same count again the next
__host__ __device__ inline void lk_pyr_item(const LkDev &d, int32_t l, int32_t j)
{
    const int32_t *ptr = d.lvl_ptr + (size_t)(l - 1) * (d.n_frames + 1), all = d.level_pixels[l - 1];
    const int32_t img = j >= all ? 1 : 0, k = j - img * all, f = lk_frame_of(ptr, d.n_frames, k);
    const LkFrame &fr = d.frame[f];
    const int32_t at = k - ptr[f], y = at / fr.cols[l], x = at - y * fr.cols[l];
    d.pix[fr.off[img][l] + at] = lk_pyr_pixel(d.pix + fr.off[img][l - 1], fr.rows[l - 1], fr.cols[l - 1], x, y);
}

__host__ __device__ inline void lk_write_point(const LkDev &d, int32_t i, const LkPoint &p, bool keep)
{
    d.next_pt[2 * (size_t)i] = p.x; d.next_pt[2 * (size_t)i + 1] = p.y;
    d.pt_status[i] = p.status; d.err[i] = p.err; d.exit_code[i] = p.exit_code; d.keep[i] = keep ? 1 : 0;
}

// the whole call, serially, in the kernels' order (host builds: the fake launch of tests/lk, tests/lk/lk_main.cpp, tests/dev/lk_loop.cpp)
inline void lk_frames(const LkDev &d)
{
    for (int32_t l = 1; l < kLkLevels; ++l) {
        const int32_t all = d.level_pixels[l - 1];
        for (int32_t j = 0; j < 2 * all; ++j) lk_pyr_item(d, l, j);
    }
    int32_t total = 0;
    for (int32_t f = 0; f < d.n_frames; ++f) {
        const LkFrame &fr = d.frame[f];
        d.kept_ptr[f] = total;
        d.kept_cnt[f] = 0;
        for (int32_t i = d.pt_ptr[f]; i < d.pt_ptr[f + 1]; ++i) {
            const LkPoint p = lk_point(d, fr, d.pt[2 * (size_t)i], d.pt[2 * (size_t)i + 1], LkSerial{});
            const bool keep = lk_keep(p, fr.rows[0], fr.cols[0]);
            lk_write_point(d, i, p, keep);
            if (keep) { d.kept_src[total++] = i - d.pt_ptr[f]; ++d.kept_cnt[f]; }
        }
    }
    d.kept_ptr[d.n_frames] = total;
    for (int32_t i = total; i < d.n_pt; ++i) d.kept_src[i] = -1;
}

}  // namespace movba
