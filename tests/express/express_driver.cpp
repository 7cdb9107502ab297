// Drives the HOST side of movba_express (mov-slam_amd/csrc/express.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_express.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or ThreadSanitizer.
// The fake launch runs the library's own steps; every value that comes back is checked here against the loops of
// EXPRESS.h:79-192 as include/movba.h restates them, pixel by pixel, without masks.  What is under test is the host's side: every
// refusal of the header before anything is written (canaries), calls without images or items, images with padded rows packed
// tightly, images without items and with a NULL pointer, the optional arrays left out, pinned against ordinary result memory,
// calls of growing and shrinking size on one handle, a handle shared with an uploaded and a solved window whose downloads and
// runs go on around the calls, movba_express_grid, and two handles on two threads.  Exit code 0 and the last line "express
// driver: ok" = every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_express_errors();

namespace {

int fails = 0;
int seen[32] = {};         // how often check() met each code
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr int32_t kCanary = -77;
constexpr uint8_t kCanaryB = 0xEE;
constexpr uint64_t kCanaryQ = 0x7777777777777777ull;
constexpr uint8_t kPoison = 0xA5;

struct Call {
    std::vector<std::vector<uint8_t>> pixels;       // per image rows x stride, the padding poisoned
    std::vector<const uint8_t *> image;
    std::vector<int32_t> rows, cols, stride, threshold, item_ptr, rect, mode;
    std::vector<uint64_t> ref;
    // results, each one entry longer than asked for: the canary behind the end
    std::vector<uint8_t> code;
    std::vector<uint64_t> desc;
    std::vector<int32_t> count, distance, n_features;
    movba_express_desc d{};
    movba_express_result r{};
    int ni = 0, n = 0;
};

void bind(Call &s, bool with_ref, bool with_distance)
{
    s.ni = (int)s.rows.size(); s.n = (int)s.mode.size();
    s.code.assign((size_t)s.n + 1, kCanaryB); s.desc.assign(4 * (size_t)s.n + 1, kCanaryQ);
    s.count.assign((size_t)s.n + 1, kCanary); s.distance.assign((size_t)s.n + 1, kCanary); s.n_features.assign((size_t)s.ni + 1, kCanary);
    s.d = movba_express_desc{};
    s.d.n_images = s.ni;
    s.d.image = s.image.data(); s.d.rows = s.rows.data(); s.d.cols = s.cols.data(); s.d.stride = s.stride.data(); s.d.threshold = s.threshold.data();
    s.d.item_ptr = s.item_ptr.data(); s.d.item_rect = s.rect.data(); s.d.item_mode = s.mode.data();
    s.d.item_ref = with_ref ? s.ref.data() : nullptr;
    s.r = movba_express_result{};
    s.r.code = s.code.data(); s.r.desc = s.desc.data(); s.r.count = s.count.data(); s.r.n_features = s.n_features.data();
    s.r.distance = with_distance ? s.distance.data() : nullptr;
    s.r.status = 99;
}

// ni images of up to max_rows x max_cols (a noisy step, noise, or one value; every third with padded rows; every fifth without
// items, every tenth of those with a NULL pointer), up to max_items rects each: most inside the image and of one of the four
// shapes, some outside it, some of other shapes
void make_call(Call &s, int ni, int max_rows, int max_cols, int max_items, bool with_ref, bool with_distance, unsigned seed)
{
    std::mt19937 rng(seed);
    s = Call{};
    s.item_ptr.assign(1, 0);
    for (int i = 0; i < ni; ++i) {
        const int rows = i == ni - 1 ? max_rows : 1 + (int)(rng() % (unsigned)max_rows), cols = i == ni - 1 ? max_cols : 1 + (int)(rng() % (unsigned)max_cols);
        const int stride = cols + (i % 3 == 1 ? 1 + (int)(rng() % 37) : 0), kind = (int)(rng() % 4);
        std::vector<uint8_t> px((size_t)rows * stride, kPoison);
        const int a = (int)(rng() % 256), b = (int)(rng() % 256), cut = (int)(rng() % (unsigned)(rows + cols));
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x)
                px[(size_t)y * stride + x] = kind == 0 ? (uint8_t)a : kind == 1 ? (uint8_t)(rng() % 256) : (uint8_t)std::clamp((x + y < cut ? a : b) + (int)(rng() % 9) - 4, 0, 255);
        const bool empty = i % 5 == 4 && i != ni - 1;
        s.pixels.push_back(std::move(px));
        s.rows.push_back(rows); s.cols.push_back(cols); s.stride.push_back(stride);
        s.threshold.push_back(i % 7 == 0 ? 0 : i % 7 == 3 ? 255 : 5 + (int)(rng() % 60));
        const int n = empty ? 0 : (int)(rng() % (unsigned)(max_items + 1));
        for (int k = 0; k < n; ++k) {
            const int w = 8 << (rng() % 2), h = 8 << (rng() % 2), roll = (int)(rng() % 16);
            int32_t rc[4] = { (int32_t)(rng() % (unsigned)std::max(1, cols - w)), (int32_t)(rng() % (unsigned)std::max(1, rows - h)), w, h };
            if (roll == 0) rc[0] = cols - w;                    // touches the last column: rejected
            if (roll == 1) rc[1] = -1 - (int32_t)(rng() % 9);
            if (roll == 2) { rc[2] = 4 << (rng() % 4); rc[3] = 32 >> (rng() % 4); }
            if (roll == 3) rc[0] = INT32_MAX - (int32_t)(rng() % 8);
            s.rect.insert(s.rect.end(), rc, rc + 4);
            s.mode.push_back(rng() % 3 == 0 ? MOVBA_EX_DESCRIBE : MOVBA_EX_DETECT);
            for (int q = 0; q < 4; ++q) s.ref.push_back(((uint64_t)rng() << 32) | rng());
        }
        s.item_ptr.push_back((int32_t)s.mode.size());
    }
    for (int i = 0; i < ni; ++i) s.image.push_back(s.item_ptr[i + 1] == s.item_ptr[i] && i % 10 == 9 ? nullptr : s.pixels[i].data());
    if (s.ref.empty()) s.ref.assign(4, 0);
    bind(s, with_ref, with_distance);
}

bool untouched(const Call &s)
{
    bool ok = true;
    for (uint8_t v : s.code) ok &= v == kCanaryB;
    for (uint64_t v : s.desc) ok &= v == kCanaryQ;
    for (const std::vector<int32_t> *a : { &s.count, &s.distance, &s.n_features })
        for (int32_t v : *a) ok &= v == kCanary;
    return ok;
}

// ---- EXPRESS.h:79-192 over one block, loop by loop ----

struct Blk {
    const uint8_t *p;
    int step, cols, rows;
    int at(int row, int col) const { return p[(size_t)row * step + col]; }
};

uint8_t center_of(const Blk &m)
{
    const uint8_t center_row = (uint8_t)(m.rows / 2), center_col = (uint8_t)(m.cols / 2);
    return (uint8_t)((m.at(center_col, center_row) + m.at(center_col - 1, center_row - 1) + m.at(center_col, center_row - 1) + m.at(center_col - 1, center_row)) / 4);
}

void descriptor_of(const Blk &m, int threshold, bool bits[256])
{
    const uint8_t center = center_of(m), low = (uint8_t)(center - threshold), high = (uint8_t)(center + threshold);
    std::fill(bits, bits + 256, false);
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols; ++x) {
            const int v = m.at(y, x + 1);
            if (low > v || high < v) bits[y * m.rows + x] = true;
        }
}

// -1: the precheck failed, 0: no pass succeeded, 1: one did
int express_of(const Blk &m, int threshold)
{
    const uint8_t center = center_of(m), low = (uint8_t)(center - threshold), high = (uint8_t)(center + threshold);
    const uint8_t precheck = (uint8_t)(m.rows * m.cols * .125);
    uint8_t f = 0;
    for (int row = 0; row < m.rows; ++row) {
        for (int col = 0; col < m.cols; ++col) {
            const int v = m.at(row, col + 1);
            if (low > v || high < v) f++;
        }
        if (f >= precheck) break;
    }
    if (f < precheck) return -1;
    const uint8_t slices = (uint8_t)(m.rows + m.cols - 1), rounds = (uint8_t)std::round(slices * .25), u_rounds = (uint8_t)(slices - rounds);
    for (int a = 0; a < 2; ++a) {
        uint8_t wins = 0, losses = 0;
        for (int i = 0; i < slices; ++i) {
            uint8_t win = 0, loss = 0;
            for (int y = 0; y < m.rows; ++y) {
                const int k = y + i - (m.rows - 1);
                if (k < 0 || k >= m.cols) continue;
                const int v = m.at(y, a == 0 ? k : m.cols - 1 - k);
                if (low > v || high < v) win++; else loss++;
            }
            if (wins < rounds) { if (win >= loss) wins++; else wins = 0; }
            if (losses < rounds) { if (loss > win) losses++; else losses = 0; }
            if (i > u_rounds && (wins == 0 || losses == 0)) break;
        }
        if (wins >= rounds && losses >= rounds) return 1;
    }
    return 0;
}

// what came back (pinned or not) against the loops
void check(const Call &s, const movba_express_result &r)
{
    bool ok = true;
    for (int i = 0; i < s.ni; ++i) {
        int features = 0;
        for (int k = s.item_ptr[i]; k < s.item_ptr[i + 1]; ++k) {
            const int32_t x = s.rect[4 * k], y = s.rect[4 * k + 1], w = s.rect[4 * k + 2], h = s.rect[4 * k + 3];
            int code;
            bool bits[256] = {};
            bool have = false;
            if (!(x >= 0 && y >= 0 && (long long)x + w < s.cols[i] && (long long)y + h < s.rows[i])) code = MOVBA_EX_REJ_BOUNDS;
            else if (!((w == 8 || w == 16) && (h == 8 || h == 16))) code = MOVBA_EX_REJ_SHAPE;
            else {
                const Blk m{ s.pixels[i].data() + (size_t)y * s.stride[i] + x, s.stride[i], w, h };
                if (s.mode[k] == MOVBA_EX_DESCRIBE) code = MOVBA_EX_DESCRIBED;
                else {
                    const int e = express_of(m, s.threshold[i]);
                    code = e < 0 ? MOVBA_EX_REJ_FLAT : e == 0 ? MOVBA_EX_REJ_NO_EDGE : MOVBA_EX_FEATURE;
                }
                have = code == MOVBA_EX_FEATURE || code == MOVBA_EX_DESCRIBED;
                if (have) descriptor_of(m, s.threshold[i], bits);
            }
            features += code == MOVBA_EX_FEATURE;
            __atomic_add_fetch(&seen[code], 1, __ATOMIC_RELAXED);
            int count = 0, dist = 0;
            for (int b = 0; b < 256; ++b) {
                const bool got = (r.desc[4 * (size_t)k + (b >> 6)] >> (b & 63)) & 1;
                ok &= got == bits[b];
                count += bits[b];
                if (s.d.item_ref) dist += bits[b] != (bool)((s.ref[4 * (size_t)k + (b >> 6)] >> (b & 63)) & 1);
            }
            ok &= r.code[k] == code && r.count[k] == (have ? count : -1);
            if (r.distance) ok &= r.distance[k] == (have && s.d.item_ref ? dist : -1);
        }
        ok &= r.n_features[i] == features;
    }
    EXPECT(ok);
}

void canaries_in_place(const Call &s)
{
    EXPECT(s.code[s.n] == kCanaryB && s.desc[4 * (size_t)s.n] == kCanaryQ && s.count[s.n] == kCanary && s.distance[s.n] == kCanary && s.n_features[s.ni] == kCanary);
}

// variant 0: ordinary results, 1: all pinned, 2: the descriptors and the counts pinned, the rest ordinary
void run_call(movba_handle *h, int ni, int max_rows, int max_cols, int max_items, unsigned seed, int variant)
{
    Call s;
    make_call(s, ni, max_rows, max_cols, max_items, seed % 2 == 0, seed % 3 != 0, seed);
    std::vector<void *> blocks;
    auto pin = [&](size_t bytes) { void *p = movba_host_alloc(bytes ? bytes : 8); EXPECT(p != nullptr); blocks.push_back(p); return p; };
    movba_express_result r = s.r;
    const size_t n = (size_t)s.n;
    if (variant == 1) { r.code = (uint8_t *)pin(n); r.n_features = (int32_t *)pin(4 * (size_t)s.ni); if (r.distance) r.distance = (int32_t *)pin(4 * n); }
    if (variant >= 1) { r.desc = (uint64_t *)pin(32 * n); r.count = (int32_t *)pin(4 * n); }
    for (void *p : blocks) if (!p) return;
    EXPECT(movba_express(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK);
    if (s.n) check(s, r);
    if (variant == 0 && !s.n) EXPECT(untouched(s));
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_images, most rows, most columns, most items of an image
    const int rounds[][4] = { { 3, 30, 40, 9 }, { 12, 120, 200, 300 }, { 1, 17, 17, 1 }, { 2, 1080, 1920, 4000 }, { 40, 64, 48, 60 },
                              { 5, 16, 16, 7 }, { 64, 90, 33, 25 }, { 4, 257, 19, 0 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], q[3], seed + k, k % 3); ++k; }
}

void grid_calls()
{
    const int sizes[][2] = { { 16, 16 }, { 17, 17 }, { 24, 24 }, { 25, 40 }, { 240, 320 }, { 1080, 1920 }, { 8, 400 }, { 400, 9 }, { 0, 0 }, { -5, 100 } };
    for (const auto &q : sizes) {
        std::vector<int32_t> want;
        for (int y = 8; y < q[0] - 8; y += 16)
            for (int x = 8; x < q[1] - 8; x += 16) { const int32_t rc[4] = { x - 8, y - 8, 16, 16 }; want.insert(want.end(), rc, rc + 4); }
        const int n = (int)want.size() / 4;
        EXPECT(movba_express_grid(q[0], q[1], nullptr, 0) == n);
        std::vector<int32_t> got(want.size() + 1, kCanary);
        EXPECT(movba_express_grid(q[0], q[1], got.data(), n) == n && got[want.size()] == kCanary);
        got.pop_back();
        EXPECT(got == want);
        if (n > 1) {                    // a cap below the count: the first rects, the count all the same
            std::vector<int32_t> part(4 * (size_t)(n - 1) + 1, kCanary);
            EXPECT(movba_express_grid(q[0], q[1], part.data(), n - 1) == n && part[4 * (size_t)(n - 1)] == kCanary);
            EXPECT(std::equal(part.begin(), part.end() - 1, want.begin()));
        }
    }
    EXPECT(movba_express_grid(1080, 1920, nullptr, 0) == 7973);
    int32_t one[4];
    EXPECT(movba_express_grid(100, 100, one, -1) == MOVBA_ERR_ARG && movba_express_grid(100, 100, nullptr, 3) == MOVBA_ERR_ARG);
    EXPECT(movba_express_grid(INT32_MAX, INT32_MAX, nullptr, 0) == MOVBA_ERR_ARG && movba_express_grid(INT32_MAX, 17, nullptr, 0) == (INT32_MAX - 17) / 16 + 1);
    EXPECT(movba_express_grid(INT32_MAX, 17, one, 1) > 0 && one[0] == 0 && one[1] == 0 && one[2] == 16 && one[3] == 16);
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 32; ++which) {
        Call s;
        make_call(s, 6, 40, 50, 30, true, true, 4u);
        EXPECT(s.item_ptr[1] > 0 && s.item_ptr[2] > s.item_ptr[1] && s.item_ptr[5] == s.item_ptr[4] && s.n > 8);     // (the cases below count on these)
        movba_express_desc &d = s.d;
        movba_express_result &r = s.r;
        switch (which) {
        case 0: d.n_images = -1; break;
        case 1: d.n_images = MOVBA_MAX_EXPRESS_IMAGES + 1; break;
        case 2: d.item_ptr = nullptr; break;
        case 3: s.item_ptr[0] = 1; break;
        case 4: s.item_ptr[3] = s.item_ptr[2] - 1; break;               // descending
        case 5: s.item_ptr[0] = -1; break;
        case 6: for (size_t k = 1; k < s.item_ptr.size(); ++k) s.item_ptr[k] = MOVBA_MAX_EXPRESS_ITEMS + 1; break;       // nothing behind it is read
        case 7: d.image = nullptr; break;
        case 8: d.rows = nullptr; break;
        case 9: d.cols = nullptr; break;
        case 10: d.stride = nullptr; break;
        case 11: d.threshold = nullptr; break;
        case 12: d.item_rect = nullptr; break;
        case 13: d.item_mode = nullptr; break;
        case 14: r.code = nullptr; break;
        case 15: r.desc = nullptr; break;
        case 16: r.count = nullptr; break;
        case 17: r.n_features = nullptr; break;
        case 18: s.image[1] = nullptr; break;                           // an image that has items
        case 19: s.rows[2] = 0; break;
        case 20: s.cols[0] = 0; break;
        case 21: s.rows[4] = -3; break;                                 // (an image without items is checked all the same)
        case 22: s.stride[1] = s.cols[1] - 1; break;
        case 23: s.threshold[0] = -1; break;
        case 24: s.threshold[3] = 256; break;
        case 25: s.mode[5] = 2; break;
        case 26: s.mode[0] = -1; break;
        case 27: for (int i = 0; i < 6; ++i) { s.rows[i] = 16384; s.cols[i] = 16384; s.stride[i] = 16384; } break;     // 6 x 2^28 pixels: refused before a pixel is read
        case 28: s.mode[s.n - 1] = 77; break;
        case 29: s.threshold[4] = 1000; break;
        case 30: s.stride[4] = 0; break;
        case 31: s.item_ptr[6] = s.item_ptr[5] - 1; break;
        }
        const int rc = movba_express(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, 5, 30, 44, 12, true, true, 5u);
    EXPECT(movba_express(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_express(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_express(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    // what is not wrong: no distance array, no references, a reference without the distance array
    EXPECT(movba_express(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    s.r.distance = nullptr;
    EXPECT(movba_express(h, &s.d, &s.r) == MOVBA_OK);
    check(s, s.r);
    bind(s, false, true);
    EXPECT(movba_express(h, &s.d, &s.r) == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    // no images, or no items: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    {
        Call e;
        make_call(e, 4, 20, 20, 3, true, true, 8u);
        e.d.n_images = 0;
        EXPECT(movba_express(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        EXPECT(untouched(e));
        bind(e, true, true);
        std::fill(e.item_ptr.begin(), e.item_ptr.end(), 0);
        e.d.rows = nullptr; e.r.code = nullptr;
        EXPECT(movba_express(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        EXPECT(untouched(e));
        movba_express_desc none{};
        movba_express_result r0{};
        r0.status = 99;
        EXPECT(movba_express(h, &none, &r0) == MOVBA_OK && r0.status == MOVBA_OK);
    }
}

struct Win {
    std::vector<double> poses, points, obs, isig, out_poses, out_points, out_chi2;
    std::vector<uint8_t> fixed, out_outlier;
    std::vector<int32_t> ep, el;
    movba_lba_desc d{};
    movba_lba_result r{};
};

void make_window(Win &w, int NP, int P, unsigned seed)
{
    std::mt19937 rng(seed);
    w.poses.assign(7 * (size_t)NP, 0.0); w.fixed.assign(NP, 0); w.points.resize(3 * (size_t)P);
    for (int i = 0; i < NP; ++i) { w.poses[7 * i + 3] = 1.0; w.poses[7 * i + 4] = 0.3 * i; w.poses[7 * i + 5] = 0.01 * (double)(rng() % 50); w.fixed[i] = i < 2; }
    for (double &x : w.points) x = 1.0 + 0.001 * (double)(rng() % 4000);
    for (int l = 0; l < P; ++l)
        for (int k = l % (NP - 2); k < l % (NP - 2) + 3; ++k) { w.ep.push_back(k); w.el.push_back(l); }
    const size_t E = w.ep.size();
    w.obs.assign(2 * E, 100.0); w.isig.assign(E, 1.0);
    w.d.n_poses = NP; w.d.n_points = P; w.d.n_edges = (int32_t)E;
    w.d.poses = w.poses.data(); w.d.pose_fixed = w.fixed.data(); w.d.points = w.points.data();
    w.d.edge_pose = w.ep.data(); w.d.edge_point = w.el.data(); w.d.obs = w.obs.data(); w.d.inv_sigma2 = w.isig.data();
    w.d.fx = w.d.fy = 320; w.d.cx = 320; w.d.cy = 240; w.d.huber_delta = 2.236; w.d.chi2_gate = 5.0; w.d.max_iters = 10; w.d.flags = MOVBA_FLAG_STALE_ERROR_QUIRK;
    w.out_poses.assign(7 * (size_t)NP, 0.0); w.out_points.assign(3 * (size_t)P, 0.0); w.out_chi2.assign(E, 0.0); w.out_outlier.assign(E, 9);
    w.r.poses = w.out_poses.data(); w.r.points = w.out_points.data(); w.r.chi2 = w.out_chi2.data(); w.r.outlier = w.out_outlier.data();
}

// the call between the steps of a window's life on the same handle: the window, its download and its runs go on as they were
void beside_a_window(movba_handle *h, int reps, unsigned seed)
{
    Win w;
    make_window(w, 9, 600, seed);
    for (int rep = 0; rep < reps; ++rep) {
        EXPECT(movba_lba_upload(h, &w.d) == MOVBA_OK);
        run_call(h, 8, 60, 80, 40, seed + 1, rep % 3);                           // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, 31, 100, 90, 70, seed + 2, (rep + 1) % 3);                   // solved, not downloaded
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        const std::vector<double> first = w.out_poses;
        run_call(h, 3, 480, 640, 1200, seed + 3, (rep + 2) % 3);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        run_call(h, 4, 50, 50, 20, seed + 4, 0);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first);
    }
}

}  // namespace

int main()
{
    grid_calls();
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        invalid_calls(h);
        growing_and_shrinking(h, 11u);
        beside_a_window(h, 2, 40u);
        invalid_calls(h);
        movba_destroy(h);
    }
    {
        auto ex_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            for (int it = 0; it < 2; ++it) growing_and_shrinking(h, seed + 100 * it);
            movba_destroy(h);
        };
        auto lba_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            beside_a_window(h, 2, seed);
            movba_destroy(h);
        };
        std::thread a(ex_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_express_errors() == 0);
    for (int code : { MOVBA_EX_FEATURE, MOVBA_EX_DESCRIBED, MOVBA_EX_REJ_BOUNDS, MOVBA_EX_REJ_SHAPE, MOVBA_EX_REJ_FLAT, MOVBA_EX_REJ_NO_EDGE }) EXPECT(seen[code] >= 100);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("express driver: ok\n");
    return 0;
}
