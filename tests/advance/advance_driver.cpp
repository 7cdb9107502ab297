// Drives the HOST side of movba_advance (mov-slam_amd/csrc/advance.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_advance.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or ThreadSanitizer.
// The fake launch runs the library's own steps (whose values tests/test_advance_cpu.py holds to the restatement through
// adv_main.cpp); what is under test here is the host's side: every refusal of the header before anything is written (canaries),
// calls without frames, frames with padded rows packed tightly, frames without items and with a NULL image, grid_ptr left out,
// pinned against ordinary result memory, calls of growing and shrinking size on one handle, a handle shared with an uploaded and
// a solved window whose downloads and runs go on around the calls, and two handles on two threads.  What comes back is checked
// against the rules that tie the arrays together: `order` is the sorted permutation, the segments are dense and padded, ids and
// counts add up, kept features carry their source's track and age, claims and fates agree with kp_found.  Exit code 0 and the
// last line "advance driver: ok" = every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_advance_errors();

namespace {

int fails = 0;
int seen[32] = {};         // how often check() met each fate
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr uint8_t kCanary = 0xEE, kPoison = 0xA5;

int lattice(int rows, int cols) { return rows <= 16 || cols <= 16 ? 0 : ((rows - 17) / 16 + 1) * ((cols - 17) / 16 + 1); }

// one result array of the caller with a canary element behind its end
struct Arr {
    std::vector<uint8_t> bytes;
    size_t used = 0;
    void size(size_t n, size_t elem) { used = n * elem; bytes.assign(used + elem, kCanary); }
    template <typename T> T *as() { return reinterpret_cast<T *>(bytes.data()); }
    template <typename T> const T *as() const { return reinterpret_cast<const T *>(bytes.data()); }
    bool untouched() const { return std::all_of(bytes.begin(), bytes.end(), [](uint8_t v) { return v == kCanary; }); }
    bool canary() const { return std::all_of(bytes.begin() + (long)used, bytes.end(), [](uint8_t v) { return v == kCanary; }); }
};

struct Call {
    std::vector<std::vector<uint8_t>> pixels;
    std::vector<const uint8_t *> image;
    std::vector<int32_t> rows, cols, stride, threshold, first_id, prev_ptr, mv_ptr, kp_ptr, grid_ptr;
    std::vector<uint8_t> force_grid, prev_coverage, grid_covered;
    std::vector<float> prev_pt, mv_pt;
    std::vector<int32_t> prev_mb, prev_age, prev_track, prev_cand, mv_dindx, kp_rect;
    std::vector<uint64_t> prev_desc;
    Arr out[16];            // in the order of movba_advance_result's fields
    movba_advance_desc d{};
    movba_advance_result r{};
    size_t nf = 0, np = 0, nk = 0, ng = 0, cap = 0;
};

void bind(Call &s, bool with_grid)
{
    s.nf = s.rows.size(); s.np = s.prev_age.size(); s.nk = s.kp_rect.size() / 4; s.ng = s.grid_covered.size(); s.cap = s.np + s.nk + s.ng;
    const size_t n[16] = { s.np, s.np, s.np, s.np, s.nk, s.nk, s.nf, s.nf, s.nf, 4 * s.nf + 1, s.cap, s.cap, 2 * s.cap, 4 * s.cap, s.cap, 4 * s.cap };
    const size_t elem[16] = { 4, 1, 4, 4, 1, 1, 4, 1, 4, 4, 4, 4, 4, 4, 4, 8 };
    for (int k = 0; k < 16; ++k) s.out[k].size(n[k], elem[k]);
    movba_advance_desc &d = s.d;
    d = movba_advance_desc{};
    d.n_frames = (int32_t)s.nf;
    d.image = s.image.data(); d.rows = s.rows.data(); d.cols = s.cols.data(); d.stride = s.stride.data(); d.threshold = s.threshold.data();
    d.force_grid = s.force_grid.data(); d.first_id = s.first_id.data(); d.prev_ptr = s.prev_ptr.data(); d.prev_pt = s.prev_pt.data();
    d.prev_mb = s.prev_mb.data(); d.prev_age = s.prev_age.data(); d.prev_track = s.prev_track.data(); d.prev_desc = s.prev_desc.data();
    d.prev_coverage = s.prev_coverage.data(); d.prev_cand = s.prev_cand.data(); d.mv_ptr = s.mv_ptr.data(); d.mv_pt = s.mv_pt.data();
    d.mv_dindx = s.mv_dindx.data(); d.kp_ptr = s.kp_ptr.data(); d.kp_rect = s.kp_rect.data();
    d.grid_ptr = with_grid ? s.grid_ptr.data() : nullptr; d.grid_covered = with_grid ? s.grid_covered.data() : nullptr;
    movba_advance_result &r = s.r;
    r = movba_advance_result{};
    r.order = s.out[0].as<int32_t>(); r.fate = s.out[1].as<uint8_t>(); r.chosen_mv = s.out[2].as<int32_t>(); r.distance = s.out[3].as<int32_t>();
    r.kp_found = s.out[4].as<uint8_t>(); r.kp_code = s.out[5].as<uint8_t>(); r.mov_cnt = s.out[6].as<int32_t>(); r.grid_ran = s.out[7].as<uint8_t>();
    r.next_id = s.out[8].as<int32_t>(); r.seg_ptr = s.out[9].as<int32_t>(); r.feat_src = s.out[10].as<int32_t>(); r.feat_track = s.out[11].as<int32_t>();
    r.feat_pt = s.out[12].as<float>(); r.feat_rect = s.out[13].as<int32_t>(); r.feat_age = s.out[14].as<int32_t>(); r.feat_desc = s.out[15].as<uint64_t>();
    r.status = 99;
}

// nf frames of up to max_rows x max_cols (a noisy step, noise, or one value; every third with padded rows; every fifth without
// anything, every tenth of those with a NULL image - such frames are at most 16 x 16, so they have no lattice either), up to
// max_prev previous features, max_prev / 2 vectors and max_kps macroblocks each
void make_call(Call &s, int nf, int max_rows, int max_cols, int max_prev, int max_kps, bool with_grid, unsigned seed)
{
    std::mt19937 rng(seed);
    s = Call{};
    s.prev_ptr.assign(1, 0); s.mv_ptr.assign(1, 0); s.kp_ptr.assign(1, 0); s.grid_ptr.assign(1, 0);
    for (int i = 0; i < nf; ++i) {
        const bool empty = i % 5 == 4 && i != nf - 1;
        const int rows = empty ? 1 + (int)(rng() % 16) : i == nf - 1 ? max_rows : 18 + (int)(rng() % (unsigned)std::max(1, max_rows - 17));
        const int cols = empty ? 1 + (int)(rng() % 16) : i == nf - 1 ? max_cols : 18 + (int)(rng() % (unsigned)std::max(1, max_cols - 17));
        const int stride = cols + (i % 3 == 1 ? 1 + (int)(rng() % 37) : 0), kind = (int)(rng() % 4);
        std::vector<uint8_t> px((size_t)rows * stride, kPoison);
        const int a = (int)(rng() % 256), b = (int)(rng() % 256), cut = (int)(rng() % (unsigned)(rows + cols));
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x)
                px[(size_t)y * stride + x] = kind == 0 ? (uint8_t)a : kind == 1 ? (uint8_t)(rng() % 256) : (uint8_t)std::clamp((x + y < cut ? a : b) + (int)(rng() % 9) - 4, 0, 255);
        s.pixels.push_back(std::move(px));
        s.rows.push_back(rows); s.cols.push_back(cols); s.stride.push_back(stride);
        s.threshold.push_back(i % 7 == 0 ? 0 : i % 7 == 3 ? 255 : 5 + (int)(rng() % 60));
        s.force_grid.push_back((uint8_t)(rng() % 3 == 0 ? 7 : 0));
        s.first_id.push_back(i % 4 == 3 ? (1 << 30) : (int32_t)(rng() % 1000));
        const int np = empty ? 0 : (int)(rng() % (unsigned)(max_prev + 1)), nm = empty || !np ? 0 : 1 + np / 2, nk = empty ? 0 : (int)(rng() % (unsigned)(max_kps + 1));
        for (int k = 0; k < nk; ++k) {
            const int w = 8 << (rng() % 2), h = 8 << (rng() % 2), roll = (int)(rng() % 16);
            int32_t rc[4] = { (int32_t)(rng() % (unsigned)std::max(1, cols - w)), (int32_t)(rng() % (unsigned)std::max(1, rows - h)), w, h };
            if (roll == 0) rc[0] = cols - w;
            if (roll == 1) rc[1] = -1 - (int32_t)(rng() % 9);
            if (roll == 2) { rc[2] = 4 << (rng() % 4); rc[3] = 32 >> (rng() % 4); }
            if (roll == 3) rc[0] = INT32_MAX - (int32_t)(rng() % 8);
            s.kp_rect.insert(s.kp_rect.end(), rc, rc + 4);
        }
        for (int m = 0; m < nm; ++m) {
            s.mv_pt.push_back((float)((int)(rng() % 97) - 48) * 0.25f); s.mv_pt.push_back((float)((int)(rng() % 97) - 48) * 0.25f);
            s.mv_dindx.push_back(nk ? (int32_t)(rng() % (unsigned)(nk + 1)) - 1 : -1);
        }
        for (int k = 0; k < np; ++k) {
            s.prev_pt.push_back((float)(rng() % (unsigned)(4 * cols)) * 0.25f); s.prev_pt.push_back((float)(rng() % (unsigned)(4 * rows)) * 0.25f);
            s.prev_mb.push_back(8 << (rng() % 2)); s.prev_mb.push_back(8 << (rng() % 2));
            s.prev_age.push_back(k % 11 == 0 ? INT32_MAX - 1 : (int32_t)(rng() % 3));
            s.prev_track.push_back((int32_t)s.prev_track.size() + 5000);
            const bool blank = rng() % 3 == 0;      // (the descriptor of every block of a one-value frame: such features are kept)
            for (int q = 0; q < 4; ++q) s.prev_desc.push_back(blank ? 0 : ((uint64_t)rng() << 32) | rng());
            s.prev_coverage.push_back((uint8_t)(rng() % 9 == 0));
            const int nc = (int)(rng() % 5);
            for (int c = 0; c < 4; ++c) s.prev_cand.push_back(c < nc ? (int32_t)(rng() % (unsigned)nm) : -1);
        }
        const int ng = lattice(rows, cols);
        for (int g = 0; g < ng; ++g) s.grid_covered.push_back((uint8_t)(rng() % 4 == 0 ? 3 : 0));
        s.prev_ptr.push_back((int32_t)s.prev_age.size()); s.mv_ptr.push_back((int32_t)s.mv_dindx.size());
        s.kp_ptr.push_back((int32_t)s.kp_rect.size() / 4); s.grid_ptr.push_back((int32_t)s.grid_covered.size());
    }
    for (int i = 0; i < nf; ++i) s.image.push_back(i % 10 == 9 && i != nf - 1 ? nullptr : s.pixels[i].data());
    // (data() of an empty vector may be NULL, which the call refuses only where the counts need the array)
    for (std::vector<int32_t> *v : { &s.prev_mb, &s.prev_age, &s.prev_track, &s.prev_cand, &s.mv_dindx, &s.kp_rect }) v->reserve(1);
    s.prev_pt.reserve(1); s.mv_pt.reserve(1); s.prev_desc.reserve(1); s.prev_coverage.reserve(1); s.grid_covered.reserve(1);
    bind(s, with_grid);
}

bool untouched(const Call &s)
{
    bool ok = true;
    for (const Arr &a : s.out) ok &= a.untouched();
    return ok;
}

void canaries_in_place(const Call &s)
{
    for (const Arr &a : s.out) EXPECT(a.canary());
}

uint64_t sort_key(const Call &s, size_t g)
{
    int count = 0;
    for (int q = 0; q < 4; ++q) count += __builtin_popcountll(s.prev_desc[4 * g + q]);
    return ((uint64_t)(uint32_t)(INT32_MAX - s.prev_age[g]) << 32) | (uint64_t)(256 - count);
}

// what came back (pinned or not) against the rules that tie the arrays together
void check(const Call &s, const movba_advance_result &r)
{
    bool ok = true;
    int32_t at = 0;
    for (size_t f = 0; f < s.nf; ++f) {
        const int32_t p0 = s.prev_ptr[f], np = s.prev_ptr[f + 1] - p0, k0 = s.kp_ptr[f], nk = s.kp_ptr[f + 1] - k0, ng = lattice(s.rows[f], s.cols[f]);
        // order: a permutation, ascending by (age descending, count descending, index ascending)
        std::vector<char> hit((size_t)np, 0);
        for (int32_t i = 0; i < np; ++i) {
            const int32_t idx = r.order[p0 + i];
            ok &= idx >= 0 && idx < np && !hit[(size_t)std::clamp(idx, 0, np - 1)];
            if (idx < 0 || idx >= np) continue;
            hit[(size_t)idx] = 1;
            if (i) {
                const int32_t before = r.order[p0 + i - 1];
                const uint64_t a = sort_key(s, (size_t)(p0 + before)), b = sort_key(s, (size_t)(p0 + idx));
                ok &= a < b || (a == b && before < idx);
            }
        }
        // fates against claims: a macroblock is found exactly when some feature that arrived (kept, far or lost) has it as dindx
        std::vector<char> reached((size_t)nk, 0);
        int32_t kept = 0;
        for (int32_t i = 0; i < np; ++i) {
            const size_t g = (size_t)(p0 + i);
            const int fate = r.fate[g];
            __atomic_add_fetch(&seen[fate & 31], 1, __ATOMIC_RELAXED);
            ok &= fate == MOVBA_ADV_KEPT || fate == MOVBA_ADV_COVERAGE || fate == MOVBA_ADV_NO_MV || fate == MOVBA_ADV_REJ_BOUNDS || fate == MOVBA_ADV_LOST_CLAIM || fate == MOVBA_ADV_FAR;
            ok &= (fate == MOVBA_ADV_COVERAGE) == (s.prev_coverage[g] != 0);
            if (fate == MOVBA_ADV_COVERAGE || fate == MOVBA_ADV_NO_MV) { ok &= r.chosen_mv[g] == -1 && r.distance[g] == -1; continue; }
            const int32_t m = r.chosen_mv[g];
            ok &= m >= 0 && m < s.mv_ptr[f + 1] - s.mv_ptr[f];
            if (m < 0 || m >= s.mv_ptr[f + 1] - s.mv_ptr[f]) continue;
            ok &= m == s.prev_cand[4 * g] || m == s.prev_cand[4 * g + 1] || m == s.prev_cand[4 * g + 2] || m == s.prev_cand[4 * g + 3];
            if (fate == MOVBA_ADV_REJ_BOUNDS) { ok &= r.distance[g] == -1; continue; }
            ok &= r.distance[g] >= 0 && r.distance[g] <= 256;
            ok &= fate == MOVBA_ADV_LOST_CLAIM || (fate == MOVBA_ADV_KEPT) == (r.distance[g] <= 40);
            const int32_t dst = s.mv_dindx[(size_t)(s.mv_ptr[f] + m)];
            ok &= fate != MOVBA_ADV_LOST_CLAIM || dst >= 0;
            if (dst >= 0) reached[(size_t)dst] = 1;
            kept += fate == MOVBA_ADV_KEPT;
        }
        int32_t fresh = 0;
        for (int32_t m = 0; m < nk; ++m) {
            ok &= r.kp_found[k0 + m] == reached[(size_t)m];
            ok &= r.kp_found[k0 + m] ? r.kp_code[k0 + m] == 0 : r.kp_code[k0 + m] == MOVBA_EX_FEATURE || (r.kp_code[k0 + m] >= MOVBA_EX_REJ_BOUNDS && r.kp_code[k0 + m] <= MOVBA_EX_REJ_NO_EDGE);
            fresh += r.kp_code[k0 + m] == MOVBA_EX_FEATURE;
        }
        const int32_t *seg = r.seg_ptr + 4 * f;
        const int32_t grid = seg[3] - seg[2];
        ok &= seg[0] == at && seg[1] - seg[0] == kept && seg[2] - seg[1] == fresh && grid >= 0 && grid <= ng;
        ok &= r.mov_cnt[f] == fresh && r.grid_ran[f] == (s.force_grid[f] || fresh < 60) && (r.grid_ran[f] || grid == 0);
        ok &= r.next_id[f] == s.first_id[f] + fresh + grid;
        for (int32_t o = seg[0]; o < seg[1] && ok; ++o) {
            const int32_t i = r.feat_src[o];
            ok &= i >= 0 && i < np && (o == seg[0] || r.feat_src[o - 1] < i);
            if (i < 0 || i >= np) break;
            const size_t g = (size_t)(p0 + r.order[p0 + i]);
            ok &= r.fate[g] == MOVBA_ADV_KEPT && r.feat_track[o] == s.prev_track[g] && r.feat_age[o] == s.prev_age[g] + 1;
            ok &= r.feat_rect[4 * o + 2] == s.prev_mb[2 * g] && r.feat_rect[4 * o + 3] == s.prev_mb[2 * g + 1];
            ok &= r.feat_rect[4 * o] == (int32_t)(r.feat_pt[2 * o] - (float)(s.prev_mb[2 * g] / 2));
        }
        for (int32_t o = seg[1]; o < seg[3] && ok; ++o) {
            ok &= r.feat_track[o] == s.first_id[f] + 1 + (o - seg[1]) && r.feat_age[o] == 0;
            ok &= r.feat_pt[2 * o] == (float)(r.feat_rect[4 * o] + r.feat_rect[4 * o + 2] / 2) && r.feat_pt[2 * o + 1] == (float)(r.feat_rect[4 * o + 1] + r.feat_rect[4 * o + 3] / 2);
            if (o < seg[2]) ok &= r.kp_code[k0 + r.feat_src[o]] == MOVBA_EX_FEATURE && std::equal(r.feat_rect + 4 * o, r.feat_rect + 4 * o + 4, s.kp_rect.begin() + 4 * (k0 + r.feat_src[o]));
            else ok &= r.feat_src[o] >= 0 && r.feat_src[o] < ng && r.feat_rect[4 * o + 2] == 16 && (!s.d.grid_ptr || !s.grid_covered[(size_t)(s.grid_ptr[f] + r.feat_src[o])]);
        }
        at = seg[3];
    }
    ok &= r.seg_ptr[4 * s.nf] == at;
    for (size_t o = (size_t)at; o < s.cap; ++o) {
        ok &= r.feat_src[o] == -1 && r.feat_track[o] == -1 && r.feat_age[o] == -1 && std::isnan(r.feat_pt[2 * o]) && std::isnan(r.feat_pt[2 * o + 1]);
        for (int q = 0; q < 4; ++q) ok &= r.feat_rect[4 * o + q] == -1 && r.feat_desc[4 * o + q] == 0;
    }
    EXPECT(ok);
}

// variant 0: ordinary results; 1: then once more with all results pinned; 2: with the feature list pinned and the rest ordinary
// (written a second time over the first call's arrays) - held to the ordinary result bit by bit
void run_call(movba_handle *h, int nf, int max_rows, int max_cols, int max_prev, int max_kps, unsigned seed, int variant)
{
    Call s;
    make_call(s, nf, max_rows, max_cols, max_prev, max_kps, seed % 2 == 0, seed);
    EXPECT(movba_advance(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    if (variant == 0) return;
    std::vector<void *> blocks;
    movba_advance_result r = s.r;
    void **field[16] = { (void **)&r.order, (void **)&r.fate, (void **)&r.chosen_mv, (void **)&r.distance, (void **)&r.kp_found, (void **)&r.kp_code,
                         (void **)&r.mov_cnt, (void **)&r.grid_ran, (void **)&r.next_id, (void **)&r.seg_ptr, (void **)&r.feat_src, (void **)&r.feat_track,
                         (void **)&r.feat_pt, (void **)&r.feat_rect, (void **)&r.feat_age, (void **)&r.feat_desc };
    for (int k = variant == 1 ? 0 : 10; k < 16; ++k) {
        void *p = movba_host_alloc(s.out[k].used ? s.out[k].used : 8);
        EXPECT(p != nullptr);
        if (!p) return;
        blocks.push_back(p);
        *field[k] = p;
    }
    EXPECT(movba_advance(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK);
    check(s, r);
    for (int k = variant == 1 ? 0 : 10; k < 16; ++k) EXPECT(std::memcmp(*field[k], s.out[k].bytes.data(), s.out[k].used) == 0);
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_frames, most rows, most columns, most previous features, most macroblocks of a frame
    const int rounds[][5] = { { 3, 30, 40, 9, 5 }, { 12, 120, 200, 300, 200 }, { 1, 17, 17, 1, 1 }, { 2, 270, 480, 3000, 600 }, { 40, 64, 48, 60, 30 },
                              { 5, 18, 18, 7, 0 }, { 64, 90, 33, 25, 40 }, { 4, 257, 19, 0, 9 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], q[3], q[4], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 44; ++which) {
        Call s;
        make_call(s, 6, 40, 50, 30, 20, true, 4u);
        EXPECT(s.prev_ptr[1] > 1 && s.mv_ptr[1] > 0 && s.kp_ptr[1] > 0 && s.prev_ptr[5] == s.prev_ptr[4] && s.np > 8);     // (the cases below count on these)
        movba_advance_desc &d = s.d;
        movba_advance_result &r = s.r;
        switch (which) {
        case 0: d.n_frames = -1; break;
        case 1: d.n_frames = MOVBA_MAX_EXPRESS_IMAGES + 1; break;
        case 2: d.prev_ptr = nullptr; break;
        case 3: d.mv_ptr = nullptr; break;
        case 4: d.kp_ptr = nullptr; break;
        case 5: s.prev_ptr[0] = 1; break;
        case 6: s.mv_ptr[3] = s.mv_ptr[2] - 1; break;
        case 7: s.kp_ptr[0] = -1; break;
        case 8: s.grid_ptr[0] = 1; break;
        case 9: s.grid_ptr[1] += 1; break;                              // not the lattice's length
        case 10: d.image = nullptr; break;
        case 11: d.rows = nullptr; break;
        case 12: d.stride = nullptr; break;
        case 13: d.force_grid = nullptr; break;
        case 14: d.first_id = nullptr; break;
        case 15: d.prev_pt = nullptr; break;
        case 16: d.prev_desc = nullptr; break;
        case 17: d.prev_cand = nullptr; break;
        case 18: d.mv_pt = nullptr; break;
        case 19: d.mv_dindx = nullptr; break;
        case 20: d.kp_rect = nullptr; break;
        case 21: d.grid_covered = nullptr; break;
        case 22: r.order = nullptr; break;
        case 23: r.kp_found = nullptr; break;
        case 24: r.seg_ptr = nullptr; break;
        case 25: r.feat_desc = nullptr; break;
        case 26: s.image[0] = nullptr; break;                           // a frame that has items
        case 27: s.rows[2] = 0; break;
        case 28: s.stride[1] = s.cols[1] - 1; break;
        case 29: s.threshold[3] = 256; break;
        case 30: s.prev_mb[1] = 12; break;
        case 31: s.prev_mb[0] = 32; break;
        case 32: s.prev_age[1] = -1; break;
        case 33: s.prev_age[0] = INT32_MAX; break;
        case 34: s.prev_cand[2] = -2; break;
        case 35: s.prev_cand[5] = s.mv_ptr[1]; break;                   // one past the frame's vectors
        case 36: s.mv_dindx[0] = s.kp_ptr[1]; break;
        case 37: s.mv_dindx[0] = -2; break;
        case 38: s.prev_pt[1] = NAN; break;
        case 39: s.prev_pt[0] = 1048577.0f; break;
        case 40: s.mv_pt[0] = -INFINITY; break;
        case 41: s.first_id[0] = -1; break;
        case 42: s.first_id[0] = INT32_MAX - 2; break;                  // first_id + n_kps + n_grid above INT32_MAX
        case 43: for (size_t i = 1; i < s.prev_ptr.size(); ++i) s.prev_ptr[i] = MOVBA_MAX_ADVANCE_PREV + 1; break;      // nothing behind it is read
        }
        const int rc = movba_advance(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, 5, 30, 44, 12, 9, true, 5u);
    EXPECT(movba_advance(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_advance(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_advance(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    EXPECT(movba_advance(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    // no frames: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    Call e;
    make_call(e, 4, 20, 20, 3, 3, true, 8u);
    e.d.n_frames = 0; e.d.prev_ptr = nullptr; e.r.order = nullptr;
    EXPECT(movba_advance(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
    EXPECT(untouched(e));
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
        run_call(h, 8, 60, 80, 40, 30, seed + 1, rep % 3);                          // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, 31, 100, 90, 70, 50, seed + 2, (rep + 1) % 3);                  // solved, not downloaded
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        const std::vector<double> first = w.out_poses;
        run_call(h, 3, 240, 320, 1200, 800, seed + 3, (rep + 2) % 3);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        run_call(h, 4, 50, 50, 20, 10, seed + 4, 0);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first);
    }
}

}  // namespace

int main()
{
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
        auto adv_thread = [](unsigned seed) {
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
        std::thread a(adv_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_advance_errors() == 0);
    for (int fate : { MOVBA_ADV_KEPT, MOVBA_ADV_COVERAGE, MOVBA_ADV_NO_MV, MOVBA_ADV_REJ_BOUNDS, MOVBA_ADV_LOST_CLAIM, MOVBA_ADV_FAR }) EXPECT(seen[fate] >= 20);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("advance driver: ok\n");
    return 0;
}
