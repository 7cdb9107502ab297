// Drives the HOST side of movba_mv_raster (mov-slam_amd/csrc/mv_raster.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_mv_raster.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or
// ThreadSanitizer.  The fake launch runs the library's own steps (whose values tests/test_mv_raster_cpu.py holds to the
// restatement through mvr_main.cpp); what is under test here is the host's side: every refusal of the header before anything is
// written (canaries), calls without frames, frames without records or without queries, pinned against ordinary result memory,
// calls of growing and shrinking size on one handle, a handle shared with an uploaded and a solved window whose downloads and
// runs go on around the calls, and two handles on two threads.  What comes back is checked against a painted image: the driver
// paints the four slots per pixel as the reference does and gathers.  Exit code 0 and the last line "mv_raster driver: ok" =
// every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_mv_raster_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr uint8_t kCanary = 0xEE;
constexpr int kOut = 11;

int lattice_nx(int n) { return n <= 16 ? 0 : (n - 17) / 16 + 1; }
int lattice(int rows, int cols) { return lattice_nx(rows) * lattice_nx(cols); }

// one result array of the caller with a canary element behind its end
struct Arr {
    std::vector<uint8_t> bytes;
    size_t used = 0;
    void size(size_t n, size_t elem) { used = n * elem; bytes.assign(used + elem, kCanary); }
    template <typename T> T *as() { return reinterpret_cast<T *>(bytes.data()); }
    bool untouched() const { return std::all_of(bytes.begin(), bytes.end(), [](uint8_t v) { return v == kCanary; }); }
    bool canary() const { return std::all_of(bytes.begin() + (long)used, bytes.end(), [](uint8_t v) { return v == kCanary; }); }
};

struct Call {
    std::vector<int32_t> rows, cols, rec_ptr, q_ptr, source, ref;
    std::vector<double> threshold;
    std::vector<uint8_t> want, w, h;
    std::vector<int16_t> sx, sy, dx, dy;
    std::vector<float> q_pt;
    Arr out[kOut];          // in the order of movba_mv_raster_result's fields
    movba_mv_raster_desc d{};
    movba_mv_raster_result r{};
    size_t nf = 0, nr = 0, nq = 0, ng = 0;
};

void bind(Call &s)
{
    s.nf = s.rows.size(); s.nr = s.w.size(); s.nq = s.q_pt.size() / 2; s.ng = 0;
    for (size_t f = 0; f < s.nf; ++f) s.ng += (size_t)lattice(s.rows[f], s.cols[f]);
    const size_t n[kOut] = { s.nf + 1, 4 * s.nr, 2 * s.nr, s.nr, s.nr, 4 * s.nq, s.nf + 1, s.ng, s.nf, s.nf, s.nf };
    const size_t elem[kOut] = { 4, 4, 4, 4, 4, 4, 4, 1, 4, 8, 1 };
    for (int k = 0; k < kOut; ++k) s.out[k].size(n[k], elem[k]);
    movba_mv_raster_desc &d = s.d;
    d = movba_mv_raster_desc{};
    d.n_frames = (int32_t)s.nf;
    d.rows = s.rows.data(); d.cols = s.cols.data(); d.coverage_threshold = s.threshold.data(); d.want_grid = s.want.data(); d.rec_ptr = s.rec_ptr.data();
    d.src_x = s.sx.data(); d.src_y = s.sy.data(); d.dst_x = s.dx.data(); d.dst_y = s.dy.data(); d.w = s.w.data(); d.h = s.h.data();
    d.source = s.source.data(); d.ref = s.ref.data(); d.q_ptr = s.q_ptr.data(); d.q_pt = s.q_pt.data();
    movba_mv_raster_result &r = s.r;
    r = movba_mv_raster_result{};
    r.kept_ptr = s.out[0].as<int32_t>(); r.kp_rect = s.out[1].as<int32_t>(); r.mv_pt = s.out[2].as<float>(); r.mv_dindx = s.out[3].as<int32_t>();
    r.rec_kept = s.out[4].as<int32_t>(); r.cand = s.out[5].as<int32_t>(); r.grid_ptr = s.out[6].as<int32_t>(); r.grid_covered = s.out[7].as<uint8_t>();
    r.cover_px = s.out[8].as<int32_t>(); r.coverage_area = s.out[9].as<double>(); r.force_grid = s.out[10].as<uint8_t>();
    r.status = 99;
}

// nf frames of up to max_rows x max_cols (every fifth without records, every seventh without queries), up to max_rec records
// whose sources and destinations reach over every border, up to max_q queries that reach over it too
void make_call(Call &s, int nf, int max_rows, int max_cols, int max_rec, int max_q, unsigned seed)
{
    std::mt19937 rng(seed);
    s = Call{};
    s.rec_ptr.assign(1, 0); s.q_ptr.assign(1, 0);
    for (int i = 0; i < nf; ++i) {
        const int rows = i == nf - 1 ? max_rows : 1 + (int)(rng() % (unsigned)max_rows), cols = i == nf - 1 ? max_cols : 1 + (int)(rng() % (unsigned)max_cols);
        s.rows.push_back(rows); s.cols.push_back(cols);
        s.threshold.push_back(i % 3 == 0 ? 0.0 : (double)(rng() % 400) / 100.0);
        s.want.push_back((uint8_t)(i % 2 ? 5 : 0));
        const int nr = i % 5 == 4 ? 0 : (int)(rng() % (unsigned)(max_rec + 1)), nq = i % 7 == 6 ? 0 : (int)(rng() % (unsigned)(max_q + 1));
        for (int k = 0; k < nr; ++k) {
            s.sx.push_back((int16_t)((int)(rng() % (unsigned)(cols + 48)) - 24)); s.sy.push_back((int16_t)((int)(rng() % (unsigned)(rows + 48)) - 24));
            s.dx.push_back((int16_t)((int)(rng() % (unsigned)(cols + 12)) - 6)); s.dy.push_back((int16_t)((int)(rng() % (unsigned)(rows + 12)) - 6));
            s.w.push_back((uint8_t)(4 << (rng() % 3))); s.h.push_back((uint8_t)(4 << (rng() % 3)));
            s.source.push_back(-1 - (int32_t)(rng() % 3)); s.ref.push_back(0);
        }
        for (int k = 0; k < nq; ++k) {
            s.q_pt.push_back((float)((int)(rng() % (unsigned)(4 * cols + 24)) - 12) * 0.25f); s.q_pt.push_back((float)((int)(rng() % (unsigned)(4 * rows + 24)) - 12) * 0.25f);
        }
        s.rec_ptr.push_back((int32_t)s.w.size()); s.q_ptr.push_back((int32_t)s.q_pt.size() / 2);
    }
    // (data() of an empty vector may be NULL, which the call refuses only where the counts need the array)
    s.sx.reserve(1); s.sy.reserve(1); s.dx.reserve(1); s.dy.reserve(1); s.w.reserve(1); s.h.reserve(1); s.source.reserve(1); s.ref.reserve(1); s.q_pt.reserve(1);
    bind(s);
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

// what came back (pinned or not) against an image painted as the reference paints it
void check(const Call &s, const movba_mv_raster_result &r)
{
    bool ok = true;
    int32_t at = 0, g_at = 0;
    for (size_t f = 0; f < s.nf; ++f) {
        const int W = s.cols[f], H = s.rows[f];
        std::vector<int32_t> mvi((size_t)W * H * 4, -1);
        int32_t m = 0, cover = 0;
        ok &= r.kept_ptr[f] == at && r.grid_ptr[f] == g_at;
        for (int32_t i = s.rec_ptr[f]; i < s.rec_ptr[f + 1]; ++i) {
            const int hx = s.w[i] / 2, hy = s.h[i] / 2;
            if (s.dx[i] + hx >= W || s.dy[i] + hy >= H) { ok &= r.rec_kept[i] == -1; continue; }
            const size_t o = (size_t)(at + m);
            ok &= r.rec_kept[i] == m && r.mv_dindx[o] == m;
            ok &= r.kp_rect[4 * o] == std::max(s.dx[i] - hx, 0) && r.kp_rect[4 * o + 1] == std::max(s.dy[i] - hy, 0) && r.kp_rect[4 * o + 2] == s.w[i] && r.kp_rect[4 * o + 3] == s.h[i];
            ok &= r.mv_pt[2 * o] == (float)(s.dx[i] - s.sx[i]) && r.mv_pt[2 * o + 1] == (float)(s.dy[i] - s.sy[i]);
            for (int y = std::max(s.sy[i] - hy, 0); y <= std::min(s.sy[i] + hy, H - 1); ++y)
                for (int x = std::max(s.sx[i] - hx, 0); x <= std::min(s.sx[i] + hx, W - 1); ++x) {
                    int32_t *v = &mvi[4 * ((size_t)y * W + x)];
                    if (v[0] == -1) v[0] = m; else if (v[1] == -1) v[1] = m; else if (v[2] == -1) v[2] = m; else v[3] = m;
                }
            cover += s.w[i] * s.h[i];
            ++m;
        }
        at += m;
        const double area = (double)cover / (double)(W * H);
        ok &= r.cover_px[f] == cover && r.coverage_area[f] == area && r.force_grid[f] == (area < s.threshold[f] ? 1 : 0);
        for (int32_t q = s.q_ptr[f]; q < s.q_ptr[f + 1]; ++q) {
            const int x = (int)s.q_pt[2 * q], y = (int)s.q_pt[2 * q + 1];
            const bool inside = x >= 0 && y >= 0 && x < W && y < H;
            for (int c = 0; c < 4; ++c) ok &= r.cand[4 * q + c] == (inside ? mvi[4 * ((size_t)y * W + x) + c] : -1);
        }
        const int nx = lattice_nx(W), ng = lattice(H, W);
        for (int g = 0; g < ng; ++g) {
            const int x = (g % nx) * 16 + 8, y = (g / nx) * 16 + 8;
            ok &= r.grid_covered[g_at + g] == (s.want[f] && mvi[4 * ((size_t)y * W + x)] >= 0 ? 1 : 0);
        }
        g_at += ng;
    }
    ok &= r.kept_ptr[s.nf] == at && r.grid_ptr[s.nf] == g_at;
    for (size_t o = (size_t)at; o < s.nr; ++o) {
        ok &= r.mv_dindx[o] == -1 && std::isnan(r.mv_pt[2 * o]) && std::isnan(r.mv_pt[2 * o + 1]);
        for (int q = 0; q < 4; ++q) ok &= r.kp_rect[4 * o + q] == -1;
    }
    EXPECT(ok);
}

// variant 0: ordinary results; 1: then once more with all results pinned; 2: with the per-record results pinned and the rest
// ordinary (written a second time over the first call's arrays) - held to the ordinary result bit by bit
void run_call(movba_handle *h, int nf, int max_rows, int max_cols, int max_rec, int max_q, unsigned seed, int variant)
{
    Call s;
    make_call(s, nf, max_rows, max_cols, max_rec, max_q, seed);
    EXPECT(movba_mv_raster(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    if (variant == 0) return;
    std::vector<void *> blocks;
    movba_mv_raster_result r = s.r;
    void **field[kOut] = { (void **)&r.kept_ptr, (void **)&r.kp_rect, (void **)&r.mv_pt, (void **)&r.mv_dindx, (void **)&r.rec_kept, (void **)&r.cand,
                           (void **)&r.grid_ptr, (void **)&r.grid_covered, (void **)&r.cover_px, (void **)&r.coverage_area, (void **)&r.force_grid };
    const int first = variant == 1 ? 0 : 1, last = variant == 1 ? kOut : 5;
    std::vector<std::vector<uint8_t>> before;
    for (int k = first; k < last; ++k) {
        void *p = movba_host_alloc(s.out[k].used ? s.out[k].used : 8);
        EXPECT(p != nullptr);
        if (!p) return;
        blocks.push_back(p);
        before.emplace_back(s.out[k].bytes.begin(), s.out[k].bytes.begin() + (long)s.out[k].used);
        *field[k] = p;
    }
    EXPECT(movba_mv_raster(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK);
    check(s, r);
    for (int k = first; k < last; ++k) EXPECT(!s.out[k].used || std::memcmp(*field[k], before[(size_t)(k - first)].data(), s.out[k].used) == 0);
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_frames, most rows, most columns, most records, most queries of a frame
    const int rounds[][5] = { { 3, 30, 40, 20, 9 }, { 12, 120, 200, 900, 300 }, { 1, 1, 1, 3, 3 }, { 2, 270, 480, 6000, 2000 }, { 40, 64, 48, 60, 30 },
                              { 5, 18, 18, 0, 7 }, { 64, 90, 33, 70, 0 }, { 4, 257, 19, 300, 40 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], q[3], q[4], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 43; ++which) {
        Call s;
        make_call(s, 6, 40, 50, 30, 20, 4u);
        EXPECT(s.rec_ptr[1] > 1 && s.q_ptr[1] > 1 && s.nr > 8 && s.nq > 8);       // (the cases below count on these)
        movba_mv_raster_desc &d = s.d;
        movba_mv_raster_result &r = s.r;
        switch (which) {
        case 0: d.n_frames = -1; break;
        case 1: d.n_frames = MOVBA_MAX_EXPRESS_IMAGES + 1; break;
        case 2: d.rec_ptr = nullptr; break;
        case 3: d.q_ptr = nullptr; break;
        case 4: s.rec_ptr[0] = 1; break;
        case 5: s.rec_ptr[3] = s.rec_ptr[2] - 1; break;
        case 6: s.q_ptr[0] = -1; break;
        case 7: s.q_ptr[2] = s.q_ptr[1] - 1; break;
        case 8: d.rows = nullptr; break;
        case 9: d.cols = nullptr; break;
        case 10: d.coverage_threshold = nullptr; break;
        case 11: d.want_grid = nullptr; break;
        case 12: d.src_x = nullptr; break;
        case 13: d.src_y = nullptr; break;
        case 14: d.dst_x = nullptr; break;
        case 15: d.dst_y = nullptr; break;
        case 16: d.w = nullptr; break;
        case 17: d.h = nullptr; break;
        case 18: d.source = nullptr; break;
        case 19: d.ref = nullptr; break;
        case 20: d.q_pt = nullptr; break;
        case 21: r.kept_ptr = nullptr; break;
        case 22: r.kp_rect = nullptr; break;
        case 23: r.mv_pt = nullptr; break;
        case 24: r.mv_dindx = nullptr; break;
        case 25: r.rec_kept = nullptr; break;
        case 26: r.cand = nullptr; break;
        case 27: r.grid_ptr = nullptr; break;
        case 28: r.grid_covered = nullptr; break;
        case 29: r.cover_px = nullptr; break;
        case 30: r.coverage_area = nullptr; break;
        case 31: r.force_grid = nullptr; break;
        case 32: s.rows[2] = 0; break;
        case 33: s.cols[1] = 32768; break;
        case 34: s.w[1] = 12; break;
        case 35: s.h[0] = 32; break;
        case 36: s.w[2] = 0; break;
        case 37: s.ref[1] = 1; break;
        case 38: s.source[0] = 0; break;
        case 39: s.q_pt[1] = NAN; break;
        case 40: s.q_pt[0] = 1048577.0f; break;
        case 41: s.threshold[1] = INFINITY; break;
        case 42: for (size_t i = 1; i < s.rec_ptr.size(); ++i) s.rec_ptr[i] = (1 << 20) + 1; break;     // nothing behind it is read
        }
        const int rc = movba_mv_raster(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, 5, 30, 44, 12, 9, 5u);
    EXPECT(movba_mv_raster(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_mv_raster(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_mv_raster(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    EXPECT(movba_mv_raster(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    // no frames: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    Call e;
    make_call(e, 4, 20, 20, 3, 3, 8u);
    e.d.n_frames = 0; e.d.rec_ptr = nullptr; e.r.kept_ptr = nullptr;
    EXPECT(movba_mv_raster(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
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
        auto mvr_thread = [](unsigned seed) {
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
        std::thread a(mvr_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_mv_raster_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("mv_raster driver: ok\n");
    return 0;
}
