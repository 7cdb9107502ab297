// Drives the HOST side of movba_lk_track (mov-slam_amd/csrc/lk.cpp) against the stand-in runtime and fake device of tests/hipstub
// and the fake launch of fake_lk.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or ThreadSanitizer.  The fake launch
// runs the library's own steps (whose values tests/test_lk_cpu.py holds to the restatement through lk_main.cpp); what is under
// test here is the host's side: every refusal of the header before anything is written (canaries), calls without frames, frames
// without points and without images, rows with padding behind them, pinned against ordinary result memory, calls of growing and
// shrinking size on one handle, a handle shared with an uploaded and a solved window whose downloads and runs go on around the
// calls, and two handles on two threads.  What comes back is checked against the same steps run over the driver's own layout -
// tight images, one buffer per frame - so a stride, an offset or a level table that the host got wrong shows.  Exit code 0 and
// the last line "lk driver: ok" = every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "lk.h"
#include "movba.h"

extern "C" int fake_lk_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr uint8_t kCanary = 0xEE;
constexpr int kOut = 7;

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
    std::vector<int32_t> rows, cols, stride, win, pt_ptr;
    std::vector<std::vector<uint8_t>> prev, next;       // rows x stride; empty for a frame without images
    std::vector<const uint8_t *> prev_p, next_p;
    std::vector<float> pt;
    Arr out[kOut];          // in the order of movba_lk_result's fields
    movba_lk_desc d{};
    movba_lk_result r{};
    size_t nf = 0, np = 0;
};

void bind(Call &s)
{
    s.nf = s.rows.size(); s.np = s.pt.size() / 2;
    const size_t n[kOut] = { 2 * s.np, s.np, s.np, s.np, s.np, s.nf + 1, s.np };
    const size_t elem[kOut] = { 4, 1, 4, 1, 1, 4, 4 };
    for (int k = 0; k < kOut; ++k) s.out[k].size(n[k], elem[k]);
    s.prev_p.clear(); s.next_p.clear();
    for (size_t f = 0; f < s.nf; ++f) {
        s.prev_p.push_back(s.prev[f].empty() ? nullptr : s.prev[f].data());
        s.next_p.push_back(s.next[f].empty() ? nullptr : s.next[f].data());
    }
    movba_lk_desc &d = s.d;
    d = movba_lk_desc{};
    d.n_frames = (int32_t)s.nf;
    d.prev_image = s.prev_p.data(); d.next_image = s.next_p.data();
    d.rows = s.rows.data(); d.cols = s.cols.data(); d.stride = s.stride.data(); d.win = s.win.data(); d.pt_ptr = s.pt_ptr.data(); d.pt = s.pt.data();
    d.max_level = 3; d.max_iter = 20; d.eps = 0.01; d.min_eig_threshold = 1e-4;
    movba_lk_result &r = s.r;
    r = movba_lk_result{};
    r.next_pt = s.out[0].as<float>(); r.pt_status = s.out[1].as<uint8_t>(); r.err = s.out[2].as<float>(); r.exit_code = s.out[3].as<uint8_t>();
    r.keep = s.out[4].as<uint8_t>(); r.kept_ptr = s.out[5].as<int32_t>(); r.kept_src = s.out[6].as<int32_t>();
    r.status = 99;
}

// nf frames of up to max_rows x max_cols with windows of 3 .. max_win that fit them (every fifth frame without points, every
// tenth of those without images), rows with up to 7 bytes of padding that differ between the two images, up to max_pt points
// that reach over every border; the next image is the previous one moved by a pixel, plus noise
void make_call(Call &s, int nf, int max_rows, int max_cols, int max_win, int max_pt, unsigned seed)
{
    std::mt19937 rng(seed);
    s = Call{};
    s.pt_ptr.assign(1, 0);
    for (int i = 0; i < nf; ++i) {
        const int lo = 4, rows = i == nf - 1 ? max_rows : lo + (int)(rng() % (unsigned)(max_rows - lo + 1)), cols = i == nf - 1 ? max_cols : lo + (int)(rng() % (unsigned)(max_cols - lo + 1));
        int win = 3 + 2 * (int)(rng() % (unsigned)((max_win - 3) / 2 + 1));
        while (win >= rows || win >= cols) win -= 2;
        const int stride = cols + (int)(rng() % 8u), np = i % 5 == 4 ? 0 : 1 + (int)(rng() % (unsigned)max_pt);
        s.rows.push_back(rows); s.cols.push_back(cols); s.stride.push_back(stride); s.win.push_back(win);
        std::vector<uint8_t> a, b;
        if (np || i % 10 != 9) {
            a.assign((size_t)rows * stride, 0); b.assign((size_t)rows * stride, 0);
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < stride; ++x) {
                    const int v = 128 + (int)(60 * std::sin(0.37 * x + 0.11 * y) + 50 * std::sin(0.23 * y - 0.19 * x)), w = 128 + (int)(60 * std::sin(0.37 * (x - 1) + 0.11 * y) + 50 * std::sin(0.23 * y - 0.19 * (x - 1)));
                    a[(size_t)y * stride + x] = x < cols ? (uint8_t)std::clamp(v + (int)(rng() % 7u), 0, 255) : (uint8_t)(rng() & 255u);
                    b[(size_t)y * stride + x] = x < cols ? (uint8_t)std::clamp(w + (int)(rng() % 7u), 0, 255) : (uint8_t)(rng() & 255u);
                }
        }
        s.prev.push_back(a); s.next.push_back(b);
        for (int k = 0; k < np; ++k) {
            s.pt.push_back((float)((int)(rng() % (unsigned)(4 * cols + 160)) - 80) * 0.25f); s.pt.push_back((float)((int)(rng() % (unsigned)(4 * rows + 160)) - 80) * 0.25f);
        }
        s.pt_ptr.push_back((int32_t)s.pt.size() / 2);
    }
    s.pt.reserve(1);        // (data() of an empty vector may be NULL, which the call refuses only where the counts need the array)
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

// what came back (pinned or not) against lk.h's steps over tight copies of each frame alone
void check(const Call &s, const movba_lk_result &r)
{
    using namespace movba;
    bool ok = true;
    int32_t kept = 0;
    for (size_t f = 0; f < s.nf; ++f) {
        const int32_t p0 = s.pt_ptr[f], n = s.pt_ptr[f + 1] - p0;
        ok &= r.kept_ptr[f] == kept;
        if (!n) continue;
        LkFrame fr;
        lk_frame_levels(s.rows[f], s.cols[f], s.win[f], s.d.max_level, &fr);
        size_t bytes = 0;
        for (int img = 0; img < 2; ++img)
            for (int l = 0; l <= fr.levels; ++l) { fr.off[img][l] = (int64_t)bytes; bytes += (size_t)fr.rows[l] * fr.cols[l]; }
        std::vector<uint8_t> pix(bytes);
        for (int y = 0; y < s.rows[f]; ++y) {
            std::memcpy(pix.data() + fr.off[0][0] + (size_t)y * s.cols[f], s.prev[f].data() + (size_t)y * s.stride[f], (size_t)s.cols[f]);
            std::memcpy(pix.data() + fr.off[1][0] + (size_t)y * s.cols[f], s.next[f].data() + (size_t)y * s.stride[f], (size_t)s.cols[f]);
        }
        std::vector<int32_t> lvl(2 * (kLkLevels - 1), 0), pt_ptr = { 0, n }, kept_cnt(1), kept_ptr(2), kept_src((size_t)n);
        std::vector<float> next_pt(2 * (size_t)n), err((size_t)n);
        std::vector<uint8_t> status((size_t)n), code((size_t)n), keep((size_t)n);
        LkDev d{};
        d.n_frames = 1; d.n_pt = n; d.max_iter = s.d.max_iter; d.eps_sq = s.d.eps * s.d.eps; d.min_eig = s.d.min_eig_threshold;
        for (int l = 1; l < kLkLevels; ++l) d.level_pixels[l - 1] = lvl[2 * (l - 1) + 1] = l <= fr.levels ? fr.rows[l] * fr.cols[l] : 0;
        d.frame = &fr; d.pt_ptr = pt_ptr.data(); d.lvl_ptr = lvl.data(); d.pt = s.pt.data() + 2 * (size_t)p0; d.pix = pix.data(); d.kept_cnt = kept_cnt.data();
        d.next_pt = next_pt.data(); d.err = err.data(); d.pt_status = status.data(); d.exit_code = code.data(); d.keep = keep.data();
        d.kept_ptr = kept_ptr.data(); d.kept_src = kept_src.data();
        lk_frames(d);
        ok &= std::memcmp(r.next_pt + 2 * (size_t)p0, next_pt.data(), 8 * (size_t)n) == 0 && std::memcmp(r.err + p0, err.data(), 4 * (size_t)n) == 0;
        ok &= std::memcmp(r.pt_status + p0, status.data(), (size_t)n) == 0 && std::memcmp(r.exit_code + p0, code.data(), (size_t)n) == 0 && std::memcmp(r.keep + p0, keep.data(), (size_t)n) == 0;
        for (int32_t k = 0; k < kept_ptr[1]; ++k) ok &= r.kept_src[kept + k] == kept_src[(size_t)k];
        kept += kept_ptr[1];
    }
    ok &= r.kept_ptr[s.nf] == kept;
    for (size_t i = (size_t)kept; i < s.np; ++i) ok &= r.kept_src[i] == -1;
    EXPECT(ok);
}

// variant 0: ordinary results; 1: then once more with all results pinned; 2: with the per-point results pinned and the rest
// ordinary (written a second time over the first call's arrays) - held to the ordinary result bit by bit
void run_call(movba_handle *h, int nf, int max_rows, int max_cols, int max_win, int max_pt, unsigned seed, int variant)
{
    Call s;
    make_call(s, nf, max_rows, max_cols, max_win, max_pt, seed);
    EXPECT(movba_lk_track(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    if (variant == 0) return;
    std::vector<void *> blocks;
    movba_lk_result r = s.r;
    void **field[kOut] = { (void **)&r.next_pt, (void **)&r.pt_status, (void **)&r.err, (void **)&r.exit_code, (void **)&r.keep, (void **)&r.kept_ptr, (void **)&r.kept_src };
    const int first = 0, last = variant == 1 ? kOut : 5;
    std::vector<std::vector<uint8_t>> before;
    for (int k = first; k < last; ++k) {
        void *p = movba_host_alloc(s.out[k].used ? s.out[k].used : 8);
        EXPECT(p != nullptr);
        if (!p) return;
        blocks.push_back(p);
        before.emplace_back(s.out[k].bytes.begin(), s.out[k].bytes.begin() + (long)s.out[k].used);
        *field[k] = p;
    }
    EXPECT(movba_lk_track(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK);
    check(s, r);
    for (int k = first; k < last; ++k) EXPECT(!s.out[k].used || std::memcmp(*field[k], before[(size_t)(k - first)].data(), s.out[k].used) == 0);
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_frames, most rows, most columns, largest window, most points of a frame
    const int rounds[][5] = { { 3, 30, 40, 9, 9 }, { 12, 70, 90, 31, 30 }, { 1, 4, 4, 3, 3 }, { 2, 120, 200, 21, 60 }, { 40, 24, 28, 7, 6 },
                              { 5, 18, 18, 5, 1 }, { 64, 20, 33, 11, 3 }, { 4, 257, 19, 15, 20 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], q[3], q[4], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 39; ++which) {
        Call s;
        make_call(s, 6, 40, 50, 9, 20, 4u);
        EXPECT(s.pt_ptr[1] > 0 && s.pt_ptr[2] > s.pt_ptr[1] && s.np > 8);          // (the cases below count on these)
        movba_lk_desc &d = s.d;
        movba_lk_result &r = s.r;
        switch (which) {
        case 0: d.n_frames = -1; break;
        case 1: d.n_frames = MOVBA_MAX_EXPRESS_IMAGES + 1; break;
        case 2: d.pt_ptr = nullptr; break;
        case 3: s.pt_ptr[0] = 1; break;
        case 4: s.pt_ptr[3] = s.pt_ptr[2] - 1; break;
        case 5: d.prev_image = nullptr; break;
        case 6: d.next_image = nullptr; break;
        case 7: d.rows = nullptr; break;
        case 8: d.cols = nullptr; break;
        case 9: d.stride = nullptr; break;
        case 10: d.win = nullptr; break;
        case 11: d.pt = nullptr; break;
        case 12: r.next_pt = nullptr; break;
        case 13: r.pt_status = nullptr; break;
        case 14: r.err = nullptr; break;
        case 15: r.exit_code = nullptr; break;
        case 16: r.keep = nullptr; break;
        case 17: r.kept_ptr = nullptr; break;
        case 18: r.kept_src = nullptr; break;
        case 19: s.prev_p[0] = nullptr; break;
        case 20: s.next_p[1] = nullptr; break;
        case 21: s.win[0] = 4; break;
        case 22: s.win[1] = 1; break;
        case 23: s.win[2] = 33; break;
        case 24: s.rows[0] = s.win[0]; break;
        case 25: s.cols[1] = s.win[1]; break;
        case 26: s.stride[0] = s.cols[0] - 1; break;
        case 27: d.max_level = -1; break;
        case 28: d.max_level = 4; break;
        case 29: d.max_iter = 0; break;
        case 30: d.max_iter = 31; break;
        case 31: d.eps = 0.0; break;
        case 32: d.eps = NAN; break;
        case 33: d.eps = 10.5; break;
        case 34: d.min_eig_threshold = -1.0; break;
        case 35: d.min_eig_threshold = INFINITY; break;
        case 36: s.pt[1] = NAN; break;
        case 37: s.pt[0] = 1048577.0f; break;
        case 38: for (size_t i = 1; i < s.pt_ptr.size(); ++i) s.pt_ptr[i] = MOVBA_MAX_EXPRESS_ITEMS + 1; break;    // nothing behind it is read
        }
        const int rc = movba_lk_track(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    {   // more pixels than the bound: 1024 frames of 257 x 256 (the images are never read)
        Call s;
        make_call(s, 2, 12, 12, 5, 3, 6u);
        std::vector<int32_t> rows(1024, 257), cols(1024, 256), stride(1024, 256), win(1024, 5), ptr(1025, 0);
        std::vector<const uint8_t *> img(1024, nullptr);
        s.d.n_frames = 1024; s.d.rows = rows.data(); s.d.cols = cols.data(); s.d.stride = stride.data(); s.d.win = win.data(); s.d.pt_ptr = ptr.data();
        s.d.prev_image = img.data(); s.d.next_image = img.data();
        EXPECT(movba_lk_track(h, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == MOVBA_ERR_ARG && untouched(s));
    }
    Call s;
    make_call(s, 5, 30, 44, 7, 9, 5u);
    EXPECT(movba_lk_track(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_lk_track(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_lk_track(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    EXPECT(movba_lk_track(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    // no frames: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    Call e;
    make_call(e, 4, 20, 20, 5, 3, 8u);
    e.d.n_frames = 0; e.d.pt_ptr = nullptr; e.r.kept_ptr = nullptr;
    EXPECT(movba_lk_track(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
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
        run_call(h, 8, 40, 50, 9, 8, seed + 1, rep % 3);                            // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, 31, 30, 36, 7, 5, seed + 2, (rep + 1) % 3);                     // solved, not downloaded
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        const std::vector<double> first = w.out_poses;
        run_call(h, 3, 100, 130, 21, 30, seed + 3, (rep + 2) % 3);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        run_call(h, 4, 50, 50, 11, 10, seed + 4, 0);
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
        auto lk_thread = [](unsigned seed) {
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
        std::thread a(lk_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_lk_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("lk driver: ok\n");
    return 0;
}
