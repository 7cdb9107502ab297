// Drives the HOST side of movba_stereo_points (mov-slam_amd/csrc/stereo_points.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_stereo_points.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or
// ThreadSanitizer.  The fake launch runs the library's own steps (whose values tests/test_stereo_points_cpu.py holds to the
// restatement through stereo_main.cpp); what is under test here is the host's side: every refusal of the header before anything
// is written (canaries), calls without frames, frames without points, optional arrays present and absent, pinned against
// ordinary result memory, calls of growing and shrinking size on one handle, a handle shared with an uploaded and a solved window
// whose downloads and runs go on around the calls, and two handles on two threads.  What comes back is checked against the same
// steps run over the driver's own layout - one frame at a time, each alone - so an offset or a frame table that the host got
// wrong shows.  Exit code 0 and the last line "stereo driver: ok" = every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"
#include "stereo_points.h"

extern "C" int fake_stereo_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr uint8_t kCanary = 0xEE;
constexpr int kOut = 11;

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
    std::vector<int32_t> rows, cols, select, pt_ptr;
    std::vector<float> bf, max_disparity, th_depth, cam, pt, next_pt, pt_un;
    std::vector<uint8_t> status, has;
    std::vector<double> poses;
    bool with_un = false, with_poses = false, with_has = false;
    Arr out[kOut];          // in the order of movba_stereo_result's fields
    movba_stereo_desc d{};
    movba_stereo_result r{};
    size_t nf = 0, np = 0;
};

void bind(Call &s)
{
    s.nf = s.rows.size(); s.np = s.pt.size() / 2;
    const size_t n[kOut] = { s.np, s.np, s.np, s.nf, s.nf, s.nf, s.nf + 1, s.np, s.np, 3 * s.np, 3 * s.np };
    const size_t elem[kOut] = { 4, 4, 1, 4, 4, 4, 4, 4, 1, 4, 8 };
    for (int k = 0; k < kOut; ++k) s.out[k].size(n[k], elem[k]);
    movba_stereo_desc &d = s.d;
    d = movba_stereo_desc{};
    d.n_frames = (int32_t)s.nf;
    d.pt_ptr = s.pt_ptr.data(); d.pt = s.pt.data(); d.next_pt = s.next_pt.data(); d.pt_status = s.status.data();
    d.pt_un = s.with_un ? s.pt_un.data() : nullptr;
    d.rows = s.rows.data(); d.cols = s.cols.data(); d.bf = s.bf.data(); d.max_disparity = s.max_disparity.data(); d.th_depth = s.th_depth.data();
    d.cam = s.cam.data(); d.select = s.select.data();
    d.poses = s.with_poses ? s.poses.data() : nullptr;
    d.has_point = s.with_has ? s.has.data() : nullptr;
    d.max_row_diff = 4.f; d.min_disparity = 0.f; d.max_point = 100;
    movba_stereo_result &r = s.r;
    r = movba_stereo_result{};
    r.u_right = s.out[0].as<float>(); r.depth = s.out[1].as<float>(); r.code = s.out[2].as<uint8_t>(); r.n_stereo = s.out[3].as<int32_t>();
    r.median_dist = s.out[4].as<int32_t>(); r.th_dist = s.out[5].as<float>(); r.sel_ptr = s.out[6].as<int32_t>(); r.sel_src = s.out[7].as<int32_t>();
    r.sel_new = s.out[8].as<uint8_t>(); r.sel_cam = s.out[9].as<float>(); r.sel_point = s.out[10].as<double>();
    r.status = 99;
}

// nf frames of up to max_pt points (every fifth frame without points): disparities up to 40 pixels, a row noise that sometimes
// passes the gate, lost tracks with NaNs in their next_pt, the three kinds of selection; `optional` bit 0: pt_un, 1: poses, 2: has_point
void make_call(Call &s, int nf, int max_pt, unsigned seed, int optional)
{
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u01(0.f, 1.f);
    s = Call{};
    s.with_un = optional & 1; s.with_poses = optional & 2; s.with_has = optional & 4;
    s.pt_ptr.assign(1, 0);
    for (int i = 0; i < nf; ++i) {
        const int rows = 100 + (int)(rng() % 400u), cols = 120 + (int)(rng() % 500u), np = i % 5 == 4 ? 0 : (i == nf - 1 ? max_pt : 1 + (int)(rng() % (unsigned)max_pt));
        s.rows.push_back(rows); s.cols.push_back(cols); s.select.push_back((int32_t)(rng() % 3u));
        s.bf.push_back(20.f + 40.f * u01(rng)); s.max_disparity.push_back(25.f + 30.f * u01(rng)); s.th_depth.push_back(1.f + 4.f * u01(rng));
        s.cam.push_back(300.f + 200.f * u01(rng)); s.cam.push_back(300.f + 200.f * u01(rng)); s.cam.push_back(0.5f * cols); s.cam.push_back(0.5f * rows);
        const double q[7] = { u01(rng) - 0.5, u01(rng) - 0.5, u01(rng) - 0.5, 0.5 + u01(rng), 100.0 * u01(rng), -50.0 * u01(rng), 3.0 * u01(rng) };
        s.poses.insert(s.poses.end(), q, q + 7);
        for (int k = 0; k < np; ++k) {
            const float x = cols * u01(rng), y = rows * u01(rng), disparity = 40.f * u01(rng) - 1.f, dy = 5.f * (u01(rng) - 0.5f) * (k % 7 == 0 ? 3.f : 1.f);
            const bool lost = rng() % 9u == 0;
            s.pt.push_back(x); s.pt.push_back(y);
            s.next_pt.push_back(lost && k % 2 ? NAN : x - disparity); s.next_pt.push_back(lost && k % 2 ? INFINITY : y + dy);
            s.status.push_back(lost ? 0 : 1);
            s.pt_un.push_back(x + u01(rng) - 0.5f); s.pt_un.push_back(y + u01(rng) - 0.5f);
            s.has.push_back(rng() % 3u == 0);
        }
        s.pt_ptr.push_back((int32_t)s.pt.size() / 2);
    }
    for (auto *v : { &s.pt, &s.next_pt, &s.pt_un }) v->reserve(1);     // (data() of an empty vector may be NULL, which the call refuses only where the counts need the array)
    s.status.reserve(1); s.has.reserve(1);
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

// what came back (pinned or not) against stereo_points.h's steps over each frame alone
void check(const Call &s, const movba_stereo_result &r)
{
    using namespace movba;
    bool ok = true;
    int32_t sel = 0;
    for (size_t f = 0; f < s.nf; ++f) {
        const int32_t p0 = s.pt_ptr[f], n = s.pt_ptr[f + 1] - p0;
        ok &= r.sel_ptr[f] == sel;
        StFrame fr{};
        fr.rows = s.rows[f]; fr.cols = s.cols[f]; fr.select = s.select[f]; fr.bf = s.bf[f]; fr.max_disparity = s.max_disparity[f]; fr.th_depth = s.th_depth[f];
        fr.fx = s.cam[4 * f]; fr.fy = s.cam[4 * f + 1]; fr.cx = s.cam[4 * f + 2]; fr.cy = s.cam[4 * f + 3];
        st_frame_pose(s.with_poses ? s.poses.data() + 7 * f : nullptr, &fr);
        const size_t m = (size_t)n;
        std::vector<int32_t> pt_ptr = { 0, n }, dist(m), list(m), counts(1), n_stereo(1), median(1), sel_ptr(2), sel_src(m);
        std::vector<float> z(m), ur(m), depth(m), th(1), cam(3 * m);
        std::vector<uint8_t> code(m), sel_new(m);
        std::vector<double> point(3 * m);
        StDev d{};
        d.n_frames = 1; d.n_pt = n; d.max_point = s.d.max_point; d.max_row_diff = s.d.max_row_diff; d.min_disparity = s.d.min_disparity;
        d.max_close = fr.select == MOVBA_STEREO_SELECT_CLOSE ? n : 0;
        d.frame = &fr; d.pt_ptr = pt_ptr.data(); d.pt = s.pt.data() + 2 * (size_t)p0; d.next_pt = s.next_pt.data() + 2 * (size_t)p0;
        d.pt_un = s.with_un ? s.pt_un.data() + 2 * (size_t)p0 : d.pt;
        d.pt_status = s.status.data() + p0; d.has_point = s.with_has ? s.has.data() + p0 : nullptr;
        d.dist = dist.data(); d.z = z.data(); d.list = list.data(); d.counts = counts.data();
        d.u_right = ur.data(); d.depth = depth.data(); d.code = code.data(); d.n_stereo = n_stereo.data(); d.median_dist = median.data(); d.th_dist = th.data();
        d.sel_ptr = sel_ptr.data(); d.sel_src = sel_src.data(); d.sel_new = sel_new.data(); d.sel_cam = cam.data(); d.sel_point = point.data();
        st_frames(d);
        ok &= !m || (std::memcmp(r.u_right + p0, ur.data(), 4 * m) == 0 && std::memcmp(r.depth + p0, depth.data(), 4 * m) == 0 && std::memcmp(r.code + p0, code.data(), m) == 0);
        ok &= r.n_stereo[f] == n_stereo[0] && r.median_dist[f] == median[0] && std::memcmp(r.th_dist + f, th.data(), 4) == 0;
        const size_t k = (size_t)sel_ptr[1];
        ok &= !k || (std::memcmp(r.sel_src + sel, sel_src.data(), 4 * k) == 0 && std::memcmp(r.sel_new + sel, sel_new.data(), k) == 0 &&
                     std::memcmp(r.sel_cam + 3 * (size_t)sel, cam.data(), 12 * k) == 0 && std::memcmp(r.sel_point + 3 * (size_t)sel, point.data(), 24 * k) == 0);
        sel += sel_ptr[1];
    }
    ok &= r.sel_ptr[s.nf] == sel;
    for (size_t i = (size_t)sel; i < s.np; ++i) ok &= r.sel_src[i] == -1 && r.sel_new[i] == 0 && std::isnan(r.sel_cam[3 * i]) && std::isnan(r.sel_point[3 * i + 2]);
    EXPECT(ok);
}

// variant 0: ordinary results; 1: then once more with all results pinned; 2: with the per-point results pinned and the rest
// ordinary (written a second time over the first call's arrays) - held to the ordinary result bit by bit
void run_call(movba_handle *h, int nf, int max_pt, unsigned seed, int variant)
{
    Call s;
    make_call(s, nf, max_pt, seed, (int)(seed % 8u));
    EXPECT(movba_stereo_points(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    if (variant == 0) return;
    std::vector<void *> blocks;
    movba_stereo_result r = s.r;
    void **field[kOut] = { (void **)&r.u_right, (void **)&r.depth, (void **)&r.code, (void **)&r.n_stereo, (void **)&r.median_dist, (void **)&r.th_dist,
                           (void **)&r.sel_ptr, (void **)&r.sel_src, (void **)&r.sel_new, (void **)&r.sel_cam, (void **)&r.sel_point };
    const int first = 0, last = variant == 1 ? kOut : 3;
    std::vector<std::vector<uint8_t>> before;
    for (int k = first; k < last; ++k) {
        void *p = movba_host_alloc(s.out[k].used ? s.out[k].used : 8);
        EXPECT(p != nullptr);
        if (!p) return;
        blocks.push_back(p);
        before.emplace_back(s.out[k].bytes.begin(), s.out[k].bytes.begin() + (long)s.out[k].used);
        *field[k] = p;
    }
    EXPECT(movba_stereo_points(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK);
    check(s, r);
    for (int k = first; k < last; ++k) EXPECT(!s.out[k].used || std::memcmp(*field[k], before[(size_t)(k - first)].data(), s.out[k].used) == 0);
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_frames, most points of a frame
    const int rounds[][2] = { { 3, 9 }, { 12, 300 }, { 1, 1 }, { 2, 5000 }, { 40, 6 }, { 5, 1 }, { 64, 30 }, { 4, 16384 }, { 200, 3 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 52; ++which) {
        Call s;
        make_call(s, 6, 20, 4u, 7);
        EXPECT(s.pt_ptr[1] > 0 && s.pt_ptr[2] > s.pt_ptr[1] && s.np > 8);          // (the cases below count on these)
        movba_stereo_desc &d = s.d;
        movba_stereo_result &r = s.r;
        s.status[0] = 1; s.status[1] = 0;
        switch (which) {
        case 0: d.n_frames = -1; break;
        case 1: d.n_frames = MOVBA_MAX_EXPRESS_IMAGES + 1; break;
        case 2: d.pt_ptr = nullptr; break;
        case 3: s.pt_ptr[0] = 1; break;
        case 4: s.pt_ptr[3] = s.pt_ptr[2] - 1; break;
        case 5: d.pt = nullptr; break;
        case 6: d.next_pt = nullptr; break;
        case 7: d.pt_status = nullptr; break;
        case 8: d.rows = nullptr; break;
        case 9: d.cols = nullptr; break;
        case 10: d.bf = nullptr; break;
        case 11: d.max_disparity = nullptr; break;
        case 12: d.th_depth = nullptr; break;
        case 13: d.cam = nullptr; break;
        case 14: d.select = nullptr; break;
        case 15: r.u_right = nullptr; break;
        case 16: r.depth = nullptr; break;
        case 17: r.code = nullptr; break;
        case 18: r.n_stereo = nullptr; break;
        case 19: r.median_dist = nullptr; break;
        case 20: r.th_dist = nullptr; break;
        case 21: r.sel_ptr = nullptr; break;
        case 22: r.sel_src = nullptr; break;
        case 23: r.sel_new = nullptr; break;
        case 24: r.sel_cam = nullptr; break;
        case 25: r.sel_point = nullptr; break;
        case 26: s.rows[0] = 0; break;
        case 27: s.cols[1] = -3; break;
        case 28: s.select[2] = 3; break;
        case 29: s.select[0] = -1; break;
        case 30: d.max_point = -1; break;
        case 31: s.bf[1] = 0.f; break;
        case 32: s.bf[0] = NAN; break;
        case 33: s.max_disparity[2] = INFINITY; break;
        case 34: s.th_depth[0] = NAN; break;
        case 35: s.cam[0] = 0.f; break;
        case 36: s.cam[5] = -1.f; break;
        case 37: s.cam[2] = NAN; break;
        case 38: d.max_row_diff = NAN; break;
        case 39: d.min_disparity = -INFINITY; break;
        case 40: s.pt[1] = NAN; break;
        case 41: s.pt[0] = 1048577.0f; break;
        case 42: s.pt_un[3] = INFINITY; break;
        case 43: s.pt_un[2] = -1048577.0f; break;
        case 44: s.next_pt[0] = NAN; break;                  // (point 0 has status 1)
        case 45: s.next_pt[1] = 1048577.0f; break;
        case 46: s.poses[3] = NAN; break;
        case 47: s.poses[7 + 5] = INFINITY; break;
        case 48: s.poses[14] = s.poses[15] = s.poses[16] = s.poses[17] = 0.0; break;
        case 49: for (size_t i = 1; i < s.pt_ptr.size(); ++i) s.pt_ptr[i] = MOVBA_MAX_EXPRESS_ITEMS + 1; break;    // nothing behind it is read
        case 50: for (size_t i = 1; i < s.pt_ptr.size(); ++i) s.pt_ptr[i] = MOVBA_MAX_STEREO_POINTS + 1; break;
        case 51: s.pt_ptr[0] = -2; break;
        }
        const int rc = movba_stereo_points(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    {   // a next_pt that is not finite is the caller's business where pt_status is 0
        Call s;
        make_call(s, 6, 20, 4u, 7);
        s.status[1] = 0; s.next_pt[2] = NAN; s.next_pt[3] = -INFINITY;
        EXPECT(movba_stereo_points(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK && s.r.code[1] == MOVBA_STEREO_REJ_STATUS);
        check(s, s.r);
    }
    Call s;
    make_call(s, 5, 9, 5u, 3);
    EXPECT(movba_stereo_points(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_stereo_points(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_stereo_points(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    EXPECT(movba_stereo_points(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    // no frames: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    Call e;
    make_call(e, 4, 3, 8u, 0);
    e.d.n_frames = 0; e.d.pt_ptr = nullptr; e.r.sel_ptr = nullptr;
    EXPECT(movba_stereo_points(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
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
        run_call(h, 8, 80, seed + 1, rep % 3);                                      // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, 31, 50, seed + 2, (rep + 1) % 3);                               // solved, not downloaded
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        const std::vector<double> first = w.out_poses;
        run_call(h, 3, 3000, seed + 3, (rep + 2) % 3);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        run_call(h, 4, 100, seed + 4, 0);
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
        auto st_thread = [](unsigned seed) {
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
        std::thread a(st_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_stereo_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("stereo driver: ok\n");
    return 0;
}
