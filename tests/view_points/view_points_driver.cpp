// Drives movba_view_points' HOST side (mov-slam_amd/csrc/view_points.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_view_points.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or
// ThreadSanitizer.  The fake launch runs the library's own per-item arithmetic, so every value that comes back is checked
// against that arithmetic called here directly; what is under test is the host's side: every refusal of the header before
// anything is written (canaries), a call without views, empty views among others and alone, optional arrays left NULL, pinned
// against ordinary result memory, a call between the upload and the runs of a window on the same handle, and two handles on
// two threads.  Exit code 0 and the last line "view_points driver: ok" = every check held.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"
#include "view_points.h"

extern "C" int fake_view_points_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr double kCanary = -7.0;

// views of the three modes in turn around a cloud of points 2 - 12 units ahead of cameras near the origin
struct Call {
    std::vector<double> points, normals, dmax, dmin, poses, cam, bf, bounds, lsf, cosl;
    std::vector<int32_t> mode, n_levels, q, view_ptr, item;
    // results, each one entry longer than asked for: the canary behind the end
    std::vector<uint8_t> code;
    std::vector<double> z, uv, dist, vcos, ur, depth, median;
    std::vector<int32_t> level, nacc;
    movba_view_desc d{};
    movba_view_result r{};
    int n = 0, nv = 0;
};

void make_call(Call &s, const std::vector<int> &sizes, unsigned seed, int only_mode = -1)
{
    std::mt19937 rng(seed);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(rng() % 100000) / 100000.0; };
    const int np = 500, nv = (int)sizes.size();
    s.nv = nv;
    s.points.resize(3 * np); s.normals.resize(3 * np); s.dmax.resize(np); s.dmin.resize(np);
    for (int p = 0; p < np; ++p) {
        const double X[3] = { uni(-6, 6), uni(-4, 4), uni(-2, 12) };
        const double r = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) + 1e-3;
        for (int k = 0; k < 3; ++k) { s.points[3 * p + k] = X[k]; s.normals[3 * p + k] = X[k] / r + uni(-0.5, 0.5); }
        s.dmax[p] = r * uni(0.7, 3.0); s.dmin[p] = r * uni(0.3, 1.2);
    }
    s.poses.clear(); s.cam.clear(); s.bf.clear(); s.bounds.clear(); s.lsf.clear(); s.cosl.clear();
    s.mode.clear(); s.n_levels.clear(); s.q.clear(); s.view_ptr.assign(1, 0); s.item.clear();
    for (int v = 0; v < nv; ++v) {
        const double pose[7] = { uni(-0.1, 0.1), uni(-0.1, 0.1), uni(-0.1, 0.1), -2.0, uni(-0.5, 0.5), uni(-0.5, 0.5), uni(-0.5, 0.5) };
        s.poses.insert(s.poses.end(), pose, pose + 7);
        const double k[4] = { 420, 415, 320, 240 }, b[4] = { 0, 640, 0, 480 };
        s.cam.insert(s.cam.end(), k, k + 4); s.bounds.insert(s.bounds.end(), b, b + 4);
        s.bf.push_back(40.0); s.lsf.push_back(std::log(1.2)); s.cosl.push_back(0.5);
        s.mode.push_back(only_mode >= 0 ? only_mode : v % 3); s.n_levels.push_back(8); s.q.push_back(1 + v % 3);
        for (int k2 = 0; k2 < sizes[v]; ++k2) s.item.push_back((int32_t)(rng() % np));
        s.view_ptr.push_back((int32_t)s.item.size());
    }
    const int n = (int)s.item.size();
    s.n = n;
    s.code.assign((size_t)n + 1, 99); s.level.assign((size_t)n + 1, -5); s.nacc.assign((size_t)nv + 1, -5);
    s.z.assign((size_t)n + 1, kCanary); s.uv.assign(2 * (size_t)n + 1, kCanary); s.dist.assign((size_t)n + 1, kCanary);
    s.vcos.assign((size_t)n + 1, kCanary); s.ur.assign((size_t)n + 1, kCanary); s.depth.assign((size_t)n + 1, kCanary);
    s.median.assign((size_t)nv + 1, kCanary);
    s.d = movba_view_desc{};
    s.d.n_points = np; s.d.n_views = nv; s.d.points = s.points.data(); s.d.normals = s.normals.data();
    s.d.max_distance = s.dmax.data(); s.d.min_distance = s.dmin.data(); s.d.mode = s.mode.data(); s.d.poses = s.poses.data();
    s.d.cam = s.cam.data(); s.d.bf = s.bf.data(); s.d.bounds = s.bounds.data(); s.d.log_scale_factor = s.lsf.data();
    s.d.n_levels = s.n_levels.data(); s.d.cos_limit = s.cosl.data(); s.d.q = s.q.data(); s.d.view_ptr = s.view_ptr.data();
    s.d.item_point = s.item.data();
    s.r = movba_view_result{};
    s.r.code = s.code.data(); s.r.z = s.z.data(); s.r.uv = s.uv.data(); s.r.dist = s.dist.data(); s.r.view_cos = s.vcos.data();
    s.r.level = s.level.data(); s.r.ur = s.ur.data(); s.r.track_depth = s.depth.data(); s.r.n_accepted = s.nacc.data();
    s.r.median_depth = s.median.data(); s.r.status = 99; s.r.pad = 77;
}

bool untouched(const Call &s)
{
    bool ok = s.r.pad == 77;
    for (uint8_t v : s.code) ok &= v == 99;
    for (int32_t v : s.level) ok &= v == -5;
    for (int32_t v : s.nacc) ok &= v == -5;
    for (const std::vector<double> *a : { &s.z, &s.uv, &s.dist, &s.vcos, &s.ur, &s.depth, &s.median })
        for (double v : *a) ok &= v == kCanary;
    return ok;
}

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

// what came back (through r's pointers: pinned or not) against the arithmetic called directly
void check(const Call &s, const movba_view_result &r)
{
    using namespace movba;
    bool ok = true;
    for (int v = 0; v < s.nv; ++v) {
        VpView w{};
        w.mode = s.mode[v]; w.n_levels = s.n_levels[v]; w.q = s.q[v];
        for (int e = 0; e < 7; ++e) w.pose[e] = s.poses[7 * v + e];
        for (int e = 0; e < 4; ++e) { w.cam[e] = s.cam[4 * v + e]; w.bounds[e] = s.bounds[4 * v + e]; }
        w.bf = s.bf[v]; w.log_scale = s.lsf[v]; w.cos_limit = s.cosl[v];
        double view[kVpViewDoubles];
        vp_view(w, view);
        int32_t acc = 0;
        std::vector<uint64_t> keys;
        for (int i = s.view_ptr[v]; i < s.view_ptr[v + 1]; ++i) {
            const size_t p = (size_t)s.item[i];
            const VpItem it = vp_item(w.mode, w.n_levels, view, &s.points[3 * p], &s.normals[3 * p], s.dmax[p], s.dmin[p]);
            ok &= r.code[i] == it.code;
            if (r.z) ok &= same(r.z[i], it.z);
            if (r.uv) ok &= same(r.uv[2 * i], it.u) && same(r.uv[2 * i + 1], it.v);
            if (r.dist) ok &= same(r.dist[i], it.dist);
            if (r.view_cos) ok &= same(r.view_cos[i], it.view_cos);
            if (r.level) ok &= r.level[i] == it.level;
            if (r.ur) ok &= same(r.ur[i], it.ur);
            if (r.track_depth) ok &= same(r.track_depth[i], it.track_depth);
            acc += it.code < MOVBA_VP_REJ_BEHIND;
            keys.push_back(im_order_key(it.z));
        }
        ok &= r.n_accepted[v] == acc;
        if (w.mode != MOVBA_VIEW_DEPTH) ok &= std::isnan(r.median_depth[v]);
        else if (keys.empty()) ok &= r.median_depth[v] == -1.0;
        else {
            // the rank by counting, as k_init_map finds it
            const int kmed = ((int)keys.size() - 1) / w.q;
            for (size_t a = 0; a < keys.size(); ++a) {
                int below = 0, equal = 0;
                for (size_t b = 0; b < keys.size(); ++b) { below += keys[b] < keys[a]; equal += keys[b] == keys[a]; }
                if (below <= kmed && kmed < below + equal) { ok &= same(r.median_depth[v], vp_key_value(keys[a])); break; }
            }
        }
    }
    EXPECT(ok);
}

void canaries_in_place(const Call &s)
{
    EXPECT(s.code[s.n] == 99 && s.level[s.n] == -5 && s.nacc[s.nv] == -5 && s.median[s.nv] == kCanary);
    EXPECT(s.z[s.n] == kCanary && s.uv[2 * (size_t)s.n] == kCanary && s.dist[s.n] == kCanary && s.vcos[s.n] == kCanary && s.ur[s.n] == kCanary &&
           s.depth[s.n] == kCanary);
}

void run_call(movba_handle *h, const std::vector<int> &sizes, unsigned seed, int variant)
{
    Call s;
    make_call(s, sizes, seed);
    std::vector<void *> blocks;
    auto pin = [&](size_t bytes) { void *p = movba_host_alloc(bytes ? bytes : 8); EXPECT(p != nullptr); blocks.push_back(p); return p; };
    movba_view_result r = s.r;
    const size_t n = (size_t)s.n, nv = (size_t)s.nv;
    if (variant == 1) {                 // everything pinned
        r.code = static_cast<uint8_t *>(pin(n)); r.z = static_cast<double *>(pin(8 * n)); r.uv = static_cast<double *>(pin(16 * n));
        r.dist = static_cast<double *>(pin(8 * n)); r.view_cos = static_cast<double *>(pin(8 * n)); r.level = static_cast<int32_t *>(pin(4 * n));
        r.ur = static_cast<double *>(pin(8 * n)); r.track_depth = static_cast<double *>(pin(8 * n));
        r.n_accepted = static_cast<int32_t *>(pin(4 * nv)); r.median_depth = static_cast<double *>(pin(8 * nv));
    } else if (variant == 2) {          // some pinned, some left out
        r.code = static_cast<uint8_t *>(pin(n)); r.uv = static_cast<double *>(pin(16 * n)); r.median_depth = static_cast<double *>(pin(8 * nv));
        r.z = nullptr; r.view_cos = nullptr; r.ur = nullptr;
    } else if (variant == 3) {          // every optional array left out
        r.z = r.uv = r.dist = r.view_cos = r.ur = r.track_depth = nullptr; r.level = nullptr;
    }
    for (void *p : blocks) if (!p) return;
    EXPECT(movba_view_points(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK && r.pad == 77);
    check(s, r);
    canaries_in_place(s);
    if (variant == 3) for (double v : s.z) EXPECT(v == kCanary);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    const std::vector<std::vector<int>> rounds = { { 5 }, { 0, 3, 0, 0, 700, 1 }, { 20000, 0, 4500 }, { 1 }, { 300, 300, 300 }, { 0, 0, 0 },
                                                   { 64, 256, 257, 1023, 255, 513 }, { 0, 0, 9000 }, { 1, 1, 1, 1, 1, 1, 1 } };
    int k = 0;
    for (const auto &sz : rounds) { run_call(h, sz, seed + k, k % 4); ++k; }
}

void invalid_calls(movba_handle *h)
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int which = 0; which < 41; ++which) {
        Call s;
        make_call(s, { 40, 0, 60, 10 }, 3u);           // modes 0 1 2 0
        movba_view_desc &d = s.d;
        movba_view_result &r = s.r;
        switch (which) {
        case 0: d.n_views = -1; break;
        case 1: d.n_points = -1; break;
        case 2: d.n_views = MOVBA_MAX_VIEW_BATCH + 1; break;
        case 3: s.view_ptr[0] = 1; break;
        case 4: s.view_ptr[2] = 30; break;                  // descending
        case 5: s.item[7] = 500; break;
        case 6: s.item[0] = -1; break;
        case 7: s.mode[1] = 3; break;
        case 8: s.mode[0] = -1; break;
        case 9: d.mode = nullptr; break;
        case 10: d.poses = nullptr; break;
        case 11: d.cam = nullptr; break;
        case 12: d.view_ptr = nullptr; break;
        case 13: d.item_point = nullptr; break;
        case 14: d.points = nullptr; break;
        case 15: d.normals = nullptr; break;
        case 16: d.max_distance = nullptr; break;
        case 17: d.min_distance = nullptr; break;
        case 18: d.bounds = nullptr; break;
        case 19: d.log_scale_factor = nullptr; break;
        case 20: d.n_levels = nullptr; break;
        case 21: d.cos_limit = nullptr; break;
        case 22: d.q = nullptr; break;
        case 23: r.code = nullptr; break;
        case 24: r.n_accepted = nullptr; break;
        case 25: r.median_depth = nullptr; break;
        case 26: s.cam[4] = 0.0; break;
        case 27: s.cam[1] = inf; break;
        case 28: s.cam[8] = -420.0; break;
        case 29: s.cam[2] = nan; break;
        case 30: s.bf[3] = inf; break;
        case 31: s.bounds[5] = nan; break;
        case 32: s.cosl[0] = nan; break;
        case 33: s.lsf[1] = inf; break;
        case 34: s.n_levels[3] = 0; break;
        case 35: s.q[2] = 0; break;
        case 36: s.lsf[0] = 0.0; break;
        case 37: s.lsf[3] = -0.2; break;
        case 38: s.poses[7 * 2 + 5] = nan; break;
        case 39: s.poses[7] = s.poses[8] = s.poses[9] = s.poses[10] = 0.0; break;
        case 40: s.poses[3] = inf; break;
        }
        const int rc = movba_view_points(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, { 10, 20, 30 }, 5u);
    EXPECT(movba_view_points(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_view_points(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_view_points(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    // what is not wrong: q < 1 on a view that is no DEPTH view, a log_scale_factor that is not positive on one that is no FRUSTUM
    // view, the arrays no mode reads left out
    s.q[0] = 0; s.q[1] = -3; s.lsf[1] = -1.0; s.lsf[2] = 0.0;
    EXPECT(movba_view_points(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    s.lsf[1] = s.lsf[2] = std::log(1.2);
    check(s, s.r);
    {
        Call e;
        make_call(e, { 100, 0, 7 }, 6u, MOVBA_VIEW_DEPTH);
        e.d.normals = e.d.max_distance = e.d.min_distance = e.d.bounds = e.d.log_scale_factor = e.d.cos_limit = e.d.bf = nullptr;
        e.d.n_levels = nullptr;
        EXPECT(movba_view_points(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK && e.nacc[0] == 100 && e.nacc[1] == 0 && e.nacc[2] == 7 && e.median[1] == -1.0);
        check(e, e.r);
        canaries_in_place(e);
        Call f;
        make_call(f, { 50, 5 }, 7u, MOVBA_VIEW_FUSE);
        f.d.log_scale_factor = f.d.cos_limit = f.d.bf = nullptr; f.d.n_levels = f.d.q = nullptr;
        EXPECT(movba_view_points(h, &f.d, &f.r) == MOVBA_OK);
        check(f, f.r);
    }
    // no views: MOVBA_OK and nothing but the status written
    {
        Call e;
        make_call(e, { 10 }, 8u);
        e.d.n_views = 0;
        EXPECT(movba_view_points(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        e.r.status = 99;
        EXPECT(untouched(e));
        movba_view_desc none{};
        movba_view_result r0{};
        r0.status = 99;
        EXPECT(movba_view_points(h, &none, &r0) == MOVBA_OK && r0.status == MOVBA_OK);
    }
    // views without items: the counts and the medians, no item array needed
    {
        Call e;
        make_call(e, { 0, 0, 0, 0 }, 9u);
        e.r.code = nullptr; e.d.item_point = nullptr; e.d.points = nullptr;
        EXPECT(movba_view_points(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        for (int v = 0; v < 4; ++v) EXPECT(e.nacc[v] == 0 && (v == 2 ? e.median[v] == -1.0 : std::isnan(e.median[v])));
        EXPECT(e.nacc[4] == -5 && e.median[4] == kCanary);
    }
}

struct Win {
    std::vector<double> poses, points, obs, isig, out_poses, out_points, out_chi2;
    std::vector<uint8_t> fixed, out_outlier;
    std::vector<int32_t> ep, el;
    movba_lba_desc d{};
    movba_lba_result r{};
};

void make_window(Win &w, int NP, int P)
{
    w.poses.assign(7 * (size_t)NP, 0.0); w.fixed.assign(NP, 0); w.points.assign(3 * (size_t)P, 1.0);
    for (int i = 0; i < NP; ++i) { w.poses[7 * i + 3] = 1.0; w.poses[7 * i + 4] = 0.3 * i; w.fixed[i] = i < 2; }
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

// a window uploaded, movba_view_points, the window's run, the call again, downloaded, run again, downloaded: both downloads are
// what the fake device exports
void shared_with_a_window(movba_handle *h, int reps, unsigned seed)
{
    Win w;
    make_window(w, 9, 600);
    for (int rep = 0; rep < reps; ++rep) {
        EXPECT(movba_lba_upload(h, &w.d) == MOVBA_OK);
        run_call(h, { 3000 + 500 * rep, 0, 800 }, seed + rep, rep % 4);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, { 100, 5000, 70 }, seed + 50 + rep, (rep + 1) % 4);
        for (int round = 0; round < 2; ++round) {
            EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK);
            EXPECT(w.r.n_solves == 10 && w.r.iters_done == 10 && w.out_poses[3] == 1.0 && w.out_points[0] == 1.0 && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
            std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0); std::fill(w.out_points.begin(), w.out_points.end(), 0.0);
            if (round == 0) {
                EXPECT(movba_lba_run(h) == MOVBA_OK);
                run_call(h, { 10, 20, 30 }, seed + 90 + rep, 1);
            }
        }
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
        shared_with_a_window(h, 2, 40u);
        invalid_calls(h);
        movba_destroy(h);
    }
    {
        auto vp_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            for (int it = 0; it < 2; ++it) growing_and_shrinking(h, seed + 100 * it);
            movba_destroy(h);
        };
        auto lba_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            shared_with_a_window(h, 3, seed);
            movba_destroy(h);
        };
        std::thread a(vp_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_view_points_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("view_points driver: ok\n");
    return 0;
}
