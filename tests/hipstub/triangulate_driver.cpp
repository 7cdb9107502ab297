// Drives movba_triangulate's HOST side (mov-slam_amd/csrc/triangulate.cpp) against the fake device of this directory
// (fake_device.cpp, fake_triangulate.cpp), under AddressSanitizer + UndefinedBehaviorSanitizer or ThreadSanitizer: invalid
// descriptors (refused before anything is written), calls that grow and shrink with empty pairs and stereo arrays coming and
// going, pinned and ordinary result arrays, a call between an LBA upload and its run, and two threads on two handles.  The
// fake device runs the library's per-match arithmetic, so recovered points and codes are checked too.
// Exit code 0 and the last line "TRIANGULATE OK" = every check held.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_triangulate_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

// a current keyframe at the origin and n_pairs neighbours to its side; every match observes a point 5 - 25 m ahead exactly
struct Scene {
    std::vector<double> poses, cam, bf, b, obs1, obs2, ur1, ur2, d1, d2, truth, points;
    std::vector<int32_t> pv, pp;
    std::vector<uint8_t> code;
    movba_tri_desc d{};
    movba_tri_result r{};
    int n = 0;
};

void make_scene(Scene &s, const std::vector<int> &sizes, unsigned seed, bool stereo)
{
    std::mt19937 rng(seed);
    const int np = (int)sizes.size(), nv = np + 1;
    s.poses.assign(7 * (size_t)nv, 0.0); s.cam.clear(); s.bf.assign(nv, 40.0); s.b.assign(nv, 0.125);
    for (int v = 0; v < nv; ++v) {
        s.poses[7 * v + 3] = 1.0; s.poses[7 * v + 4] = -0.4 * v;        // centre at x = 0.4 v
        const double k[4] = { 320, 320, 320, 240 };
        s.cam.insert(s.cam.end(), k, k + 4);
    }
    s.pv.clear(); s.pp.assign(1, 0);
    for (int p = 0; p < np; ++p) { s.pv.push_back(0); s.pv.push_back(p + 1); s.pp.push_back(s.pp.back() + sizes[p]); }
    const int n = s.pp.back();
    s.n = n;
    s.obs1.resize(2 * (size_t)n); s.obs2.resize(2 * (size_t)n); s.truth.resize(3 * (size_t)n);
    s.ur1.assign(n, -1.0); s.ur2.assign(n, -1.0); s.d1.assign(n, -1.0); s.d2.assign(n, -1.0);
    for (int p = 0, m = 0; p < np; ++p)
        for (int k = 0; k < sizes[p]; ++k, ++m) {
            const double X = -2.0 + 0.004 * (rng() % 1000), Y = -1.0 + 0.002 * (rng() % 1000), Z = 5.0 + 0.02 * (rng() % 1000);
            s.truth[3 * m] = X; s.truth[3 * m + 1] = Y; s.truth[3 * m + 2] = Z;
            const double x2 = X - 0.4 * (p + 1);
            s.obs1[2 * m] = 320 * X / Z + 320; s.obs1[2 * m + 1] = 320 * Y / Z + 240;
            s.obs2[2 * m] = 320 * x2 / Z + 320; s.obs2[2 * m + 1] = 320 * Y / Z + 240;
            if (stereo && m % 3 == 0) { s.ur1[m] = s.obs1[2 * m] - 40.0 / Z; s.d1[m] = Z; }
        }
    s.points.assign(3 * (size_t)n + 3, -7.0); s.code.assign((size_t)n + 1, 99);
    s.d = movba_tri_desc{};
    s.d.n_views = nv; s.d.n_pairs = np; s.d.poses = s.poses.data(); s.d.cam = s.cam.data();
    s.d.pair_view = s.pv.data(); s.d.pair_ptr = s.pp.data(); s.d.obs1 = s.obs1.data(); s.d.obs2 = s.obs2.data();
    if (stereo) {
        s.d.bf = s.bf.data(); s.d.b = s.b.data(); s.d.ur1 = s.ur1.data(); s.d.depth1 = s.d1.data();
        s.d.ur2 = s.ur2.data(); s.d.depth2 = s.d2.data();
    }
    s.d.reproj_gate = 5.0; s.d.far_threshold = 0.0;
    s.r = movba_tri_result{};
    s.r.points = s.points.data(); s.r.code = s.code.data(); s.r.status = 99; s.r.n_accepted = -5;
}

void check_results(const Scene &s, const double *points, const uint8_t *code, bool stereo)
{
    bool ok = true;
    for (int m = 0; m < s.n; ++m) {
        const uint8_t want = (stereo && m % 3 == 0) ? MOVBA_TRI_STEREO1 : MOVBA_TRI_DLT;
        ok &= code[m] == want;
        for (int k = 0; k < 3; ++k) ok &= std::fabs(points[3 * m + k] - s.truth[3 * m + k]) < 1e-8;
    }
    EXPECT(ok);
}

void run_scene(movba_handle *h, const std::vector<int> &sizes, unsigned seed, bool stereo, bool pinned)
{
    Scene s;
    make_scene(s, sizes, seed, stereo);
    double *pp = nullptr; uint8_t *pc = nullptr;
    if (pinned && s.n > 0) {
        pp = static_cast<double *>(movba_host_alloc(sizeof(double) * 3 * (size_t)s.n));
        pc = static_cast<uint8_t *>(movba_host_alloc((size_t)s.n));
        EXPECT(pp && pc);
        if (!pp || !pc) return;
        s.r.points = pp; s.r.code = pc;
    }
    EXPECT(movba_triangulate(h, &s.d, &s.r) == MOVBA_OK);
    EXPECT(s.r.status == MOVBA_OK && s.r.n_accepted == s.n);
    check_results(s, s.r.points, s.r.code, stereo);
    // nothing written past the arrays' ends
    if (!pinned) EXPECT(s.points[3 * (size_t)s.n] == -7.0 && s.code[s.n] == 99);
    if (pp) movba_host_free(pp);
    if (pc) movba_host_free(pc);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    const std::vector<std::vector<int>> rounds = { { 5 }, { 0, 3, 0, 0, 700, 1 }, { 20000, 0, 45000 }, { 1 }, { 300, 300 },
                                                   { 90000, 90000, 20 }, { 0, 0, 0 }, { 64, 256, 257, 1023 } };
    int k = 0;
    for (const auto &sz : rounds) { run_scene(h, sz, seed + k, k % 2 == 1, k % 3 == 2); ++k; }
}

void invalid_calls(movba_handle *h)
{
    Scene s;
    make_scene(s, { 10, 0, 20 }, 3u, true);
    auto refused = [&](movba_tri_desc d, const char *what) {
        movba_tri_result r = s.r;
        r.status = 99; r.n_accepted = -5;
        const int rc = movba_triangulate(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || r.n_accepted != -5 || s.points[0] != -7.0 || s.code[0] != 99) {
            std::fprintf(stderr, "invalid call not refused cleanly: %s (rc %d)\n", what, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    };
    movba_tri_desc d = s.d;
    d.n_views = -1; refused(d, "negative n_views"); d = s.d;
    d.n_pairs = -1; refused(d, "negative n_pairs"); d = s.d;
    std::vector<int32_t> pp = s.pp;
    pp[0] = 1; d.pair_ptr = pp.data(); refused(d, "pair_ptr[0] != 0"); pp = s.pp;
    pp[2] = 5; d.pair_ptr = pp.data(); refused(d, "pair_ptr descending"); d = s.d;
    std::vector<int32_t> pv = s.pv;
    pv[3] = s.d.n_views; d.pair_view = pv.data(); refused(d, "view index too large");
    pv[3] = -1; refused(d, "view index negative"); d = s.d;
    d.bf = nullptr; refused(d, "ur without bf"); d = s.d;
    d.b = nullptr; refused(d, "ur without b"); d = s.d;
    d.depth1 = nullptr; refused(d, "ur1 without depth1"); d = s.d;
    d.depth2 = nullptr; refused(d, "ur2 without depth2"); d = s.d;
    d.reproj_gate = std::nan(""); refused(d, "NaN gate"); d.reproj_gate = INFINITY; refused(d, "infinite gate"); d = s.d;
    d.far_threshold = std::nan(""); refused(d, "NaN far threshold"); d = s.d;
    d.obs1 = nullptr; refused(d, "NULL obs1"); d = s.d;
    d.obs2 = nullptr; refused(d, "NULL obs2"); d = s.d;
    d.poses = nullptr; refused(d, "NULL poses"); d = s.d;
    d.cam = nullptr; refused(d, "NULL cam"); d = s.d;
    d.pair_ptr = nullptr; refused(d, "NULL pair_ptr"); d = s.d;
    d.pair_view = nullptr; refused(d, "NULL pair_view"); d = s.d;
    {
        movba_tri_result r = s.r; r.points = nullptr; r.status = 99;
        EXPECT(movba_triangulate(h, &s.d, &r) == MOVBA_ERR_ARG && r.status == MOVBA_ERR_ARG && s.code[0] == 99);
        r = s.r; r.code = nullptr; r.status = 99;
        EXPECT(movba_triangulate(h, &s.d, &r) == MOVBA_ERR_ARG && r.status == MOVBA_ERR_ARG && s.points[0] == -7.0);
    }
    EXPECT(movba_triangulate(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_triangulate(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_triangulate(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    // no matches: MOVBA_OK, nothing written but status and the count
    Scene e;
    make_scene(e, { 0, 0 }, 4u, false);
    e.r.points = nullptr; e.r.code = nullptr;
    EXPECT(movba_triangulate(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK && e.r.n_accepted == 0);
    movba_tri_desc none{};
    none.reproj_gate = 5.0;
    EXPECT(movba_triangulate(h, &none, &e.r) == MOVBA_OK);
    // ... and the valid descriptor still works afterwards
    EXPECT(movba_triangulate(h, &s.d, &s.r) == MOVBA_OK && s.r.n_accepted == s.n);
    check_results(s, s.r.points, s.r.code, true);
}

// an LBA window uploaded, then a triangulation on the same handle, then the window's run: the window's arrays leave the staging
// buffer before the call overwrites it, and the window's results are still downloaded after it
void lba_with_triangulation(movba_handle *h, int reps, unsigned seed)
{
    const int NP = 12, P = 800;
    std::vector<double> poses(7 * NP, 0.0), points(3 * P, 1.0), obs, isig;
    std::vector<uint8_t> fixed(NP, 0);
    std::vector<int32_t> ep, el;
    for (int i = 0; i < NP; ++i) { poses[7 * i + 3] = 1.0; poses[7 * i + 4] = 0.3 * i; fixed[i] = i < 2; }
    std::mt19937 rng(9);
    for (int l = 0; l < P; ++l) {
        const int run = 2 + (int)(rng() % 4), first = (int)(rng() % (unsigned)(NP - run + 1));
        for (int k = first; k < first + run; ++k) { ep.push_back(k); el.push_back(l); }
    }
    const size_t E = ep.size();
    obs.assign(2 * E, 100.0); isig.assign(E, 1.0);
    movba_lba_desc w{};
    w.n_poses = NP; w.n_points = P; w.n_edges = (int32_t)E;
    w.poses = poses.data(); w.pose_fixed = fixed.data(); w.points = points.data();
    w.edge_pose = ep.data(); w.edge_point = el.data(); w.obs = obs.data(); w.inv_sigma2 = isig.data();
    w.fx = w.fy = 320; w.cx = 320; w.cy = 240; w.huber_delta = 2.236; w.chi2_gate = 5.0; w.max_iters = 10; w.flags = MOVBA_FLAG_STALE_ERROR_QUIRK;
    std::vector<double> op(7 * NP, 0.0), opt(3 * P, 0.0), oc(E, 0.0);
    std::vector<uint8_t> oo(E, 9);
    movba_lba_result res{};
    res.poses = op.data(); res.points = opt.data(); res.chi2 = oc.data(); res.outlier = oo.data();
    for (int rep = 0; rep < reps; ++rep) {
        EXPECT(movba_lba_upload(h, &w) == MOVBA_OK);
        run_scene(h, { 3000 + 500 * rep, 0, 800 }, seed + rep, rep % 2 == 0, false);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_scene(h, { 100, 5000 }, seed + 50 + rep, false, rep % 2 == 1);
        EXPECT(movba_lba_download(h, &res) == MOVBA_OK);
        EXPECT(res.n_solves == 10 && op[3] == 1.0 && opt[0] == 1.0 && oo[0] == 0 && oc[0] == 1.0);
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
        invalid_calls(h);
        movba_destroy(h);
    }
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        lba_with_triangulation(h, 3, 70u);
        movba_destroy(h);
    }
    {
        auto tri_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            for (int it = 0; it < 2; ++it) growing_and_shrinking(h, seed + 100 * it);
            movba_destroy(h);
        };
        auto lba_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            lba_with_triangulation(h, 3, seed);
            movba_destroy(h);
        };
        std::thread a(tri_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_triangulate_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("TRIANGULATE OK\n");
    return 0;
}
