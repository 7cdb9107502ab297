// Drives movba_two_view's HOST side (mov-slam_amd/csrc/two_view.cpp) against the fake device of this directory (fake_device.cpp,
// fake_two_view.cpp), under AddressSanitizer + UndefinedBehaviorSanitizer or ThreadSanitizer: invalid descriptors (refused
// before anything is written: canaries), n == 0, pairs under 5 matches, pinned and ordinary result arrays, a batch against its
// solo calls bit for bit, a call between an LBA upload and its run, two threads on two handles.
// Exit code 0 and the last line "TWO_VIEW OK" = every check held.
// With two arguments (input file, output file) it solves the one pair of the input file instead and writes the result with
// its hypothesis tables, all as doubles: tests/test_two_view_cpu.py compares the library's own arithmetic with its restatement.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_two_view_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

// camera 2 one unit to the side of camera 1, points 4 - 20 units ahead, a fifth of the matches wrong
struct Pair {
    std::vector<double> obs1, obs2, points;
    std::vector<uint8_t> inlier, good, code;
    movba_two_view_desc d{};
    movba_two_view_result r{};
    int n = 0;
};

void make_pair(Pair &s, int n, unsigned seed, int iters = 24)
{
    std::mt19937 rng(seed);
    s.n = n;
    s.obs1.resize(2 * (size_t)n + 2); s.obs2.resize(2 * (size_t)n + 2);
    for (int m = 0; m < n; ++m) {
        const double X = -3.0 + 0.006 * (rng() % 1000), Y = -2.0 + 0.004 * (rng() % 1000), Z = 4.0 + 0.016 * (rng() % 1000);
        s.obs1[2 * m] = 450 * X / Z + 320; s.obs1[2 * m + 1] = 450 * Y / Z + 240;
        s.obs2[2 * m] = 450 * (X - 1.0) / Z + 320; s.obs2[2 * m + 1] = 450 * Y / Z + 240;
        if (m % 5 == 4) { s.obs2[2 * m] = (double)(rng() % 640); s.obs2[2 * m + 1] = (double)(rng() % 480); }
    }
    s.points.assign(3 * (size_t)n + 3, -7.0); s.inlier.assign((size_t)n + 1, 99); s.good.assign((size_t)n + 1, 99); s.code.assign((size_t)n + 1, 99);
    s.d = movba_two_view_desc{};
    s.d.n_matches = n; s.d.ransac_iters = iters; s.d.obs1 = s.obs1.data(); s.d.obs2 = s.obs2.data();
    s.d.fx = 450; s.d.fy = 450; s.d.cx = 320; s.d.cy = 240;
    s.d.threshold = 1.0; s.d.confidence = 0.999; s.d.sigma = 1.0; s.d.min_parallax_deg = 1.0; s.d.max_depth = 50.0;
    s.d.min_triangulated = 50; s.d.ransac_seed = seed;
    s.r = movba_two_view_result{};
    s.r.inlier = s.inlier.data(); s.r.points = s.points.data(); s.r.good = s.good.data(); s.r.code = s.code.data();
    s.r.status = 99; s.r.outcome = 99;
}

void check_ok(const Pair &s)
{
    EXPECT(s.r.status == MOVBA_OK && s.r.outcome == MOVBA_TV_OK);
    EXPECT(s.r.n_inliers >= s.n * 3 / 4 && s.r.n_pass <= s.r.n_inliers && s.r.n_good <= s.r.n_pass);
    // T21 of a camera one unit to the right: identity rotation, t = (-1, 0, 0)
    EXPECT(std::fabs(s.r.pose[3]) > 1.0 - 1e-9 && std::fabs(s.r.pose[4] + 1.0) < 1e-6 && std::fabs(s.r.pose[5]) < 1e-6);
    EXPECT(s.points[3 * (size_t)s.n] == -7.0 && s.inlier[s.n] == 99 && s.good[s.n] == 99 && s.code[s.n] == 99);
}

bool same_result(const Pair &a, const Pair &b)
{
    return std::memcmp(a.r.pose, b.r.pose, sizeof a.r.pose) == 0 && std::memcmp(a.r.E, b.r.E, sizeof a.r.E) == 0 &&
           std::memcmp(&a.r.parallax_deg, &b.r.parallax_deg, 8) == 0 && a.r.outcome == b.r.outcome && a.r.n_inliers == b.r.n_inliers &&
           a.r.n_pass == b.r.n_pass && a.r.n_good == b.r.n_good && a.r.samples_used == b.r.samples_used && a.inlier == b.inlier &&
           a.good == b.good && a.code == b.code && std::memcmp(a.points.data(), b.points.data(), 8 * a.points.size()) == 0;
}

void invalid_calls(movba_handle *h)
{
    Pair s[2];
    make_pair(s[0], 200, 3u); make_pair(s[1], 120, 4u);
    auto refused = [&](movba_two_view_desc d1, movba_two_view_result r1, const char *what) {
        movba_two_view_desc ds[2] = { s[0].d, d1 };
        movba_two_view_result rs[2] = { s[0].r, r1 };
        rs[0].status = rs[1].status = 99; rs[0].outcome = rs[1].outcome = 99; rs[0].n_inliers = -5;
        const int rc = movba_two_view(h, ds, rs, 2);
        const bool clean = s[0].points[0] == -7.0 && s[0].inlier[0] == 99 && s[0].code[0] == 99 && s[0].good[0] == 99 && s[1].points[0] == -7.0 &&
                           s[1].inlier[0] == 99 && rs[0].outcome == 99 && rs[0].n_inliers == -5 && rs[1].outcome == 99;
        if (rc != MOVBA_ERR_ARG || rs[0].status != MOVBA_ERR_ARG || rs[1].status != MOVBA_ERR_ARG || !clean) {
            std::fprintf(stderr, "invalid call not refused cleanly: %s (rc %d)\n", what, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    };
    movba_two_view_desc d = s[1].d;
    const movba_two_view_result r = s[1].r;
    d.n_matches = -1; refused(d, r, "negative n_matches"); d = s[1].d;
    d.n_matches = MOVBA_MAX_TWO_VIEW_MATCHES + 1; refused(d, r, "too many matches"); d = s[1].d;
    d.ransac_iters = 0; refused(d, r, "no samples"); d.ransac_iters = MOVBA_MAX_TWO_VIEW_ITERS + 1; refused(d, r, "too many samples"); d = s[1].d;
    d.obs1 = nullptr; refused(d, r, "NULL obs1"); d = s[1].d;
    d.obs2 = nullptr; refused(d, r, "NULL obs2"); d = s[1].d;
    d.fx = 0.0; refused(d, r, "fx = 0"); d.fx = std::nan(""); refused(d, r, "NaN fx"); d = s[1].d;
    d.fy = -1.0; refused(d, r, "negative fy"); d = s[1].d;
    d.cx = INFINITY; refused(d, r, "infinite cx"); d = s[1].d;
    d.threshold = 0.0; refused(d, r, "threshold 0"); d = s[1].d;
    d.confidence = std::nan(""); refused(d, r, "NaN confidence"); d = s[1].d;
    d.sigma = -1.0; refused(d, r, "negative sigma"); d = s[1].d;
    d.min_parallax_deg = std::nan(""); refused(d, r, "NaN parallax"); d = s[1].d;
    d.max_depth = 0.0; refused(d, r, "max_depth 0"); d = s[1].d;
    d.min_triangulated = -1; refused(d, r, "negative min_triangulated"); d = s[1].d;
    movba_two_view_result q = r;
    q.inlier = nullptr; refused(d, q, "NULL inlier"); q = r;
    q.points = nullptr; refused(d, q, "NULL points"); q = r;
    q.good = nullptr; refused(d, q, "NULL good"); q = r;
    q.code = nullptr; refused(d, q, "NULL code");
    EXPECT(movba_two_view(nullptr, &s[0].d, &s[0].r, 1) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view(h, nullptr, &s[0].r, 1) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view(h, &s[0].d, nullptr, 1) == MOVBA_ERR_ARG);
    EXPECT(movba_two_view(h, &s[0].d, &s[0].r, -1) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view(h, &s[0].d, &s[0].r, MOVBA_MAX_TWO_VIEW_BATCH + 1) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view(h, nullptr, nullptr, 0) == MOVBA_OK);
    // ... and the valid descriptor still works afterwards
    EXPECT(movba_two_view(h, &s[0].d, &s[0].r, 1) == MOVBA_OK);
    check_ok(s[0]);
}

// a batch with pairs under 5 matches and pinned arrays in it against the solo calls
void batch_against_solo(movba_handle *h, unsigned seed)
{
    const int sizes[6] = { 150, 4, 90, 0, 260, 5 };
    Pair b[6], solo[6];
    movba_two_view_desc ds[6];
    movba_two_view_result rs[6];
    for (int k = 0; k < 6; ++k) { make_pair(b[k], sizes[k], seed + k); make_pair(solo[k], sizes[k], seed + k); ds[k] = b[k].d; rs[k] = b[k].r; }
    const size_t n2 = 90;
    double *pp = static_cast<double *>(movba_host_alloc(sizeof(double) * 3 * n2));
    uint8_t *pc = static_cast<uint8_t *>(movba_host_alloc(n2));
    EXPECT(pp && pc);
    if (!pp || !pc) return;
    rs[2].points = pp; rs[2].code = pc;
    std::vector<int32_t> nsol(24, -3);
    std::vector<double> hE(24 * 90, -3.0), hl(24 * 10, -3.0);
    rs[4].hyp_nsol = nsol.data(); rs[4].hyp_E = hE.data(); rs[4].hyp_loss = hl.data();
    EXPECT(movba_two_view(h, ds, rs, 6) == MOVBA_OK);
    std::memcpy(b[2].points.data(), pp, sizeof(double) * 3 * n2); std::memcpy(b[2].code.data(), pc, n2);
    for (int k = 0; k < 6; ++k) {
        b[k].r = rs[k];
        EXPECT(movba_two_view(h, &solo[k].d, &solo[k].r, 1) == MOVBA_OK);
        EXPECT(rs[k].status == (sizes[k] >= 5 ? MOVBA_OK : MOVBA_EMPTY) && solo[k].r.status == rs[k].status);
        EXPECT(same_result(b[k], solo[k]));
        if (sizes[k] < 5) EXPECT(rs[k].outcome == MOVBA_TV_NO_MODEL && b[k].inlier[0] == 99 && b[k].points[0] == -7.0);
    }
    check_ok(solo[0]); check_ok(solo[4]);
    EXPECT(solo[5].r.status == MOVBA_OK && solo[5].r.outcome != MOVBA_TV_OK);      // (5 matches: fewer than min_triangulated)
    bool diag = true;
    for (int k = 0; k < 24; ++k) diag &= nsol[k] >= 0 && nsol[k] <= 10 && (nsol[k] == 10 || std::isinf(hl[10 * k + nsol[k]])) && (nsol[k] == 0 || hl[10 * k] >= 0.0);
    EXPECT(diag);
    movba_host_free(pp); movba_host_free(pc);
}

void lba_with_two_view(movba_handle *h, int reps, unsigned seed)
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
        Pair a; make_pair(a, 300 + 100 * rep, seed + rep);
        EXPECT(movba_two_view(h, &a.d, &a.r, 1) == MOVBA_OK); check_ok(a);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        Pair b; make_pair(b, 150, seed + 50 + rep);
        EXPECT(movba_two_view(h, &b.d, &b.r, 1) == MOVBA_OK); check_ok(b);
        EXPECT(movba_lba_download(h, &res) == MOVBA_OK);
        EXPECT(res.n_solves == 10 && op[3] == 1.0 && opt[0] == 1.0 && oo[0] == 0 && oc[0] == 1.0);
    }
}

int solve_file(const char *fin, const char *fout)
{
    FILE *f = std::fopen(fin, "rb");
    if (!f) return 2;
    int32_t hd[3];
    double cam[4];
    if (std::fread(hd, 4, 3, f) != 3 || std::fread(cam, 8, 4, f) != 4) return 2;
    const int n = hd[0], iters = hd[1];
    Pair s; make_pair(s, n, (unsigned)hd[2], iters);
    if (std::fread(s.obs1.data(), 8, 2 * (size_t)n, f) != 2 * (size_t)n || std::fread(s.obs2.data(), 8, 2 * (size_t)n, f) != 2 * (size_t)n) return 2;
    std::fclose(f);
    s.d.fx = cam[0]; s.d.fy = cam[1]; s.d.cx = cam[2]; s.d.cy = cam[3];
    std::vector<int32_t> nsol(iters);
    std::vector<double> hE(90 * (size_t)iters), hl(10 * (size_t)iters);
    s.r.hyp_nsol = nsol.data(); s.r.hyp_E = hE.data(); s.r.hyp_loss = hl.data();
    movba_handle *h = nullptr;
    if (movba_create(&h, 0, nullptr, nullptr) != MOVBA_OK || movba_two_view(h, &s.d, &s.r, 1) != MOVBA_OK) return 3;
    movba_destroy(h);
    std::vector<double> out;
    for (int e = 0; e < 7; ++e) out.push_back(s.r.pose[e]);
    for (int e = 0; e < 9; ++e) out.push_back(s.r.E[e]);
    const double tail[8] = { s.r.parallax_deg, (double)s.r.outcome, (double)s.r.n_inliers, (double)s.r.n_pass, (double)s.r.n_good,
                             (double)s.r.samples_used, (double)s.r.status, 0.0 };
    out.insert(out.end(), tail, tail + 8);
    for (int m = 0; m < n; ++m) out.push_back(s.inlier[m]);
    for (int m = 0; m < n; ++m) out.push_back(s.good[m]);
    for (int m = 0; m < n; ++m) out.push_back(s.code[m]);
    out.insert(out.end(), s.points.begin(), s.points.begin() + 3 * (size_t)n);
    for (int k = 0; k < iters; ++k) out.push_back(nsol[k]);
    out.insert(out.end(), hE.begin(), hE.end());
    out.insert(out.end(), hl.begin(), hl.end());
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return fake_two_view_errors() ? 4 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 3) return solve_file(argv[1], argv[2]);
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        invalid_calls(h);
        batch_against_solo(h, 11u);
        invalid_calls(h);
        movba_destroy(h);
    }
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        lba_with_two_view(h, 2, 70u);
        movba_destroy(h);
    }
    {
        auto tv_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            batch_against_solo(h, seed);
            movba_destroy(h);
        };
        auto lba_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            lba_with_two_view(h, 2, seed);
            movba_destroy(h);
        };
        std::thread a(tv_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_two_view_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("TWO_VIEW OK\n");
    return 0;
}
