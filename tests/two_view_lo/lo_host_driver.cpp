// Drives movba_two_view_lo's HOST side (mov-slam_amd/csrc/two_view.cpp: the front it shares with movba_two_view, the refit
// slot's sizing, upload and read-out) against the fake device of tests/hipstub under AddressSanitizer +
// UndefinedBehaviorSanitizer.  The fake device does not run the refit and never writes the slot, so every call must come back
// with movba_two_view's results bit for bit and kept = steps = 0: what is checked here is the host's layout and hand-offs,
// lo_iters outside its range refused before anything is written (canaries), n == 0, `info` NULL or given, batches with pairs
// under 5 matches and pinned arrays.  Exit code 0 and the last line "TWO_VIEW_LO OK" = every check held.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "movba.h"

extern "C" int fake_two_view_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

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

bool same_result(const Pair &a, const Pair &b)
{
    return std::memcmp(a.r.pose, b.r.pose, sizeof a.r.pose) == 0 && std::memcmp(a.r.E, b.r.E, sizeof a.r.E) == 0 &&
           std::memcmp(&a.r.parallax_deg, &b.r.parallax_deg, 8) == 0 && a.r.status == b.r.status && a.r.outcome == b.r.outcome &&
           a.r.n_inliers == b.r.n_inliers && a.r.n_pass == b.r.n_pass && a.r.n_good == b.r.n_good && a.r.samples_used == b.r.samples_used &&
           a.inlier == b.inlier && a.good == b.good && a.code == b.code && std::memcmp(a.points.data(), b.points.data(), 8 * a.points.size()) == 0;
}

void invalid_calls(movba_handle *h)
{
    Pair s[2];
    make_pair(s[0], 200, 3u); make_pair(s[1], 120, 4u);
    const int bad[4] = { -1, MOVBA_MAX_TWO_VIEW_LO_ITERS + 1, -2147483647 - 1, 2147483647 };
    for (int lo : bad) {
        movba_two_view_desc ds[2] = { s[0].d, s[1].d };
        movba_two_view_result rs[2] = { s[0].r, s[1].r };
        movba_two_view_lo_info info[2];
        std::memset(info, 0x5a, sizeof info);
        rs[0].status = rs[1].status = 99; rs[0].outcome = rs[1].outcome = 99; rs[0].n_inliers = -5;
        EXPECT(movba_two_view_lo(h, ds, rs, 2, lo, info) == MOVBA_ERR_ARG);
        EXPECT(rs[0].status == MOVBA_ERR_ARG && rs[1].status == MOVBA_ERR_ARG && rs[0].outcome == 99 && rs[1].outcome == 99 && rs[0].n_inliers == -5);
        EXPECT(s[0].points[0] == -7.0 && s[0].inlier[0] == 99 && s[0].code[0] == 99 && s[0].good[0] == 99 && s[1].points[0] == -7.0);
        const unsigned char *b = reinterpret_cast<const unsigned char *>(info);
        bool untouched = true;
        for (size_t k = 0; k < sizeof info; ++k) untouched &= b[k] == 0x5a;
        EXPECT(untouched);
        EXPECT(movba_two_view_lo(h, nullptr, nullptr, 0, lo, nullptr) == MOVBA_ERR_ARG);
    }
    // an invalid descriptor is refused as by movba_two_view
    {
        movba_two_view_desc d = s[1].d;
        movba_two_view_result r = s[1].r;
        movba_two_view_lo_info info;
        std::memset(&info, 0x5a, sizeof info);
        d.ransac_iters = 0; r.status = 99; r.outcome = 99;
        EXPECT(movba_two_view_lo(h, &d, &r, 1, 10, &info) == MOVBA_ERR_ARG && r.status == MOVBA_ERR_ARG && r.outcome == 99 && info.kept == 0x5a5a5a5a);
    }
    EXPECT(movba_two_view_lo(nullptr, &s[0].d, &s[0].r, 1, 10, nullptr) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view_lo(h, nullptr, &s[0].r, 1, 10, nullptr) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view_lo(h, &s[0].d, nullptr, 1, 10, nullptr) == MOVBA_ERR_ARG);
    EXPECT(movba_two_view_lo(h, &s[0].d, &s[0].r, -1, 10, nullptr) == MOVBA_ERR_ARG && s[0].r.status == 99);
    EXPECT(movba_two_view_lo(h, &s[0].d, &s[0].r, MOVBA_MAX_TWO_VIEW_BATCH + 1, 10, nullptr) == MOVBA_ERR_ARG && s[0].r.status == 99);
    for (int lo : { 0, 10, MOVBA_MAX_TWO_VIEW_LO_ITERS }) EXPECT(movba_two_view_lo(h, nullptr, nullptr, 0, lo, nullptr) == MOVBA_OK);
}

// a batch with pairs under 5 matches and pinned arrays in it: movba_two_view_lo against movba_two_view
void batch_against_plain(movba_handle *h, unsigned seed, int lo_iters, bool with_info)
{
    const int sizes[6] = { 150, 4, 90, 0, 260, 5 };
    Pair b[6], plain[6];
    movba_two_view_desc ds[6];
    movba_two_view_result rs[6];
    movba_two_view_lo_info info[7];
    std::memset(info, 0x5a, sizeof info);
    for (int k = 0; k < 6; ++k) { make_pair(b[k], sizes[k], seed + k); make_pair(plain[k], sizes[k], seed + k); ds[k] = b[k].d; rs[k] = b[k].r; }
    const size_t n2 = 90;
    double *pp = static_cast<double *>(movba_host_alloc(sizeof(double) * 3 * n2));
    uint8_t *pc = static_cast<uint8_t *>(movba_host_alloc(n2));
    EXPECT(pp && pc);
    if (!pp || !pc) return;
    rs[2].points = pp; rs[2].code = pc;
    EXPECT(movba_two_view_lo(h, ds, rs, 6, lo_iters, with_info ? info : nullptr) == MOVBA_OK);
    std::memcpy(b[2].points.data(), pp, sizeof(double) * 3 * n2); std::memcpy(b[2].code.data(), pc, n2);
    for (int k = 0; k < 6; ++k) {
        b[k].r = rs[k];
        EXPECT(movba_two_view(h, &plain[k].d, &plain[k].r, 1) == MOVBA_OK);
        EXPECT(rs[k].status == (sizes[k] >= 5 ? MOVBA_OK : MOVBA_EMPTY));
        EXPECT(same_result(b[k], plain[k]));
        if (with_info) EXPECT(info[k].kept == 0 && info[k].steps == 0 && info[k].pad == 0 && info[k].loss == info[k].loss0);
    }
    EXPECT(plain[0].r.outcome == MOVBA_TV_OK && plain[4].r.outcome == MOVBA_TV_OK);
    EXPECT(info[6].kept == 0x5a5a5a5a);         // (the entry behind the last is not the call's)
    movba_host_free(pp); movba_host_free(pc);
}

}  // namespace

int main()
{
    movba_handle *h = nullptr;
    EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
    invalid_calls(h);
    for (int lo : { 0, 10, MOVBA_MAX_TWO_VIEW_LO_ITERS })
        for (int with_info = 0; with_info < 2; ++with_info) batch_against_plain(h, 11u + (unsigned)lo, lo, with_info != 0);
    invalid_calls(h);
    movba_destroy(h);
    EXPECT(fake_two_view_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("TWO_VIEW_LO OK\n");
    return 0;
}
