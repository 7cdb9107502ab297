// Drives movba_init_map's HOST side (mov-slam_amd/csrc/init_map.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_init_map.cpp, under the sanitizers.  The fake launch does not optimise (it returns
// the start estimate normalised: what the kernel gives for max_iters == 0), so what is checked here is the host's side: every
// refusal of the header before anything is written (canaries), n == 0, pairs without a used match between solved ones, the mask
// layout against the compacted one, pinned against ordinary result memory, `trace` NULL or given, and a call between two
// solves of an uploaded window.  Exit code 0 and the last line "init_map driver: ok" = every check held.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "movba.h"

extern "C" int fake_init_map_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// camera 2 one unit to the side of camera 1, points 4 - 20 units ahead; `spread`: the matches sit under a mask among slots of NaN
struct Pair {
    std::vector<double> obs1, obs2, pts, s1, s2, out_pts, out_chi2;
    std::vector<uint8_t> use;
    movba_init_map_desc d{};
    movba_init_map_result r{};
    int n = 0, n_used = 0;
};

void make_pair(Pair &s, int n_used, unsigned seed, bool spread, bool sigmas = false)
{
    std::mt19937 rng(seed);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int n = spread ? n_used + n_used / 2 + 3 : n_used;
    s.n = n; s.n_used = n_used;
    s.use.assign((size_t)n, spread ? 0 : 1);
    if (spread)
        for (int placed = 0; placed < n_used;) { const int i = (int)(rng() % (unsigned)n); if (!s.use[i]) { s.use[i] = 1 + (uint8_t)(rng() % 200); ++placed; } }
    std::mt19937 val(seed * 7919u + 1u);            // (the same values in the same order, spread out or not)
    s.obs1.assign(2 * (size_t)n, nan); s.obs2.assign(2 * (size_t)n, nan); s.pts.assign(3 * (size_t)n, nan);
    s.s1.assign((size_t)n, nan); s.s2.assign((size_t)n, nan);
    for (int m = 0; m < n; ++m) {
        if (!s.use[m]) continue;
        const double X = -3.0 + 0.006 * (val() % 1000), Y = -2.0 + 0.004 * (val() % 1000), Z = 4.0 + 0.016 * (val() % 1000);
        s.obs1[2 * m] = 450 * X / Z + 320; s.obs1[2 * m + 1] = 450 * Y / Z + 240;
        s.obs2[2 * m] = 450 * (X - 1.0) / Z + 320.4; s.obs2[2 * m + 1] = 450 * Y / Z + 239.7;
        s.pts[3 * m] = 1.01 * X; s.pts[3 * m + 1] = 1.01 * Y; s.pts[3 * m + 2] = 1.01 * Z;
        s.s1[m] = 1.0 / (1.0 + (val() % 3)); s.s2[m] = 1.0 / (1.0 + (val() % 3));
    }
    s.out_pts.assign(3 * (size_t)n + 3, -7.0); s.out_chi2.assign(2 * (size_t)n + 2, -7.0);
    s.d = movba_init_map_desc{};
    s.d.n_matches = n; s.d.max_iters = 20; s.d.max_trials = 0; s.d.min_tracked = 50;
    s.d.obs1 = s.obs1.data(); s.d.obs2 = s.obs2.data(); s.d.points = s.pts.data();
    s.d.use = spread ? s.use.data() : nullptr;
    if (sigmas) { s.d.inv_sigma2_1 = s.s1.data(); s.d.inv_sigma2_2 = s.s2.data(); }
    const double pose[7] = { 0.002, -0.001, 0.003, -2.0, -1.0, 0.01, 0.02 };       // (not normalised, w < 0)
    for (int e = 0; e < 7; ++e) s.d.pose2[e] = pose[e];
    s.d.fx = 450; s.d.fy = 450; s.d.cx = 320; s.d.cy = 240; s.d.huber_delta = 2.2360680103302;
    s.r = movba_init_map_result{};
    s.r.points = s.out_pts.data(); s.r.chi2 = s.out_chi2.data();
    s.r.status = 99; s.r.outcome = 99; s.r.n_used = -5; s.r.median_depth = -7.0;
}

bool untouched(const Pair &s)
{
    bool ok = s.r.outcome == 99 && s.r.n_used == -5 && s.r.median_depth == -7.0;
    for (double v : s.out_pts) ok &= v == -7.0;
    for (double v : s.out_chi2) ok &= v == -7.0;
    return ok;
}

// the used slots of two results of the same matches, and their scalars, equal to the bit; unused slots NaN; the canaries behind
// the arrays' ends in place
bool same_used(const Pair &a, const Pair &b)
{
    bool ok = std::memcmp(a.r.pose, b.r.pose, sizeof a.r.pose) == 0 && std::memcmp(&a.r.median_depth, &b.r.median_depth, 8) == 0 &&
              std::memcmp(&a.r.cost, &b.r.cost, 8) == 0 && std::memcmp(&a.r.cost0, &b.r.cost0, 8) == 0 && a.r.outcome == b.r.outcome &&
              a.r.status == b.r.status && a.r.n_used == b.r.n_used && a.r.n_solves == b.r.n_solves;
    std::vector<int> ia, ib;
    for (int m = 0; m < a.n; ++m) if (a.use[m]) ia.push_back(m);
    for (int m = 0; m < b.n; ++m) if (b.use[m]) ib.push_back(m);
    ok &= ia.size() == ib.size();
    for (size_t k = 0; ok && k < ia.size(); ++k)
        ok &= std::memcmp(&a.out_pts[3 * ia[k]], &b.out_pts[3 * ib[k]], 24) == 0 && std::memcmp(&a.out_chi2[2 * ia[k]], &b.out_chi2[2 * ib[k]], 16) == 0;
    for (const Pair *s : { &a, &b }) {
        for (int m = 0; m < s->n; ++m)
            if (!s->use[m]) ok &= std::isnan(s->out_pts[3 * m]) && std::isnan(s->out_pts[3 * m + 2]) && std::isnan(s->out_chi2[2 * m + 1]);
        ok &= s->out_pts[3 * (size_t)s->n] == -7.0 && s->out_chi2[2 * (size_t)s->n] == -7.0;
    }
    return ok;
}

void invalid_calls(movba_handle *h)
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int which = 0; which < 19; ++which) {
        Pair s[2];
        make_pair(s[0], 80, 3u, false); make_pair(s[1], 60, 4u, true);
        movba_init_map_desc &d = s[1].d;
        movba_init_map_result &r = s[1].r;
        switch (which) {
        case 0: d.n_matches = -1; break;
        case 1: d.n_matches = MOVBA_MAX_TWO_VIEW_MATCHES + 1; break;
        case 2: d.obs1 = nullptr; break;
        case 3: d.obs2 = nullptr; break;
        case 4: d.points = nullptr; break;
        case 5: r.points = nullptr; break;
        case 6: d.max_iters = -1; break;
        case 7: d.max_iters = MOVBA_MAX_INIT_MAP_ITERS + 1; break;
        case 8: d.max_trials = -1; break;
        case 9: d.min_tracked = -1; break;
        case 10: d.fx = 0.0; break;
        case 11: d.fy = inf; break;
        case 12: d.fx = -450.0; break;
        case 13: d.cx = nan; break;
        case 14: d.cy = inf; break;
        case 15: d.huber_delta = nan; break;
        case 16: d.pose2[5] = nan; break;
        case 17: d.pose2[0] = d.pose2[1] = d.pose2[2] = d.pose2[3] = 0.0; break;
        case 18: d.pose2[3] = inf; break;
        }
        movba_init_map_desc ds[2] = { s[0].d, s[1].d };
        movba_init_map_result rs[2] = { s[0].r, s[1].r };
        movba_init_map_trace tr[2];
        std::memset(tr, 0x5a, sizeof tr);
        EXPECT(movba_init_map(h, ds, rs, 2, tr) == MOVBA_ERR_ARG);
        EXPECT(rs[0].status == MOVBA_ERR_ARG && rs[1].status == MOVBA_ERR_ARG);
        s[0].r = rs[0]; s[1].r = rs[1];
        EXPECT(untouched(s[0]) && untouched(s[1]));
        const unsigned char *b = reinterpret_cast<const unsigned char *>(tr);
        bool clean = true;
        for (size_t k = 0; k < sizeof tr; ++k) clean &= b[k] == 0x5a;
        EXPECT(clean);
    }
    Pair s;
    make_pair(s, 70, 5u, false);
    EXPECT(movba_init_map(nullptr, &s.d, &s.r, 1, nullptr) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_init_map(h, nullptr, &s.r, 1, nullptr) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_init_map(h, &s.d, nullptr, 1, nullptr) == MOVBA_ERR_ARG);
    EXPECT(movba_init_map(h, &s.d, &s.r, -1, nullptr) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_init_map(h, &s.d, &s.r, MOVBA_MAX_TWO_VIEW_BATCH + 1, nullptr) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_init_map(h, nullptr, nullptr, 0, nullptr) == MOVBA_OK);
    EXPECT(movba_init_map(h, &s.d, &s.r, 0, nullptr) == MOVBA_OK && s.r.status == 99 && untouched(s));
}

// a batch with pairs without a used match between solved ones, masks, information arrays, pinned arrays and a trace: every
// solved pair against its own solo call in the other layout
void batch(movba_handle *h, unsigned seed, bool with_trace)
{
    const int sizes[8] = { 150, 0, 49, 1, 260, 0, 50, 5 };
    const bool spread[8] = { true, false, false, true, false, true, true, false };
    Pair b[8], other[8];
    movba_init_map_desc ds[8];
    movba_init_map_result rs[8];
    movba_init_map_trace tr[9];
    std::memset(tr, 0x5a, sizeof tr);
    for (int k = 0; k < 8; ++k) {
        make_pair(b[k], sizes[k], seed + k, spread[k], k % 2 == 0);
        make_pair(other[k], sizes[k], seed + k, !spread[k], k % 2 == 0);
        ds[k] = b[k].d; rs[k] = b[k].r;
    }
    // pair 5: matches, but a mask of zeros
    std::fill(b[5].use.begin(), b[5].use.end(), 0);
    // pair 4's points and pair 6's chi2 in pinned memory
    double *pp = static_cast<double *>(movba_host_alloc(sizeof(double) * 3 * (size_t)b[4].n));
    double *pc = static_cast<double *>(movba_host_alloc(sizeof(double) * 2 * (size_t)b[6].n));
    EXPECT(pp && pc);
    if (!pp || !pc) return;
    rs[4].points = pp; rs[6].chi2 = pc;
    EXPECT(movba_init_map(h, ds, rs, 8, with_trace ? tr : nullptr) == MOVBA_OK);
    std::memcpy(b[4].out_pts.data(), pp, sizeof(double) * 3 * (size_t)b[4].n);
    std::memcpy(b[6].out_chi2.data(), pc, sizeof(double) * 2 * (size_t)b[6].n);
    for (int k = 0; k < 8; ++k) {
        b[k].r = rs[k];
        const bool empty = sizes[k] == 0 || k == 5;
        EXPECT(rs[k].status == (empty ? MOVBA_EMPTY : MOVBA_OK));
        if (with_trace) EXPECT(tr[k].n_trace == 0 && tr[k].pad == 0);
        if (empty) {
            EXPECT(rs[k].n_used == 0 && rs[k].outcome == MOVBA_IM_FEW_TRACKED && std::isnan(rs[k].median_depth) && rs[k].n_solves == 0);
            EXPECT(std::fabs(rs[k].pose[3] - 1.0) < 1e-5 && rs[k].pose[4] == -1.0);
            for (double v : b[k].out_pts) EXPECT(v == -7.0);
            for (double v : b[k].out_chi2) EXPECT(v == -7.0);
            continue;
        }
        EXPECT(rs[k].n_used == sizes[k] && rs[k].outcome == (sizes[k] < 50 ? MOVBA_IM_FEW_TRACKED : MOVBA_IM_OK));
        EXPECT(rs[k].median_depth > 4.0 && rs[k].cost == rs[k].cost0 && rs[k].cost > 0.0 && rs[k].pose[3] > 0.0);
        EXPECT(movba_init_map(h, &other[k].d, &other[k].r, 1, nullptr) == MOVBA_OK);
        EXPECT(same_used(b[k], other[k]));
    }
    EXPECT(tr[8].n_trace == 0x5a5a5a5a);         // (the entry behind the last is not the call's)
    movba_host_free(pp); movba_host_free(pc);
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

// an uploaded window, run, movba_init_map, downloaded, run again, downloaded: both downloads are what the fake device exports
void between_two_solves(movba_handle *h)
{
    Win w;
    make_window(w, 9, 600);
    Pair s;
    make_pair(s, 120, 9u, true);
    EXPECT(movba_lba_upload(h, &w.d) == MOVBA_OK);
    EXPECT(movba_init_map(h, &s.d, &s.r, 1, nullptr) == MOVBA_OK && s.r.n_used == 120);
    EXPECT(movba_lba_run(h) == MOVBA_OK);
    EXPECT(movba_init_map(h, &s.d, &s.r, 1, nullptr) == MOVBA_OK);
    for (int round = 0; round < 2; ++round) {
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK);
        EXPECT(w.r.n_solves == 10 && w.r.iters_done == 10 && w.out_poses[3] == 1.0 && w.out_points[0] == 1.0 && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0); std::fill(w.out_points.begin(), w.out_points.end(), 0.0);
        if (round == 0) {
            EXPECT(movba_lba_run(h) == MOVBA_OK);
            EXPECT(movba_init_map(h, &s.d, &s.r, 1, nullptr) == MOVBA_OK && s.r.status == MOVBA_OK);
        }
    }
}

}  // namespace

int main()
{
    movba_handle *h = nullptr;
    EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
    invalid_calls(h);
    for (int with_trace = 0; with_trace < 2; ++with_trace) batch(h, 11u + 20u * (unsigned)with_trace, with_trace != 0);
    between_two_solves(h);
    invalid_calls(h);
    movba_destroy(h);
    EXPECT(fake_init_map_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("init_map driver: ok\n");
    return 0;
}
