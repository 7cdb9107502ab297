// Drives the HOST side of movba_covisibility (mov-slam_amd/csrc/covisibility.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_covisibility.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or
// ThreadSanitizer.  The fake launch runs the library's own per-query steps; every value that comes back is checked here against
// a std::map restatement of the reference's loop.  What is under test is the host's side: every refusal of the header before
// anything is written (canaries), calls without queries, optional arrays left out, pinned against ordinary result memory, calls
// of growing and shrinking size on one handle, a handle shared with an uploaded and a solved window whose downloads and runs go
// on around the calls, and two handles on two threads.  Exit code 0 and the last line "covisibility driver: ok" = every check
// held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_covisibility_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr int32_t kCanary = -77;

struct Call {
    std::vector<int32_t> obs_ptr, obs_view, query_ptr, query_point, query_self;
    std::vector<uint8_t> eligible;
    // results, each one entry longer than asked for: the canary behind the end
    std::vector<int32_t> n_counted, n_connected, best_view, best_weight, out_view, out_weight;
    movba_covis_desc d{};
    movba_covis_result r{};
    int nv = 0, np = 0, nq = 0, max_out = 0;
};

void bind(Call &s, int nv, int min_weight, int max_out)
{
    s.nv = nv; s.np = (int)s.obs_ptr.size() - 1; s.nq = (int)s.query_ptr.size() - 1; s.max_out = max_out;
    for (std::vector<int32_t> *a : { &s.n_counted, &s.n_connected, &s.best_view, &s.best_weight }) a->assign((size_t)s.nq + 1, kCanary);
    s.out_view.assign((size_t)s.nq * max_out + 1, kCanary); s.out_weight.assign((size_t)s.nq * max_out + 1, kCanary);
    s.d = movba_covis_desc{};
    s.d.n_views = nv; s.d.n_points = s.np; s.d.n_queries = s.nq; s.d.min_weight = min_weight; s.d.max_out = max_out; s.d.pad = 55;
    s.d.obs_ptr = s.obs_ptr.data(); s.d.obs_view = s.obs_view.data(); s.d.query_ptr = s.query_ptr.data(); s.d.query_point = s.query_point.data();
    s.d.query_self = s.query_self.empty() ? nullptr : s.query_self.data();
    s.d.eligible = s.eligible.empty() ? nullptr : s.eligible.data();
    s.r = movba_covis_result{};
    s.r.n_counted = s.n_counted.data(); s.r.n_connected = s.n_connected.data(); s.r.best_view = s.best_view.data(); s.r.best_weight = s.best_weight.data();
    s.r.out_view = s.out_view.data(); s.r.out_weight = s.out_weight.data(); s.r.status = 99; s.r.pad = 77;
}

// nv views, np points with lists of 0 .. max_len observers (duplicates allowed), nq queries of 0 .. max_items items (repeats
// allowed); optional: 0 neither self nor eligible, 1 both, 2 self only
void make_call(Call &s, int nv, int np, int max_len, int nq, int max_items, int min_weight, int max_out, int optional, unsigned seed)
{
    std::mt19937 rng(seed);
    s.obs_ptr.assign(1, 0); s.obs_view.clear(); s.query_ptr.assign(1, 0); s.query_point.clear(); s.query_self.clear(); s.eligible.clear();
    for (int p = 0; p < np; ++p) {
        const int len = (nv == 0 || p % 7 == 3) ? 0 : (int)(rng() % (unsigned)(max_len + 1));
        for (int k = 0; k < len; ++k) s.obs_view.push_back((int32_t)(rng() % (unsigned)nv));
        s.obs_ptr.push_back((int32_t)s.obs_view.size());
    }
    for (int q = 0; q < nq; ++q) {
        const int n = (np == 0 || q % 5 == 4) ? 0 : (int)(rng() % (unsigned)(max_items + 1));
        for (int k = 0; k < n; ++k) s.query_point.push_back((int32_t)(rng() % (unsigned)np));
        s.query_ptr.push_back((int32_t)s.query_point.size());
        if (optional) s.query_self.push_back(nv && q % 3 ? (int32_t)(rng() % (unsigned)nv) : -1);
    }
    if (optional == 1) for (int v = 0; v < nv; ++v) s.eligible.push_back(rng() % 8 != 0);
    bind(s, nv, min_weight, max_out);
}

bool untouched(const Call &s)
{
    bool ok = s.r.pad == 77;
    for (const std::vector<int32_t> *a : { &s.n_counted, &s.n_connected, &s.best_view, &s.best_weight, &s.out_view, &s.out_weight })
        for (int32_t v : *a) ok &= v == kCanary;
    return ok;
}

// what came back (pinned or not) against the loop as the reference writes it
void check(const Call &s, const movba_covis_result &r)
{
    bool ok = true;
    for (int q = 0; q < s.nq; ++q) {
        std::map<int32_t, int> counter;
        const int32_t self = s.query_self.empty() ? -1 : s.query_self[q];
        for (int32_t i = s.query_ptr[q]; i < s.query_ptr[q + 1]; ++i) {
            const int32_t p = s.query_point[i];
            for (int32_t k = s.obs_ptr[p]; k < s.obs_ptr[p + 1]; ++k) {
                const int32_t v = s.obs_view[k];
                if (v == self || (!s.eligible.empty() && !s.eligible[v])) continue;
                counter[v]++;
            }
        }
        int nmax = 0, vmax = -1, reaching = 0;
        std::vector<std::pair<int, int32_t>> pairs;
        for (const auto &kv : counter) {
            if (kv.second > nmax) { nmax = kv.second; vmax = kv.first; }
            reaching += kv.second >= s.d.min_weight;
            pairs.push_back({ kv.second, kv.first });
        }
        std::sort(pairs.begin(), pairs.end());
        std::reverse(pairs.begin(), pairs.end());
        ok &= r.n_counted[q] == (int32_t)counter.size() && r.best_view[q] == vmax && r.best_weight[q] == nmax;
        ok &= r.n_connected[q] == (counter.empty() ? 0 : reaching ? reaching : 1);
        for (int k = 0; k < s.max_out; ++k) {
            const bool in = k < (int)pairs.size();
            ok &= r.out_view[(size_t)q * s.max_out + k] == (in ? pairs[k].second : -1) && r.out_weight[(size_t)q * s.max_out + k] == (in ? pairs[k].first : 0);
        }
    }
    EXPECT(ok);
}

void canaries_in_place(const Call &s)
{
    EXPECT(s.n_counted[s.nq] == kCanary && s.n_connected[s.nq] == kCanary && s.best_view[s.nq] == kCanary && s.best_weight[s.nq] == kCanary);
    EXPECT(s.out_view[(size_t)s.nq * s.max_out] == kCanary && s.out_weight[(size_t)s.nq * s.max_out] == kCanary && s.r.pad == 77);
}

// variant 0: ordinary results, 1: all pinned, 2: the hand-out pinned, the scalars ordinary
void run_call(movba_handle *h, int nv, int np, int max_len, int nq, int max_items, int min_weight, int max_out, unsigned seed, int variant)
{
    Call s;
    make_call(s, nv, np, max_len, nq, max_items, min_weight, max_out, (int)(seed % 3), seed);
    std::vector<void *> blocks;
    auto pin = [&](size_t count) { void *p = movba_host_alloc(count ? 4 * count : 8); EXPECT(p != nullptr); blocks.push_back(p); return static_cast<int32_t *>(p); };
    movba_covis_result r = s.r;
    const size_t n_out = (size_t)nq * max_out;
    if (variant == 1) { r.n_counted = pin(nq); r.n_connected = pin(nq); r.best_view = pin(nq); r.best_weight = pin(nq); }
    if (variant >= 1) { r.out_view = pin(n_out); r.out_weight = pin(n_out); }
    for (void *p : blocks) if (!p) return;
    EXPECT(movba_covisibility(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK && r.pad == 77);
    check(s, r);
    if (variant == 0) canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_views, n_points, longest list, n_queries, most items, min_weight, max_out
    const int rounds[][7] = { { 5, 9, 3, 2, 4, 15, 5 }, { 300, 2000, 12, 40, 1500, 15, 30 }, { 1, 1, 1, 1, 1, 1, 1 }, { 8192, 40, 8192, 3, 60, 15, 8192 },
                              { 60, 20000, 6, 64, 2000, 15, 0 }, { 7, 3, 20, 4096, 2, 2, 3 }, { 0, 5, 0, 3, 4, 15, 2 }, { 500, 0, 0, 6, 0, 15, 4 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], q[3], q[4], q[5], q[6], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 33; ++which) {
        Call s;
        make_call(s, 12, 60, 9, 10, 30, 15, 6, 1, 3u);
        movba_covis_desc &d = s.d;
        movba_covis_result &r = s.r;
        switch (which) {
        case 0: d.n_views = -1; break;
        case 1: d.n_points = -1; break;
        case 2: d.n_queries = -1; break;
        case 3: d.max_out = -1; break;
        case 4: d.n_views = MOVBA_MAX_COVIS_VIEWS + 1; break;
        case 5: d.n_queries = MOVBA_MAX_COVIS_QUERIES + 1; break;
        case 6: d.min_weight = 0; break;
        case 7: d.min_weight = -15; break;
        case 8: d.max_out = (1 << 28) / 10 + 1; break;                   // n_queries x max_out above 2^28
        case 9: s.obs_ptr[0] = 1; break;
        case 10: s.obs_ptr[5] = s.obs_ptr[4] - 1; break;                 // descending
        case 11: for (size_t k = 1; k < s.obs_ptr.size(); ++k) s.obs_ptr[k] = (1 << 28) + 1; break;    // n_obs above 2^28: nothing behind it is read
        case 12: s.query_ptr[0] = 1; break;
        case 13: s.query_ptr[3] = s.query_ptr[2] - 1; break;
        case 14: for (size_t k = 1; k < s.query_ptr.size(); ++k) s.query_ptr[k] = (1 << 28) + 1; break;
        case 15: s.obs_view[2] = 12; break;
        case 16: s.obs_view[0] = -1; break;
        case 17: s.query_point[1] = 60; break;
        case 18: s.query_point[0] = -1; break;
        case 19: s.query_self[1] = 12; break;
        case 20: s.query_self[2] = -2; break;
        case 21: d.obs_ptr = nullptr; break;
        case 22: d.obs_view = nullptr; break;
        case 23: d.query_ptr = nullptr; break;
        case 24: d.query_point = nullptr; break;
        case 25: r.n_counted = nullptr; break;
        case 26: r.n_connected = nullptr; break;
        case 27: r.best_view = nullptr; break;
        case 28: r.best_weight = nullptr; break;
        case 29: r.out_view = nullptr; break;
        case 30: r.out_weight = nullptr; break;
        case 31: d.n_points = *std::max_element(s.query_point.begin(), s.query_point.end()); break;    // (an item names the point behind the last)
        case 32: d.n_views = *std::max_element(s.obs_view.begin(), s.obs_view.end()); break;           // (a list names the view behind the last)
        }
        const int rc = movba_covisibility(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, 10, 30, 5, 4, 12, 15, 10, 1, 5u);
    EXPECT(movba_covisibility(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_covisibility(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_covisibility(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    // what is not wrong: the optional arrays left out, and no hand-out at all
    s.d.eligible = nullptr; s.eligible.clear();
    EXPECT(movba_covisibility(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    s.d.query_self = nullptr; s.query_self.clear();
    EXPECT(movba_covisibility(h, &s.d, &s.r) == MOVBA_OK);
    check(s, s.r);
    canaries_in_place(s);
    {
        Call e;
        make_call(e, 10, 30, 5, 4, 12, 15, 0, 1, 6u);
        e.r.out_view = nullptr; e.r.out_weight = nullptr;
        EXPECT(movba_covisibility(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        check(e, e.r);
    }
    // no queries: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    {
        Call e;
        make_call(e, 4, 10, 3, 5, 3, 15, 4, 1, 8u);
        e.d.n_queries = 0;
        EXPECT(movba_covisibility(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        e.r.status = 99;
        EXPECT(untouched(e));
        movba_covis_desc none{};
        none.min_weight = 15;
        movba_covis_result r0{};
        r0.status = 99;
        EXPECT(movba_covisibility(h, &none, &r0) == MOVBA_OK && r0.status == MOVBA_OK);
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
        run_call(h, 40, 500, 9, 12, 300, 15, 40, seed + 1, rep % 3);                 // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, 300, 900, 20, 30, 700, 15, 10, seed + 2, (rep + 1) % 3);         // solved, not downloaded
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        const std::vector<double> first = w.out_poses;
        run_call(h, 2000, 300, 2000, 5, 100, 15, 2000, seed + 3, (rep + 2) % 3);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        run_call(h, 9, 50, 4, 3, 20, 15, 9, seed + 4, 0);
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
        auto cv_thread = [](unsigned seed) {
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
        std::thread a(cv_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_covisibility_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("covisibility driver: ok\n");
    return 0;
}
