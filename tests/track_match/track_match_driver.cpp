// Drives the HOST side of movba_track_match (mov-slam_amd/csrc/track_match.cpp) against the stand-in runtime and fake device of
// tests/hipstub and the fake launch of fake_track_match.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer or
// ThreadSanitizer.  The fake launch runs the library's own steps; every value that comes back is checked here against the double
// loop (a std::map of first slots where the loop would be long) and a std::map filled in slot order, as the reference writes them.  What is under test is the host's side: every refusal of
// the header before anything is written (canaries), calls without queries, optional arrays left out, pinned against ordinary
// result memory, calls of growing and shrinking size on one handle, a handle shared with an uploaded and a solved window whose
// downloads and runs go on around the calls, and two handles on two threads.  Exit code 0 and the last line "track_match driver:
// ok" = every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_track_match_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr int32_t kCanary = -77;
constexpr double kCanaryD = -77.5;

struct Call {
    std::vector<int32_t> view_ptr, slot_track, query_mode, query_view, query_ptr, item_track;
    std::vector<uint8_t> slot_taken;
    std::vector<double> slot_obs, slot_ur, slot_depth;
    // results, each one entry longer than asked for: the canary behind the end
    std::vector<int32_t> pair_ptr, slot1, slot2, item_slot, n_found;
    std::vector<double> obs1, obs2, ur1, ur2, depth1, depth2;
    movba_track_desc d{};
    movba_track_result r{};
    int nv = 0, nq = 0, cap = 0, n_items = 0;
};

int slots_of(const Call &s, int v) { return s.view_ptr[v + 1] - s.view_ptr[v]; }

void bind(Call &s)
{
    s.nv = (int)s.view_ptr.size() - 1; s.nq = (int)s.query_mode.size(); s.n_items = (int)s.item_track.size();
    s.cap = 0;
    for (int q = 0; q < s.nq; ++q)
        if (s.query_mode[q] == MOVBA_TM_TRIANGULATION) s.cap += slots_of(s, s.query_view[2 * q]);
    s.pair_ptr.assign((size_t)s.nq + 2, kCanary); s.slot1.assign((size_t)s.cap + 1, kCanary); s.slot2.assign((size_t)s.cap + 1, kCanary);
    s.item_slot.assign((size_t)s.n_items + 1, kCanary); s.n_found.assign((size_t)s.nq + 1, kCanary);
    s.obs1.assign(2 * (size_t)s.cap + 1, kCanaryD); s.obs2 = s.obs1;
    s.ur1.assign((size_t)s.cap + 1, kCanaryD); s.ur2 = s.ur1; s.depth1 = s.ur1; s.depth2 = s.ur1;
    s.d = movba_track_desc{};
    s.d.n_views = s.nv; s.d.n_queries = s.nq;
    s.d.view_ptr = s.view_ptr.data(); s.d.slot_track = s.slot_track.data(); s.d.slot_taken = s.slot_taken.empty() ? nullptr : s.slot_taken.data();
    s.d.slot_obs = s.slot_obs.empty() ? nullptr : s.slot_obs.data(); s.d.slot_ur = s.slot_ur.empty() ? nullptr : s.slot_ur.data();
    s.d.slot_depth = s.slot_depth.empty() ? nullptr : s.slot_depth.data();
    s.d.query_mode = s.query_mode.data(); s.d.query_view = s.query_view.data(); s.d.query_ptr = s.query_ptr.data(); s.d.item_track = s.item_track.data();
    s.r = movba_track_result{};
    s.r.pair_ptr = s.pair_ptr.data(); s.r.match_slot1 = s.slot1.data(); s.r.match_slot2 = s.slot2.data(); s.r.item_slot = s.item_slot.data();
    s.r.n_found = s.n_found.data();
    if (s.d.slot_obs) { s.r.obs1 = s.obs1.data(); s.r.obs2 = s.obs2.data(); }
    if (s.d.slot_ur) { s.r.ur1 = s.ur1.data(); s.r.ur2 = s.ur2.data(); }
    if (s.d.slot_depth) { s.r.depth1 = s.depth1.data(); s.r.depth2 = s.depth2.data(); }
    s.r.n_matches = 4242; s.r.status = 99;
}

// nv views of 0 .. max_slots slots (every fifth empty, the last one at max_slots), ids from a pool of the view's size (repeats),
// nq queries of both modes, lookups of 0 .. max_items items; optional: 0 no taken and no payload, 1 everything, 2 taken and obs only
void make_call(Call &s, int nv, int max_slots, int nq, int max_items, int optional, unsigned seed)
{
    std::mt19937 rng(seed);
    s = Call{};
    s.view_ptr.assign(1, 0);
    for (int v = 0; v < nv; ++v) {
        const int n = v == nv - 1 ? max_slots : v % 5 == 3 ? 0 : (int)(rng() % (unsigned)(max_slots + 1));
        for (int k = 0; k < n; ++k) {
            s.slot_track.push_back((int32_t)(rng() % (unsigned)(n + 1)) - n / 2);
            if (optional) s.slot_taken.push_back(rng() % 3 == 0);
            if (optional) { s.slot_obs.push_back(0.5 * (double)(rng() % 100000)); s.slot_obs.push_back(-0.25 * (double)(rng() % 100000)); }
            if (optional == 1) { s.slot_ur.push_back(k % 7 ? (double)(rng() % 640) : -1.0); s.slot_depth.push_back(std::nan(k % 2 ? "5" : "9")); }
        }
        s.view_ptr.push_back((int32_t)s.slot_track.size());
    }
    // (a payload that is asked for but has no slot to come from still needs an address)
    if (optional && s.slot_obs.empty()) { s.slot_obs.assign(2, 0.0); s.slot_taken.assign(1, 0); }
    if (optional == 1 && s.slot_ur.empty()) { s.slot_ur.assign(1, 0.0); s.slot_depth.assign(1, 0.0); }
    s.query_ptr.assign(1, 0);
    for (int q = 0; q < nq; ++q) {
        const int mode = q % 3 == 2 ? MOVBA_TM_LOOKUP : MOVBA_TM_TRIANGULATION;
        const int v2 = (int)(rng() % (unsigned)nv), v1 = q % 4 == 0 ? v2 : (int)(rng() % (unsigned)nv);
        s.query_mode.push_back(mode);
        s.query_view.push_back(mode == MOVBA_TM_LOOKUP ? -1 : v1); s.query_view.push_back(v2);
        if (mode == MOVBA_TM_LOOKUP && q % 5 != 4) {
            const int n = (int)(rng() % (unsigned)(max_items + 1)), n2 = slots_of(s, v2);
            for (int k = 0; k < n; ++k) s.item_track.push_back((int32_t)(rng() % (unsigned)(n2 + 2)) - n2 / 2);
        }
        s.query_ptr.push_back((int32_t)s.item_track.size());
    }
    bind(s);
}

bool untouched(const Call &s)
{
    bool ok = s.r.n_matches == 4242;
    for (const std::vector<int32_t> *a : { &s.pair_ptr, &s.slot1, &s.slot2, &s.item_slot, &s.n_found })
        for (int32_t v : *a) ok &= v == kCanary;
    for (const std::vector<double> *a : { &s.obs1, &s.obs2, &s.ur1, &s.ur2, &s.depth1, &s.depth2 })
        for (double v : *a) ok &= v == kCanaryD;
    return ok;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// what came back (pinned or not) against the loops as the reference writes them
void check(const Call &s, const movba_track_result &r)
{
    bool ok = r.pair_ptr[0] == 0;
    int at = 0;
    for (int q = 0; q < s.nq; ++q) {
        const int v1 = s.query_view[2 * q], v2 = s.query_view[2 * q + 1], b2 = s.view_ptr[v2], n2 = slots_of(s, v2);
        if (s.query_mode[q] == MOVBA_TM_LOOKUP) {
            std::map<int32_t, int> first;
            for (int j = 0; j < n2; ++j) first.insert({ s.slot_track[b2 + j], j });
            int found = 0;
            for (int i = s.query_ptr[q]; i < s.query_ptr[q + 1]; ++i) {
                const auto it = first.find(s.item_track[i]);
                ok &= r.item_slot[i] == (it == first.end() ? -1 : it->second);
                found += it != first.end();
            }
            ok &= r.n_found[q] == found;
        } else {
            const int b1 = s.view_ptr[v1], n1 = slots_of(s, v1);
            // the double loop itself where it is short; beyond 2^20 comparisons the free slots of view 2 in a map filled in slot
            // order, the first insertion kept - the slot the inner loop's `break` stops at
            const bool literal = (long long)n1 * n2 <= (1 << 20);
            std::map<int32_t, int> first;
            if (!literal)
                for (int j = 0; j < n2; ++j)
                    if (s.slot_taken.empty() || !s.slot_taken[b2 + j]) first.insert({ s.slot_track[b2 + j], j });
            for (int i = 0; i < n1; ++i) {
                if (!s.slot_taken.empty() && s.slot_taken[b1 + i]) continue;
                int j = -1;
                if (literal) {
                    for (int k = 0; k < n2 && j < 0; ++k)
                        if ((s.slot_taken.empty() || !s.slot_taken[b2 + k]) && s.slot_track[b1 + i] == s.slot_track[b2 + k]) j = k;
                } else {
                    const auto it = first.find(s.slot_track[b1 + i]);
                    if (it != first.end()) j = it->second;
                }
                if (j < 0) continue;
                ok &= at < s.cap && r.match_slot1[at] == i && r.match_slot2[at] == j;
                if (at < s.cap) {
                    if (r.obs1) ok &= same_bits(r.obs1[2 * at], s.slot_obs[2 * (b1 + i)]) && same_bits(r.obs1[2 * at + 1], s.slot_obs[2 * (b1 + i) + 1]);
                    if (r.obs2) ok &= same_bits(r.obs2[2 * at], s.slot_obs[2 * (b2 + j)]) && same_bits(r.obs2[2 * at + 1], s.slot_obs[2 * (b2 + j) + 1]);
                    if (r.ur1) ok &= same_bits(r.ur1[at], s.slot_ur[b1 + i]);
                    if (r.ur2) ok &= same_bits(r.ur2[at], s.slot_ur[b2 + j]);
                    if (r.depth1) ok &= same_bits(r.depth1[at], s.slot_depth[b1 + i]);
                    if (r.depth2) ok &= same_bits(r.depth2[at], s.slot_depth[b2 + j]);
                }
                ++at;
            }
            ok &= r.n_found[q] == 0;
        }
        ok &= r.pair_ptr[q + 1] == at;
    }
    ok &= r.n_matches == at;
    for (int k = at; k < s.cap; ++k) {
        ok &= r.match_slot1[k] == -1 && r.match_slot2[k] == -1;
        if (r.obs1) ok &= std::isnan(r.obs1[2 * k]) && std::isnan(r.obs1[2 * k + 1]);
        if (r.obs2) ok &= std::isnan(r.obs2[2 * k]) && std::isnan(r.obs2[2 * k + 1]);
        for (const double *a : { r.ur1, r.ur2, r.depth1, r.depth2 }) if (a) ok &= std::isnan(a[k]);
    }
    EXPECT(ok);
}

void canaries_in_place(const Call &s)
{
    EXPECT(s.pair_ptr[s.nq + 1] == kCanary && s.slot1[s.cap] == kCanary && s.slot2[s.cap] == kCanary && s.item_slot[s.n_items] == kCanary && s.n_found[s.nq] == kCanary);
    EXPECT(s.obs1[2 * (size_t)s.cap] == kCanaryD && s.obs2[2 * (size_t)s.cap] == kCanaryD && s.ur1[s.cap] == kCanaryD && s.ur2[s.cap] == kCanaryD);
    EXPECT(s.depth1[s.cap] == kCanaryD && s.depth2[s.cap] == kCanaryD);
}

// variant 0: ordinary results, 1: all pinned, 2: the matches and their payload pinned, the rest ordinary
void run_call(movba_handle *h, int nv, int max_slots, int nq, int max_items, unsigned seed, int variant)
{
    Call s;
    make_call(s, nv, max_slots, nq, max_items, (int)(seed % 3), seed);
    std::vector<void *> blocks;
    auto pin = [&](size_t bytes) { void *p = movba_host_alloc(bytes ? bytes : 8); EXPECT(p != nullptr); blocks.push_back(p); return p; };
    movba_track_result r = s.r;
    const size_t cap = (size_t)s.cap;
    if (variant == 1) { r.pair_ptr = (int32_t *)pin(4 * ((size_t)s.nq + 1)); r.item_slot = (int32_t *)pin(4 * (size_t)s.n_items); r.n_found = (int32_t *)pin(4 * (size_t)s.nq); }
    if (variant >= 1) {
        r.match_slot1 = (int32_t *)pin(4 * cap); r.match_slot2 = (int32_t *)pin(4 * cap);
        if (r.obs1) { r.obs1 = (double *)pin(16 * cap); r.obs2 = (double *)pin(16 * cap); }
        if (r.ur1) { r.ur1 = (double *)pin(8 * cap); r.depth2 = (double *)pin(8 * cap); }
    }
    for (void *p : blocks) if (!p) return;
    EXPECT(movba_track_match(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK);
    check(s, r);
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    // n_views, most slots of a view, n_queries, most items of a lookup
    const int rounds[][4] = { { 3, 9, 4, 5 }, { 12, 700, 40, 900 }, { 1, 1, 1, 1 }, { 2, MOVBA_MAX_TRACK_SLOTS, 5, 3000 }, { 40, 65, 600, 20 },
                              { 5, 0, 7, 4 }, { 6, 120, MOVBA_MAX_TRACK_QUERIES, 2 }, { 4, 257, 9, 0 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], q[3], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    for (int which = 0; which < 30; ++which) {
        Call s;
        make_call(s, 6, 40, 12, 30, 1, 4u);
        EXPECT(s.query_ptr[3] > 0 && s.cap > 0);         // (the cases below count on a lookup with items and on matches to hold)
        movba_track_desc &d = s.d;
        movba_track_result &r = s.r;
        // (queries 0, 1, 3, 4 ... are TRIANGULATION, 2, 5, 8, 11 LOOKUP; 2 and 5 have items)
        switch (which) {
        case 0: d.n_views = -1; break;
        case 1: d.n_queries = -1; break;
        case 2: d.n_queries = MOVBA_MAX_TRACK_QUERIES + 1; break;
        case 3: s.view_ptr[0] = 1; break;
        case 4: s.view_ptr[3] = s.view_ptr[2] - 1; break;                // descending
        case 5: for (size_t k = 1; k < s.view_ptr.size(); ++k) s.view_ptr[k] = (1 << 28) + 1; break;      // n_slots above 2^28: nothing behind it is read
        case 6: for (size_t k = 1; k < s.view_ptr.size(); ++k) s.view_ptr[k] = MOVBA_MAX_TRACK_SLOTS + 1; break;  // one view above the bound
        case 7: s.query_ptr[0] = 1; break;
        case 8: s.query_ptr[3] = s.query_ptr[2] - 1; break;
        case 9: for (size_t k = 1; k < s.query_ptr.size(); ++k) s.query_ptr[k] = (1 << 28) + 1; break;
        case 10: s.query_mode[1] = 2; break;
        case 11: s.query_mode[0] = -1; break;
        case 12: s.query_view[3] = 6; break;                             // view 2 out of range
        case 13: s.query_view[2] = -1; break;                            // view 1 of a TRIANGULATION query
        case 14: s.query_view[2] = 6; break;
        case 15: s.query_view[4] = 0; break;                             // a LOOKUP query whose first view is not -1
        case 16: s.query_view[5] = -1; break;                            // ... whose searched view is
        case 17: s.query_mode[2] = MOVBA_TM_TRIANGULATION; s.query_view[4] = 0; break;     // a TRIANGULATION query with items
        case 18: d.view_ptr = nullptr; break;
        case 19: d.slot_track = nullptr; break;
        case 20: d.query_mode = nullptr; break;
        case 21: d.query_view = nullptr; break;
        case 22: d.query_ptr = nullptr; break;
        case 23: d.item_track = nullptr; break;
        case 24: r.pair_ptr = nullptr; break;
        case 25: r.match_slot1 = nullptr; break;
        case 26: r.match_slot2 = nullptr; break;
        case 27: r.item_slot = nullptr; break;
        case 28: r.n_found = nullptr; break;
        case 29: d.slot_ur = nullptr; break;                             // ur1 / ur2 given without their source
        }
        const int rc = movba_track_match(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, 5, 30, 9, 12, 1, 5u);
    EXPECT(movba_track_match(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_track_match(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_track_match(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    EXPECT(untouched(s));
    // what is not wrong: a source without its outputs, one output of two, no taken array
    s.r.ur1 = nullptr; s.r.depth1 = nullptr; s.r.depth2 = nullptr; s.r.obs2 = nullptr;
    EXPECT(movba_track_match(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.r);
    s.d.slot_taken = nullptr; s.slot_taken.clear();
    EXPECT(movba_track_match(h, &s.d, &s.r) == MOVBA_OK);
    check(s, s.r);
    for (double v : s.ur1) EXPECT(v == kCanaryD);
    for (double v : s.obs2) EXPECT(v == kCanaryD);
    // no queries: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    {
        Call e;
        make_call(e, 4, 10, 5, 3, 1, 8u);
        e.d.n_queries = 0;
        EXPECT(movba_track_match(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        EXPECT(untouched(e));
        movba_track_desc none{};
        movba_track_result r0{};
        r0.status = 99;
        EXPECT(movba_track_match(h, &none, &r0) == MOVBA_OK && r0.status == MOVBA_OK);
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
        run_call(h, 8, 300, 12, 200, seed + 1, rep % 3);                         // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        run_call(h, 31, 900, 30, 700, seed + 2, (rep + 1) % 3);                  // solved, not downloaded
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        const std::vector<double> first = w.out_poses;
        run_call(h, 3, 4000, 5, 100, seed + 3, (rep + 2) % 3);
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses == first && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        run_call(h, 4, 50, 3, 20, seed + 4, 0);
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
        auto tm_thread = [](unsigned seed) {
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
        std::thread a(tm_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_track_match_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("track_match driver: ok\n");
    return 0;
}
