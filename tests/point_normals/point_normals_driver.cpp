// Drives the HOST side of movba_point_normals and movba_lba_point_normals (mov-slam_amd/csrc/point_normals.cpp) against the
// stand-in runtime and fake device of tests/hipstub and the fake launch of fake_point_normals.cpp, under AddressSanitizer +
// UndefinedBehaviorSanitizer or ThreadSanitizer.  The fake launch runs the library's own per-point arithmetic, so every value
// that comes back is checked against that arithmetic called here directly; what is under test is the host's side: every refusal
// of the header before anything is written (canaries), calls without points and without observations, pinned against ordinary
// result memory, the resident variant before an upload, before a run and after one - against the array variant fed the
// downloaded estimate and the caller-order lists, with and without flags, on edges given grouped and not - the window's
// downloads and runs around it, and two handles on two threads.  Exit code 0 and the last line "point_normals driver: ok" =
// every check held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"
#include "point_normals.h"

extern "C" int fake_point_normals_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

constexpr double kCanary = -7.0;

struct Call {
    std::vector<double> poses, points, scale;
    std::vector<int32_t> obs_ptr, obs_view, ref_view, ref_level;
    // results, each one entry longer than asked for: the canary behind the end
    std::vector<double> normals, dmax, dmin;
    movba_normals_desc d{};
    movba_normals_result r{};
    int np = 0, nv = 0;
};

void bind(Call &s)
{
    s.np = (int)s.ref_view.size(); s.nv = (int)(s.poses.size() / 7);
    s.normals.assign(3 * (size_t)s.np + 1, kCanary); s.dmax.assign((size_t)s.np + 1, kCanary); s.dmin.assign((size_t)s.np + 1, kCanary);
    s.d = movba_normals_desc{};
    s.d.n_views = s.nv; s.d.n_points = s.np; s.d.n_levels = (int32_t)s.scale.size(); s.d.pad = 55;
    s.d.poses = s.poses.data(); s.d.points = s.points.data(); s.d.obs_ptr = s.obs_ptr.data(); s.d.obs_view = s.obs_view.data();
    s.d.ref_view = s.ref_view.data(); s.d.ref_level = s.ref_level.data(); s.d.scale_factors = s.scale.data();
    s.r = movba_normals_result{};
    s.r.normals = s.normals.data(); s.r.max_distance = s.dmax.data(); s.r.min_distance = s.dmin.data(); s.r.status = 99; s.r.pad = 77;
}

// nv views near the origin, np points around them, lists of 1 .. max_len observers (every seventh point: none; its reference
// entry -1, which must not be read)
void make_call(Call &s, int nv, int np, int max_len, unsigned seed)
{
    std::mt19937 rng(seed);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(rng() % 100000) / 100000.0; };
    s.poses.clear(); s.points.clear(); s.obs_ptr.assign(1, 0); s.obs_view.clear(); s.ref_view.clear(); s.ref_level.clear();
    for (int v = 0; v < nv; ++v) {
        const double pose[7] = { uni(-0.3, 0.3), uni(-0.3, 0.3), uni(-0.3, 0.3), -1.5, uni(-2, 2), uni(-2, 2), uni(-2, 2) };
        s.poses.insert(s.poses.end(), pose, pose + 7);
    }
    s.scale.assign(8, 1.0);
    for (int k = 1; k < 8; ++k) s.scale[k] = s.scale[k - 1] * 1.2;
    for (int p = 0; p < np; ++p) {
        for (int k = 0; k < 3; ++k) s.points.push_back(uni(5, 15));
        const int len = (p % 7 == 3 || nv == 0 || max_len == 0) ? 0 : 1 + (int)(rng() % (unsigned)max_len);
        for (int k = 0; k < len; ++k) s.obs_view.push_back((int32_t)(rng() % (unsigned)nv));
        s.obs_ptr.push_back((int32_t)s.obs_view.size());
        s.ref_view.push_back(len ? (int32_t)(rng() % (unsigned)nv) : -1);
        s.ref_level.push_back((int32_t)(rng() % 8));
    }
    bind(s);
}

bool untouched(const Call &s)
{
    bool ok = s.r.pad == 77;
    for (const std::vector<double> *a : { &s.normals, &s.dmax, &s.dmin })
        for (double v : *a) ok &= v == kCanary;
    return ok;
}

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

// what came back (pinned or not) against the arithmetic called directly on the call's own arrays
void check(const Call &s, const double *normals, const double *dmax, const double *dmin)
{
    using namespace movba;
    std::vector<double> centres(3 * (size_t)s.nv);
    for (int v = 0; v < s.nv; ++v) pn_centre(&s.poses[7 * (size_t)v], &centres[3 * (size_t)v]);
    PnLists L{};
    L.ptr = s.obs_ptr.data(); L.view = s.obs_view.data();
    bool ok = true;
    for (int p = 0; p < s.np; ++p) {
        const PnPoint r = pn_point(&s.points[3 * (size_t)p], L, (size_t)p, centres.data(), s.ref_view[p], s.ref_level[p], s.scale.data(), (int32_t)s.scale.size());
        for (int k = 0; k < 3; ++k) ok &= same(normals[3 * (size_t)p + k], r.normal[k]);
        ok &= same(dmax[p], r.max_distance) && same(dmin[p], r.min_distance);
        if (s.obs_ptr[p + 1] == s.obs_ptr[p]) ok &= std::isnan(dmax[p]) && std::isnan(normals[3 * (size_t)p]);
    }
    EXPECT(ok);
}

void canaries_in_place(const Call &s)
{
    EXPECT(s.normals[3 * (size_t)s.np] == kCanary && s.dmax[s.np] == kCanary && s.dmin[s.np] == kCanary && s.r.pad == 77);
}

void run_call(movba_handle *h, int nv, int np, int max_len, unsigned seed, int variant)
{
    Call s;
    make_call(s, nv, np, max_len, seed);
    std::vector<void *> blocks;
    auto pin = [&](size_t bytes) { void *p = movba_host_alloc(bytes ? bytes : 8); EXPECT(p != nullptr); blocks.push_back(p); return static_cast<double *>(p); };
    movba_normals_result r = s.r;
    const size_t n = (size_t)np;
    if (variant == 1) { r.normals = pin(24 * n); r.max_distance = pin(8 * n); r.min_distance = pin(8 * n); }       // everything pinned
    else if (variant == 2) { r.max_distance = pin(8 * n); }                                                          // one of three
    for (void *p : blocks) if (!p) return;
    EXPECT(movba_point_normals(h, &s.d, &r) == MOVBA_OK && r.status == MOVBA_OK && r.pad == 77);
    check(s, r.normals, r.max_distance, r.min_distance);
    canaries_in_place(s);
    for (void *p : blocks) movba_host_free(p);
}

void growing_and_shrinking(movba_handle *h, unsigned seed)
{
    const int rounds[][3] = { { 3, 5, 2 }, { 40, 3000, 12 }, { 1, 1, 1 }, { 700, 50, 700 }, { 9, 20000, 6 }, { 2, 64, 3 }, { 300, 257, 300 }, { 5, 7, 0 } };
    int k = 0;
    for (const auto &q : rounds) { run_call(h, q[0], q[1], q[2], seed + k, k % 3); ++k; }
}

void invalid_calls(movba_handle *h)
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int which = 0; which < 29; ++which) {
        Call s;
        make_call(s, 12, 60, 9, 3u);
        movba_normals_desc &d = s.d;
        movba_normals_result &r = s.r;
        // (point 0 has observers: checked below)
        switch (which) {
        case 0: d.n_views = -1; break;
        case 1: d.n_points = -1; break;
        case 2: d.n_levels = -1; break;
        case 3: d.n_levels = 0; break;
        case 4: s.obs_ptr[0] = 1; break;
        case 5: s.obs_ptr[5] = s.obs_ptr[4] - 1; break;                  // descending
        case 6: s.obs_view[2] = 12; break;
        case 7: s.obs_view[0] = -1; break;
        case 8: s.ref_view[0] = 12; break;
        case 9: s.ref_view[0] = -1; break;
        case 10: s.ref_level[7] = 8; break;
        case 11: s.ref_level[3] = -1; break;                            // (the octave of a point without observers is checked too)
        case 12: s.scale[4] = 0.0; break;
        case 13: s.scale[0] = -1.0; break;
        case 14: s.scale[7] = inf; break;
        case 15: s.scale[2] = nan; break;
        case 16: s.poses[7 * 3 + 5] = nan; break;
        case 17: s.poses[2] = inf; break;
        case 18: s.poses[7] = s.poses[8] = s.poses[9] = s.poses[10] = 0.0; break;
        case 19: d.poses = nullptr; break;
        case 20: d.points = nullptr; break;
        case 21: d.obs_ptr = nullptr; break;
        case 22: d.obs_view = nullptr; break;
        case 23: d.ref_view = nullptr; break;
        case 24: d.ref_level = nullptr; break;
        case 25: d.scale_factors = nullptr; break;
        case 26: r.normals = nullptr; break;
        case 27: r.max_distance = nullptr; break;
        case 28: r.min_distance = nullptr; break;
        }
        EXPECT(s.obs_ptr[1] > s.obs_ptr[0] || which == 4);
        const int rc = movba_point_normals(h, &d, &r);
        if (rc != MOVBA_ERR_ARG || r.status != MOVBA_ERR_ARG || !untouched(s)) {
            std::fprintf(stderr, "invalid call %d not refused cleanly (rc %d)\n", which, rc);
            __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED);
        }
    }
    Call s;
    make_call(s, 10, 30, 5, 5u);
    EXPECT(movba_point_normals(nullptr, &s.d, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_point_normals(h, nullptr, &s.r) == MOVBA_ERR_ARG && s.r.status == 99);
    EXPECT(movba_point_normals(h, &s.d, nullptr) == MOVBA_ERR_ARG);
    // what is not wrong: a reference entry out of range on a point without observers (3, 10, 17, ... have none)
    s.ref_view[3] = 1000; s.ref_view[10] = -5;
    EXPECT(movba_point_normals(h, &s.d, &s.r) == MOVBA_OK && s.r.status == MOVBA_OK);
    check(s, s.normals.data(), s.dmax.data(), s.dmin.data());
    canaries_in_place(s);
    // no points: MOVBA_OK and nothing but the status written, whatever else the descriptor holds
    {
        Call e;
        make_call(e, 4, 10, 3, 8u);
        e.d.n_points = 0;
        EXPECT(movba_point_normals(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        e.r.status = 99;
        EXPECT(untouched(e));
        movba_normals_desc none{};
        movba_normals_result r0{};
        r0.status = 99;
        EXPECT(movba_point_normals(h, &none, &r0) == MOVBA_OK && r0.status == MOVBA_OK);
    }
    // points without a single observation: NaN everywhere, and the arrays nothing reads may be left out
    {
        Call e;
        make_call(e, 0, 6, 0, 9u);
        e.d.poses = nullptr; e.d.points = nullptr; e.d.obs_view = nullptr; e.d.ref_view = nullptr;
        EXPECT(movba_point_normals(h, &e.d, &e.r) == MOVBA_OK && e.r.status == MOVBA_OK);
        for (int p = 0; p < 6; ++p) EXPECT(std::isnan(e.normals[3 * p]) && std::isnan(e.normals[3 * p + 2]) && std::isnan(e.dmax[p]) && std::isnan(e.dmin[p]));
        canaries_in_place(e);
    }
}

struct Win {
    std::vector<double> poses, points, obs, isig, out_poses, out_points, out_chi2;
    std::vector<uint8_t> fixed, out_outlier;
    std::vector<int32_t> ep, el;
    movba_lba_desc d{};
    movba_lba_result r{};
};

// grouped: the edges as a flattened map gives them, point by point; otherwise shuffled (the upload then groups them, stably, and
// keeps the permutation)
void make_window(Win &w, int NP, int P, bool grouped, unsigned seed)
{
    std::mt19937 rng(seed);
    w.poses.assign(7 * (size_t)NP, 0.0); w.fixed.assign(NP, 0); w.points.resize(3 * (size_t)P);
    for (int i = 0; i < NP; ++i) { w.poses[7 * i + 3] = 1.0; w.poses[7 * i + 4] = 0.3 * i; w.poses[7 * i + 5] = 0.01 * (double)(rng() % 50); w.fixed[i] = i < 2; }
    for (double &x : w.points) x = 1.0 + 0.001 * (double)(rng() % 4000);
    for (int l = 0; l < P; ++l)
        for (int k = l % (NP - 2); k < l % (NP - 2) + 3; ++k) { w.ep.push_back(k); w.el.push_back(l); }
    const size_t E = w.ep.size();
    if (!grouped) {
        std::vector<int32_t> order(E);
        for (size_t e = 0; e < E; ++e) order[e] = (int32_t)e;
        std::shuffle(order.begin(), order.end(), rng);
        std::vector<int32_t> ep(E), el(E);
        for (size_t e = 0; e < E; ++e) { ep[e] = w.ep[order[e]]; el[e] = w.el[order[e]]; }
        w.ep = ep; w.el = el;
    }
    w.obs.assign(2 * E, 100.0); w.isig.assign(E, 1.0);
    w.d.n_poses = NP; w.d.n_points = P; w.d.n_edges = (int32_t)E;
    w.d.poses = w.poses.data(); w.d.pose_fixed = w.fixed.data(); w.d.points = w.points.data();
    w.d.edge_pose = w.ep.data(); w.d.edge_point = w.el.data(); w.d.obs = w.obs.data(); w.d.inv_sigma2 = w.isig.data();
    w.d.fx = w.d.fy = 320; w.d.cx = 320; w.d.cy = 240; w.d.huber_delta = 2.236; w.d.chi2_gate = 5.0; w.d.max_iters = 10; w.d.flags = MOVBA_FLAG_STALE_ERROR_QUIRK;
    w.out_poses.assign(7 * (size_t)NP, 0.0); w.out_points.assign(3 * (size_t)P, 0.0); w.out_chi2.assign(E, 0.0); w.out_outlier.assign(E, 9);
    w.r.poses = w.out_poses.data(); w.r.points = w.out_points.data(); w.r.chi2 = w.out_chi2.data(); w.r.outlier = w.out_outlier.data();
}

// the array call that the resident one must equal: the downloaded estimate and the window's edges as caller-order lists
void lists_of(const Win &w, const uint8_t *mask, const std::vector<int32_t> &ref_pose, const std::vector<int32_t> &ref_level, Call &s)
{
    const int P = w.d.n_points, E = w.d.n_edges;
    s.poses = w.out_poses; s.points = w.out_points;
    std::vector<std::vector<int32_t>> lists((size_t)P);
    for (int e = 0; e < E; ++e)
        if (!mask || !mask[e]) lists[(size_t)w.el[e]].push_back(w.ep[e]);
    s.obs_ptr.assign(1, 0); s.obs_view.clear();
    for (int l = 0; l < P; ++l) { s.obs_view.insert(s.obs_view.end(), lists[l].begin(), lists[l].end()); s.obs_ptr.push_back((int32_t)s.obs_view.size()); }
    s.ref_view = ref_pose; s.ref_level = ref_level;
    s.scale.assign(8, 1.0);
    for (int k = 1; k < 8; ++k) s.scale[k] = s.scale[k - 1] * 1.2;
    bind(s);
}

void resident(movba_handle *h, bool grouped, int reps, unsigned seed)
{
    Win w;
    const int NP = 9, P = 600;
    make_window(w, NP, P, grouped, seed);
    const size_t E = (size_t)w.d.n_edges;
    std::mt19937 rng(seed + 1);
    std::vector<int32_t> ref_pose(P), ref_level(P);
    for (int l = 0; l < P; ++l) { ref_pose[l] = (int32_t)(rng() % NP); ref_level[l] = (int32_t)(rng() % 8); }
    std::vector<uint8_t> mask(E);
    for (size_t e = 0; e < E; ++e) mask[e] = (w.el[e] % 5 == 0) || (rng() % 4 == 0);         // (every fifth point loses all its edges)
    std::vector<double> scale(8, 1.0);
    for (int k = 1; k < 8; ++k) scale[k] = scale[k - 1] * 1.2;
    std::vector<double> nrm(3 * (size_t)P + 1), mx((size_t)P + 1), mn((size_t)P + 1);
    auto reset = [&] { std::fill(nrm.begin(), nrm.end(), kCanary); std::fill(mx.begin(), mx.end(), kCanary); std::fill(mn.begin(), mn.end(), kCanary); };
    auto clean = [&] { bool ok = true; for (const std::vector<double> *a : { &nrm, &mx, &mn }) for (double v : *a) ok &= v == kCanary; return ok; };
    auto call = [&](const uint8_t *m, double *a, double *b, double *c) { return movba_lba_point_normals(h, ref_pose.data(), ref_level.data(), scale.data(), 8, m, a, b, c); };

    for (int rep = 0; rep < reps; ++rep) {
        reset();
        EXPECT(movba_lba_upload(h, &w.d) == MOVBA_OK);
        EXPECT(call(nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_STATE && clean());       // uploaded, not run
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        // the refusals, with a window to check against
        EXPECT(movba_lba_point_normals(nullptr, ref_pose.data(), ref_level.data(), scale.data(), 8, nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);
        EXPECT(movba_lba_point_normals(h, nullptr, ref_level.data(), scale.data(), 8, nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);
        EXPECT(movba_lba_point_normals(h, ref_pose.data(), nullptr, scale.data(), 8, nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);
        EXPECT(movba_lba_point_normals(h, ref_pose.data(), ref_level.data(), nullptr, 8, nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);
        EXPECT(movba_lba_point_normals(h, ref_pose.data(), ref_level.data(), scale.data(), 0, nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);
        EXPECT(movba_lba_point_normals(h, ref_pose.data(), ref_level.data(), scale.data(), 7, nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);   // (octave 7 exists)
        EXPECT(call(nullptr, nullptr, mx.data(), mn.data()) == MOVBA_ERR_ARG && call(nullptr, nrm.data(), nullptr, mn.data()) == MOVBA_ERR_ARG &&
               call(nullptr, nrm.data(), mx.data(), nullptr) == MOVBA_ERR_ARG);
        for (int which = 0; which < 5; ++which) {
            const int32_t keep_p = ref_pose[17], keep_l = ref_level[40];
            const double keep_s = scale[3];
            if (which == 0) ref_pose[17] = NP; else if (which == 1) ref_pose[17] = -1; else if (which == 2) ref_level[40] = 8;
            else if (which == 3) scale[3] = 0.0; else scale[3] = std::numeric_limits<double>::infinity();
            EXPECT(call(mask.data(), nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_ARG);
            ref_pose[17] = keep_p; ref_level[40] = keep_l; scale[3] = keep_s;
        }
        EXPECT(clean());

        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        for (int m = 0; m < 2; ++m) {
            const uint8_t *flags = m ? mask.data() : nullptr;
            Call s;
            lists_of(w, flags, ref_pose, ref_level, s);
            // ordinary memory, then pinned
            reset();
            EXPECT(call(flags, nrm.data(), mx.data(), mn.data()) == MOVBA_OK);
            check(s, nrm.data(), mx.data(), mn.data());
            EXPECT(nrm[3 * (size_t)P] == kCanary && mx[P] == kCanary && mn[P] == kCanary);
            if (m) for (int l = 0; l < P; l += 5) EXPECT(std::isnan(mx[l]) && std::isnan(nrm[3 * (size_t)l + 1]));
            double *pa = static_cast<double *>(movba_host_alloc(24 * (size_t)P)), *pb = static_cast<double *>(movba_host_alloc(8 * (size_t)P)),
                   *pc = static_cast<double *>(movba_host_alloc(8 * (size_t)P));
            EXPECT(pa && pb && pc);
            if (pa && pb && pc) {
                EXPECT(call(flags, pa, pb, pc) == MOVBA_OK);
                check(s, pa, pb, pc);
            }
            movba_host_free(pa); movba_host_free(pb); movba_host_free(pc);
            // ... and the array call itself on the same handle gives the same bits, and leaves the window where it was
            EXPECT(movba_point_normals(h, &s.d, &s.r) == MOVBA_OK);
            bool ok = true;
            for (size_t k = 0; k < 3 * (size_t)P; ++k) ok &= same(s.normals[k], nrm[k]);
            for (int l = 0; l < P; ++l) ok &= same(s.dmax[l], mx[l]) && same(s.dmin[l], mn[l]);
            EXPECT(ok);
        }
        // the window is still there: download again, run again, the call again
        std::fill(w.out_poses.begin(), w.out_poses.end(), 0.0);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10 && w.out_poses[3] == 1.0 && w.out_outlier[0] == 0 && w.out_chi2[0] == 1.0);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        EXPECT(call(mask.data(), nrm.data(), mx.data(), mn.data()) == MOVBA_OK);
        EXPECT(movba_lba_download(h, &w.r) == MOVBA_OK && w.r.n_solves == 10);
        EXPECT(movba_lba_reset(h) == MOVBA_OK);
        EXPECT(call(nullptr, nrm.data(), mx.data(), mn.data()) == MOVBA_ERR_STATE);                   // reset, not run
    }
}

}  // namespace

int main()
{
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        {
            double a[3], b[1], c[1];
            const int32_t z = 0;
            const double one = 1.0;
            EXPECT(movba_lba_point_normals(h, &z, &z, &one, 1, nullptr, a, b, c) == MOVBA_ERR_STATE);   // nothing uploaded
        }
        invalid_calls(h);
        growing_and_shrinking(h, 11u);
        resident(h, true, 2, 40u);
        resident(h, false, 1, 41u);
        invalid_calls(h);
        movba_destroy(h);
    }
    {
        auto pn_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            for (int it = 0; it < 2; ++it) growing_and_shrinking(h, seed + 100 * it);
            movba_destroy(h);
        };
        auto lba_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            resident(h, false, 2, seed);
            resident(h, true, 1, seed + 9);
            movba_destroy(h);
        };
        std::thread a(pn_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_point_normals_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("point_normals driver: ok\n");
    return 0;
}
