// movba_two_view and movba_two_view_lo (include/movba.h): monocular map initialisation for many frame pairs in one call, without
// and with the local optimisation of the winner; both are one front (two_view_front).  The device pass is two_view.hip (three
// kernels, and k_tv_lo for the refit); this file checks every descriptor, packs pairs + matches + samples into the handle's staging
// buffer, sends them with ONE copy, queues the launches and hands the results over after ONE synchronisation.  Per-match
// result arrays that lie in movba_host_alloc memory are written by the kernels themselves; others arrive in the staging
// buffer and are copied out.  The hypothesis tables (hyp_nsol / hyp_E / hyp_loss) stay in device scratch and are copied
// only for a caller that asks for them.  The refit's per-pair slots (TvDev::lo) exist only when a refit or `info` is asked
// for: they go up zero-filled with the inputs and come back with one copy more before the synchronisation.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"
#include "two_view.h"
#include "two_view_math.h"

using namespace movba;

namespace {

bool tv_desc_ok(const movba_two_view_desc &d, const movba_two_view_result &r)
{
    if (d.n_matches < 0 || d.n_matches > MOVBA_MAX_TWO_VIEW_MATCHES) return false;
    if (d.ransac_iters < 1 || d.ransac_iters > MOVBA_MAX_TWO_VIEW_ITERS) return false;
    if (!std::isfinite(d.fx) || !std::isfinite(d.fy) || !(d.fx > 0.0) || !(d.fy > 0.0)) return false;
    if (!std::isfinite(d.cx) || !std::isfinite(d.cy)) return false;
    if (!std::isfinite(d.threshold) || !(d.threshold > 0.0) || !std::isfinite(d.confidence)) return false;
    if (!std::isfinite(d.sigma) || d.sigma < 0.0 || !std::isfinite(d.min_parallax_deg)) return false;
    if (!std::isfinite(d.max_depth) || !(d.max_depth > 0.0) || d.min_triangulated < 0) return false;
    if (d.n_matches > 0 && (!d.obs1 || !d.obs2)) return false;
    if (d.n_matches >= 5 && (!r.inlier || !r.points || !r.good || !r.code)) return false;
    return true;
}

}  // namespace

extern "C" int movba_two_view_samples(int32_t n, int32_t n_hyp, uint32_t seed, int32_t *out)
{
    if (n < 5 || n_hyp < 0 || !out) return MOVBA_ERR_ARG;
    // the xorshift32 generator of movba_pose_ransac_samples on another stream
    uint32_t x = (seed ? seed : 0x9E3779B9u) ^ 0x85EBCA6Bu;
    if (!x) x = 0x85EBCA6Bu;
    auto next = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (int h = 0; h < n_hyp; ++h) {
        int32_t *s = out + 5 * (size_t)h;
        for (int k = 0; k < 5; ++k) {
            bool again;
            do {
                s[k] = (int32_t)(next() % (uint32_t)n);
                again = false;
                for (int j = 0; j < k; ++j) again |= s[j] == s[k];
            } while (again);
        }
    }
    return MOVBA_OK;
}

namespace {

int two_view_front(movba_handle *h, const movba_two_view_desc *descs, movba_two_view_result *results, int32_t n, int32_t lo_iters,
                   movba_two_view_lo_info *info)
{
    if (!h || n < 0 || n > MOVBA_MAX_TWO_VIEW_BATCH) return MOVBA_ERR_ARG;
    const bool lo_ok = lo_iters >= 0 && lo_iters <= MOVBA_MAX_TWO_VIEW_LO_ITERS;
    if (n == 0) return lo_ok ? MOVBA_OK : MOVBA_ERR_ARG;
    if (!descs || !results) return MOVBA_ERR_ARG;
    for (int k = 0; k < n; ++k)
        if (!lo_ok || !tv_desc_ok(descs[k], results[k])) {
            for (int j = 0; j < n; ++j) results[j].status = MOVBA_ERR_ARG;
            return MOVBA_ERR_ARG;
        }

    // totals over the pairs that are solved (5 matches or more)
    std::vector<TvPair> pairs((size_t)n);
    std::vector<int32_t> hyp_first((size_t)n + 1, 0);
    size_t M = 0, H = 0;
    for (int k = 0; k < n; ++k) {
        const movba_two_view_desc &d = descs[k];
        TvPair &p = pairs[k];
        std::memset(&p, 0, sizeof p);
        const bool solve = d.n_matches >= 5;
        p.n = solve ? d.n_matches : 0; p.n_hyp = solve ? d.ransac_iters : 0;
        p.m0 = (int32_t)M; p.h0 = (int32_t)H;
        p.min_tri = d.min_triangulated;
        p.f = 0.5 * (d.fx + d.fy); p.fx = d.fx; p.fy = d.fy; p.cx = d.cx; p.cy = d.cy;
        p.thr2 = d.threshold * d.threshold; p.conf = d.confidence; p.th2 = 4.0 * d.sigma * d.sigma;
        p.min_par = d.min_parallax_deg; p.max_depth = d.max_depth;
        hyp_first[k] = (int32_t)H;
        M += (size_t)p.n; H += (size_t)p.n_hyp;
    }
    hyp_first[n] = (int32_t)H;
    if (M > (size_t)1 << 28 || H > (size_t)1 << 22) {
        for (int j = 0; j < n; ++j) results[j].status = MOVBA_ERR_ARG;
        return MOVBA_ERR_ARG;
    }
    const size_t np = (size_t)n;

    // Device arena: [0, h2d) the inputs (one H2D copy), then scratch.  Staging buffer: the same inputs, then the results that
    // do not go straight into the caller's pinned arrays.
    Carver c;
    In<TvPair> in_pairs;
    In<int32_t> first, samp;
    In<double> obs1, obs2, lo;
    in_pairs.plan(np, c); first.plan(np + 1, c); obs1.plan(2 * M, c); obs2.plan(2 * M, c); samp.plan(5 * H, c);
    const bool want_lo = lo_iters > 0 || info;
    lo.plan(want_lo ? kTvLoDoubles * np : 0, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_cand = dv.take<double>(90 * H), o_loss = dv.take<double>(10 * H), o_cnt = dv.take<int32_t>(10 * H);
    const size_t o_nsol = dv.take<int32_t>(H), o_inl0 = dv.take<uint8_t>(M), o_cos = dv.take<double>(M);
    const size_t o_rec = dv.take<double>(kTvRecDoubles * np);
    const size_t dev_total = dv.off;
    const size_t o_out = c.take<double>(kTvOutDoubles * np);
    const size_t o_inl = c.take<uint8_t>(M), o_pts = c.take<double>(3 * M), o_good = c.take<uint8_t>(M), o_code = c.take<uint8_t>(M);
    const size_t total = c.off;

    for (int j = 0; j < n; ++j) results[j].status = MOVBA_ERR_HIP;      // (until the device work is through)
    int rc = begin_side_call(h, dev_total, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p, *sd = h->stage_dev;
    struct PairOut { Out<uint8_t> inl, good, code; Out<double> pts; };     // each pair's share of the per-match results
    std::vector<PairOut> outs(np);
    for (int k = 0; k < n; ++k) {
        const movba_two_view_desc &d = descs[k];
        movba_two_view_result &r = results[k];
        TvPair &p = pairs[k];
        const size_t m = (size_t)p.n, m0 = (size_t)p.m0;
        PairOut &v = outs[k];
        v.inl.plan_within(r.inlier, m, o_inl, m0); v.pts.plan_within(r.points, 3 * m, o_pts, 3 * m0);
        v.good.plan_within(r.good, m, o_good, m0); v.code.plan_within(r.code, m, o_code, m0);
        v.inl.bind(sd); v.pts.bind(sd); v.good.bind(sd); v.code.bind(sd);
        p.inlier = v.inl.dev; p.points = v.pts.dev; p.good = v.good.dev; p.code = v.code.dev;
        p.out = at<double>(sd, o_out) + (size_t)kTvOutDoubles * k;
        if (m) {
            std::copy_n(d.obs1, 2 * m, obs1.host(sg) + 2 * m0);
            std::copy_n(d.obs2, 2 * m, obs2.host(sg) + 2 * m0);
            (void)movba_two_view_samples(p.n, p.n_hyp, d.ransac_seed, samp.host(sg) + 5 * (size_t)p.h0);
        }
    }
    in_pairs.fill(sg, pairs.data()); first.fill(sg, hyp_first.data());
    std::fill_n(lo.host(sg), lo.count, 0.0);

    TvDev t{};
    t.n_pairs = n; t.n_hyp_total = (int32_t)H;
    t.pairs = in_pairs.dev(ar); t.hyp_first = first.dev(ar); t.obs1 = obs1.dev(ar); t.obs2 = obs2.dev(ar); t.samples = samp.dev(ar);
    t.cand = at<double>(ar, o_cand); t.loss = at<double>(ar, o_loss); t.cnt = at<int32_t>(ar, o_cnt); t.nsol = at<int32_t>(ar, o_nsol);
    t.inl0 = at<uint8_t>(ar, o_inl0); t.cosv = at<double>(ar, o_cos); t.rec = at<double>(ar, o_rec);
    t.lo = want_lo ? at<double>(ar, lo.off) : nullptr;      // (an input the refit writes back: not const)
    t.lo_iters = lo_iters;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_two_view(t, h->stream));
    if (want_lo) HIP_TRY(hipMemcpyAsync(sg + lo.off, ar + lo.off, sizeof(double) * lo.count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (int k = 0; k < n; ++k) {
        movba_two_view_result &r = results[k];
        const TvPair &p = pairs[k];
        const size_t m = (size_t)p.n;
        const PairOut &v = outs[k];
        v.inl.fetch(sg); v.pts.fetch(sg); v.good.fetch(sg); v.code.fetch(sg);
        const double *o = at<const double>(sg, o_out) + (size_t)kTvOutDoubles * k;
        for (int e = 0; e < 7; ++e) r.pose[e] = o[e];
        for (int e = 0; e < 9; ++e) r.E[e] = o[7 + e];
        r.parallax_deg = o[16]; r.outcome = (int32_t)o[17]; r.n_inliers = (int32_t)o[18]; r.n_pass = (int32_t)o[19];
        r.n_good = (int32_t)o[20]; r.samples_used = (int32_t)o[21];
        if (info) {
            // (a slot no kernel wrote - no winner, fewer than 5 matches - is still the zeros that went up)
            const double *l = lo.host(sg) + (size_t)kTvLoDoubles * k;
            movba_two_view_lo_info &fo = info[k];
            fo.loss0 = l[18]; fo.loss = l[19];
            for (int e = 0; e < 9; ++e) fo.E0[e] = l[9 + e];
            fo.kept = (int32_t)l[20]; fo.steps = (int32_t)l[21]; fo.n_inliers0 = (int32_t)l[22]; fo.pad = 0;
        }
        if (m) {
            const size_t nh = (size_t)p.n_hyp, h0 = (size_t)p.h0;
            if (r.hyp_nsol) HIP_TRY(hipMemcpy(r.hyp_nsol, ar + o_nsol + sizeof(int32_t) * h0, sizeof(int32_t) * nh, hipMemcpyDeviceToHost));
            if (r.hyp_E) HIP_TRY(hipMemcpy(r.hyp_E, ar + o_cand + sizeof(double) * 90 * h0, sizeof(double) * 90 * nh, hipMemcpyDeviceToHost));
            if (r.hyp_loss) HIP_TRY(hipMemcpy(r.hyp_loss, ar + o_loss + sizeof(double) * 10 * h0, sizeof(double) * 10 * nh, hipMemcpyDeviceToHost));
        }
    }
    for (int k = 0; k < n; ++k) results[k].status = pairs[k].n ? MOVBA_OK : MOVBA_EMPTY;
    return MOVBA_OK;
}

}  // namespace

extern "C" int movba_two_view(movba_handle *h, const movba_two_view_desc *descs, movba_two_view_result *results, int32_t n)
{
    return two_view_front(h, descs, results, n, 0, nullptr);
}

extern "C" int movba_two_view_lo(movba_handle *h, const movba_two_view_desc *descs, movba_two_view_result *results, int32_t n,
                                 int32_t lo_iters, movba_two_view_lo_info *info)
{
    return two_view_front(h, descs, results, n, lo_iters, info);
}
