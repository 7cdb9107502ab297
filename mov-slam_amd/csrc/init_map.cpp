// movba_init_map (include/movba.h): the two-keyframe bundle adjustment, median depth and rescaling behind movba_two_view for many
// frame pairs in one call.  The device pass is init_map.hip (one kernel, one workgroup per pair); this file checks every
// descriptor, packs pairs + matches into the handle's staging buffer (the mask and the information arrays a caller left NULL go
// up as ones), sends them with ONE copy, queues the launch and hands the results over after ONE synchronisation.  `points` and
// `chi2` that lie in movba_host_alloc memory are written by the kernel itself; others arrive in the staging buffer and are
// copied out.  A pair without a used match never reaches the device: its result is filled in here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "handle.h"
#include "init_map.h"

using namespace movba;

namespace {

bool im_desc_ok(const movba_init_map_desc &d, const movba_init_map_result &r)
{
    if (d.n_matches < 0 || d.n_matches > MOVBA_MAX_TWO_VIEW_MATCHES) return false;
    if (d.max_iters < 0 || d.max_iters > MOVBA_MAX_INIT_MAP_ITERS || d.max_trials < 0 || d.min_tracked < 0) return false;
    if (!std::isfinite(d.fx) || !std::isfinite(d.fy) || !(d.fx > 0.0) || !(d.fy > 0.0)) return false;
    if (!std::isfinite(d.cx) || !std::isfinite(d.cy) || !std::isfinite(d.huber_delta)) return false;
    for (int e = 0; e < 7; ++e)
        if (!std::isfinite(d.pose2[e])) return false;
    if (!(d.pose2[0] * d.pose2[0] + d.pose2[1] * d.pose2[1] + d.pose2[2] * d.pose2[2] + d.pose2[3] * d.pose2[3] > 0.0)) return false;
    if (d.n_matches > 0 && (!d.obs1 || !d.obs2 || !d.points || !r.points)) return false;
    return true;
}

// SE3Quat::normalizeRotation, as the kernel takes pose2 over (device_math.h: quat_normalize_exact)
void normalized_pose(const double in[7], double out[7])
{
    const double s = in[3] < 0.0 ? -1.0 : 1.0;
    const double n = std::sqrt(in[0] * in[0] + in[1] * in[1] + in[2] * in[2] + in[3] * in[3]);
    for (int e = 0; e < 4; ++e) out[e] = s * in[e] / n;
    for (int e = 4; e < 7; ++e) out[e] = in[e];
}

}  // namespace

extern "C" int movba_init_map(movba_handle *h, const movba_init_map_desc *descs, movba_init_map_result *results, int32_t n,
                              movba_init_map_trace *trace)
{
    if (!h || n < 0 || n > MOVBA_MAX_TWO_VIEW_BATCH) return MOVBA_ERR_ARG;
    if (n == 0) return MOVBA_OK;
    if (!descs || !results) return MOVBA_ERR_ARG;
    auto refuse = [&]() {
        for (int j = 0; j < n; ++j) results[j].status = MOVBA_ERR_ARG;
        return MOVBA_ERR_ARG;
    };
    size_t M = 0;
    for (int k = 0; k < n; ++k) {
        if (!im_desc_ok(descs[k], results[k])) return refuse();
        M += (size_t)descs[k].n_matches;
    }
    if (M > (size_t)1 << 28) return refuse();
    const size_t np = (size_t)n;

    // Staging buffer: [0, h2d) the inputs (one H2D copy), then the results that do not go straight into the caller's pinned
    // arrays.  The scratch behind the inputs on the device is sized by the used matches, which are only known once the masks
    // are staged: the staging buffer is laid out (and grown) first, the device arena after the count.
    Carver c;
    In<ImPair> in_pairs;
    In<double> obs1, obs2, pts, sig1, sig2;
    In<uint8_t> mask;
    in_pairs.plan(np, c);
    obs1.plan(2 * M, c); obs2.plan(2 * M, c); pts.plan(3 * M, c);
    sig1.plan(M, c); sig2.plan(M, c); mask.plan(M, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_out = c.take<double>(kImOutDoubles * np);
    const size_t o_trace = c.take<double>(trace ? kImTraceDoubles * np : 0);
    const size_t o_rpts = c.take<double>(3 * M), o_rchi = c.take<double>(2 * M);
    const size_t total = c.off;

    for (int j = 0; j < n; ++j) results[j].status = MOVBA_ERR_HIP;      // (until the device work is through)
    int rc = begin_side_call(h, 0, total); if (rc) return rc;

    char *sg = h->stage, *sd = h->stage_dev;
    std::vector<ImPair> pairs(np);
    struct PairOut { Out<double> pts, chi; };       // each pair's share of the per-match results
    std::vector<PairOut> outs(np);
    size_t m_at = 0, U = 0;
    for (int k = 0; k < n; ++k) {
        const movba_init_map_desc &d = descs[k];
        movba_init_map_result &r = results[k];
        ImPair &p = pairs[k];
        std::memset(&p, 0, sizeof p);
        const size_t m = (size_t)d.n_matches;
        uint8_t *use = mask.host(sg) + m_at;
        if (m) {
            std::copy_n(d.obs1, 2 * m, obs1.host(sg) + 2 * m_at);
            std::copy_n(d.obs2, 2 * m, obs2.host(sg) + 2 * m_at);
            std::copy_n(d.points, 3 * m, pts.host(sg) + 3 * m_at);
            double *s1 = sig1.host(sg) + m_at, *s2 = sig2.host(sg) + m_at;
            if (d.inv_sigma2_1) std::copy_n(d.inv_sigma2_1, m, s1); else std::fill_n(s1, m, 1.0);
            if (d.inv_sigma2_2) std::copy_n(d.inv_sigma2_2, m, s2); else std::fill_n(s2, m, 1.0);
            if (d.use) std::copy_n(d.use, m, use); else std::fill_n(use, m, uint8_t(1));
        }
        // (counted in the staged copy, which is what the kernel compacts: a caller that changes its mask meanwhile cannot make
        // the two disagree)
        size_t used = 0;
        for (size_t i = 0; i < m; ++i) used += use[i] != 0;
        p.n = used ? d.n_matches : 0; p.cap = (int32_t)used; p.m0 = (int32_t)m_at; p.s0 = (int64_t)U;
        p.max_iters = d.max_iters; p.max_trials = d.max_trials; p.min_tracked = d.min_tracked;
        for (int e = 0; e < 7; ++e) p.pose2[e] = d.pose2[e];
        p.fx = d.fx; p.fy = d.fy; p.cx = d.cx; p.cy = d.cy; p.huber = d.huber_delta;
        PairOut &v = outs[k];
        v.pts.plan_within(r.points, used ? 3 * m : 0, o_rpts, 3 * m_at); v.chi.plan_within(r.chi2, used ? 2 * m : 0, o_rchi, 2 * m_at);
        v.pts.bind(sd); v.chi.bind(sd);
        p.points = v.pts.dev; p.chi2 = v.chi.dev;       // (chi2 left out: nullptr, and the kernel skips it)
        p.out = at<double>(sd, o_out) + (size_t)kImOutDoubles * k;
        p.trace = trace ? at<double>(sd, o_trace) + (size_t)kImTraceDoubles * k : nullptr;
        m_at += m; U += used;
    }
    in_pairs.fill(sg, pairs.data());

    if (U) {
        const size_t o_idx = dv.take<int32_t>(U), o_X = dv.take<double>(3 * U), o_Xbk = dv.take<double>(3 * U);
        const size_t o_lin = dv.take<double>((size_t)kImLin * U);
        HIP_TRY(hipSetDevice(h->device));
        rc = h->pose_scratch.grow(h, dv.off); if (rc) return rc;
        char *ar = h->pose_scratch.p;
        ImDev t{};
        t.n_pairs = n;
        t.pairs = in_pairs.dev(ar);
        t.obs1 = obs1.dev(ar); t.obs2 = obs2.dev(ar); t.pts = pts.dev(ar);
        t.sig1 = sig1.dev(ar); t.sig2 = sig2.dev(ar); t.use = mask.dev(ar);
        t.idx = at<int32_t>(ar, o_idx); t.X = at<double>(ar, o_X);
        t.Xbk = at<double>(ar, o_Xbk); t.lin = at<double>(ar, o_lin);
        HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(launch_init_map(t, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }

    for (int k = 0; k < n; ++k) {
        movba_init_map_result &r = results[k];
        const ImPair &p = pairs[k];
        movba_init_map_trace *tr = trace ? trace + k : nullptr;
        if (!p.n) {
            normalized_pose(descs[k].pose2, r.pose);
            r.median_depth = std::numeric_limits<double>::quiet_NaN();
            r.lambda = r.cost0 = r.cost = 0.0;
            r.outcome = MOVBA_IM_FEW_TRACKED;
            r.n_used = r.iters_done = r.n_solves = r.last_rejected = r.n_chol_fail = r.pad = 0;
            if (tr) tr->n_trace = tr->pad = 0;
            continue;
        }
        outs[k].pts.fetch(sg); outs[k].chi.fetch(sg);
        const double *o = at<const double>(sg, o_out) + (size_t)kImOutDoubles * k;
        for (int e = 0; e < 7; ++e) r.pose[e] = o[e];
        r.median_depth = o[7]; r.outcome = (int32_t)o[8]; r.n_used = (int32_t)o[9]; r.iters_done = (int32_t)o[10];
        r.n_solves = (int32_t)o[11]; r.last_rejected = (int32_t)o[12]; r.n_chol_fail = (int32_t)o[13];
        r.lambda = o[14]; r.cost0 = o[15]; r.cost = o[16]; r.pad = 0;
        if (tr) {
            const double *t = at<const double>(sg, o_trace) + (size_t)kImTraceDoubles * k;
            const int nt = (int)t[0];
            tr->n_trace = nt; tr->pad = 0;
            for (int e = 0; e < nt; ++e) {
                tr->tr_lambda[e] = t[1 + e]; tr->tr_f0[e] = t[1 + MOVBA_MAX_TRACE + e]; tr->tr_f1[e] = t[1 + 2 * MOVBA_MAX_TRACE + e];
                tr->tr_rho[e] = t[1 + 3 * MOVBA_MAX_TRACE + e]; tr->tr_accept[e] = (int32_t)t[1 + 4 * MOVBA_MAX_TRACE + e];
            }
        }
    }
    for (int k = 0; k < n; ++k) results[k].status = pairs[k].n ? MOVBA_OK : MOVBA_EMPTY;
    return MOVBA_OK;
}
