// movba_point_normals and movba_lba_point_normals (include/movba.h): the numeric body of MapPoint::UpdateNormalAndDepth for
// many map points per call - given as arrays, or read out of the window a run left resident on the device.  The device pass is
// point_normals.hip (two kernels, one per-point function for both entry points: point_normals.h); this file checks the calls,
// packs what has to cross the bus into the handle's staging buffer, sends it with ONE copy, queues the TWO launches and hands
// the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are written by the kernels
// themselves; others arrive in the staging buffer and are copied out.
#include <cmath>
#include <cstring>

#include "handle.h"
#include "point_normals.h"

using namespace movba;

namespace {

constexpr int32_t kPnMaxObs = 1 << 28;

// n_levels, the table and every point's octave: what both entry points take as they are
bool pn_levels_ok(int32_t n_levels, const double *scale, const int32_t *ref_level, size_t np)
{
    if (n_levels < 1 || !scale || !ref_level) return false;
    for (int32_t k = 0; k < n_levels; ++k)
        if (!(scale[k] > 0.0) || !std::isfinite(scale[k])) return false;
    for (size_t p = 0; p < np; ++p)
        if (ref_level[p] < 0 || ref_level[p] >= n_levels) return false;
    return true;
}

// everything about the call that can be wrong, checked before anything is queued or written
bool pn_desc_ok(const movba_normals_desc &d, const movba_normals_result &r)
{
    if (d.n_views < 0 || d.n_points < 0 || d.n_levels < 0) return false;
    if (d.n_points == 0) return true;
    const size_t np = (size_t)d.n_points, nv = (size_t)d.n_views;
    if (!d.obs_ptr || !r.normals || !r.max_distance || !r.min_distance) return false;
    if (d.obs_ptr[0] != 0) return false;
    for (size_t p = 0; p < np; ++p)
        if (d.obs_ptr[p + 1] < d.obs_ptr[p]) return false;
    const int32_t n_obs = d.obs_ptr[np];
    if (n_obs > kPnMaxObs) return false;
    if (!pn_levels_ok(d.n_levels, d.scale_factors, d.ref_level, np)) return false;
    if (nv) {
        if (!d.poses) return false;
        for (size_t v = 0; v < nv; ++v) {
            const double *q = d.poses + 7 * v;
            for (int e = 0; e < 7; ++e)
                if (!std::isfinite(q[e])) return false;
            if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return false;
        }
    }
    if (n_obs > 0) {
        if (!d.obs_view || !d.ref_view || !d.points) return false;
        for (int32_t k = 0; k < n_obs; ++k)
            if (d.obs_view[k] < 0 || d.obs_view[k] >= d.n_views) return false;
        for (size_t p = 0; p < np; ++p)
            if (d.obs_ptr[p + 1] > d.obs_ptr[p] && (d.ref_view[p] < 0 || d.ref_view[p] >= d.n_views)) return false;
    }
    return true;
}

// the three result arrays of either entry point
struct PnOut {
    Out<double> normals, dmax, dmin;
    void plan(double *n, double *mx, double *mn, size_t np, Carver &c) { normals.plan(n, 3 * np, c); dmax.plan(mx, np, c); dmin.plan(mn, np, c); }
    void bind(char *sd, PnDev &t)
    {
        normals.bind(sd); dmax.bind(sd); dmin.bind(sd);
        t.normals = normals.dev; t.max_dist = dmax.dev; t.min_dist = dmin.dev;
    }
    void fetch(const char *sg) const { normals.fetch(sg); dmax.fetch(sg); dmin.fetch(sg); }
};

}  // namespace

extern "C" {

int movba_point_normals(movba_handle *h, const movba_normals_desc *desc, movba_normals_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_normals_desc &d = *desc;
    if (!pn_desc_ok(d, *res)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_points == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    const size_t np = (size_t)d.n_points, nv = (size_t)d.n_views, n_obs = (size_t)d.obs_ptr[np], nl = (size_t)d.n_levels;
    if (n_obs == 0) {       // (nothing for the device to do: every list is empty, MapPoint.cc:377)
        const double nan = std::nan("");
        for (size_t k = 0; k < 3 * np; ++k) res->normals[k] = nan;
        for (size_t p = 0; p < np; ++p) res->max_distance[p] = res->min_distance[p] = nan;
        res->status = MOVBA_OK;
        return MOVBA_OK;
    }

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's side-call scratch.  Behind them on the device: the views'
    // centres; behind them in the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<double> poses, pts, scale;
    In<int32_t> ptr, view, rv, rl;
    poses.plan(7 * nv, c); pts.plan(3 * np, c); ptr.plan(np + 1, c);
    view.plan(n_obs, c); rv.plan(np, c); rl.plan(np, c); scale.plan(nl, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_ctr = dv.take<double>(3 * nv);
    PnOut out;
    out.plan(res->normals, res->max_distance, res->min_distance, np, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    poses.fill(sg, d.poses); pts.fill(sg, d.points); ptr.fill(sg, d.obs_ptr);
    view.fill(sg, d.obs_view); rv.fill(sg, d.ref_view); rl.fill(sg, d.ref_level); scale.fill(sg, d.scale_factors);

    PnDev t{};
    t.n_views = d.n_views; t.n_points = d.n_points; t.n_levels = d.n_levels;
    t.poses = poses.dev(ar); t.points = pts.dev(ar); t.lists.ptr = ptr.dev(ar); t.lists.view = view.dev(ar);
    t.ref_view = rv.dev(ar); t.ref_level = rl.dev(ar); t.scale = scale.dev(ar);
    t.centres = at<double>(ar, o_ctr);
    out.bind(h->stage_dev, t);

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_point_normals(t, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    out.fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

int movba_lba_point_normals(movba_handle *h, const int32_t *ref_pose, const int32_t *ref_level, const double *scale_factors,
                            int32_t n_levels, const uint8_t *outlier, double *normals, double *max_distance, double *min_distance)
{
    if (!h || !ref_pose || !ref_level || !scale_factors || !normals || !max_distance || !min_distance || n_levels < 1) return MOVBA_ERR_ARG;
    // a run of this upload that solved the window (not one that ended before the solve, was stopped, or failed): as
    // movba_lba_marginals
    if (!h->uploaded || !h->ran || h->early_status != MOVBA_OK || h->run_status != MOVBA_OK || h->ctrl_host->n_sync_timeouts > 0)
        return MOVBA_ERR_STATE;
    const DevWindow &w = h->win;
    const size_t np = (size_t)w.P, nv = (size_t)w.NP, ne = (size_t)w.E, nl = (size_t)n_levels;
    if (!pn_levels_ok(n_levels, scale_factors, ref_level, np)) return MOVBA_ERR_ARG;
    // (the lists live on the device: which entries are read is not known here, so every one must index a pose)
    for (size_t p = 0; p < np; ++p)
        if (ref_pose[p] < 0 || ref_pose[p] >= w.NP) return MOVBA_ERR_ARG;

    // Layout as above; what crosses the bus is the reference entries, the table and the caller's flags - never read through
    // DevWindow::out_outlier, and not through a pointer the window kept from an earlier call.
    Carver c;
    In<int32_t> rv, rl;
    In<double> scale;
    In<uint8_t> mask;
    rv.plan(np, c); rl.plan(np, c); scale.plan(nl, c); mask.plan(outlier ? ne : 0, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_ctr = dv.take<double>(3 * nv);
    PnOut out;
    out.plan(normals, max_distance, min_distance, np, c);
    const size_t total = c.off;

    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    rv.fill(sg, ref_pose); rl.fill(sg, ref_level); scale.fill(sg, scale_factors); mask.fill(sg, outlier);

    PnDev t{};
    t.n_views = w.NP; t.n_points = w.P; t.n_levels = n_levels;
    t.cur = &w.ctrl->cur;               // (an address on the device: read there, as k_export reads it)
    for (int k = 0; k < 2; ++k) { t.pose_st[k] = w.st[k].pose; t.point_st[k] = w.st[k].point; }
    t.lists.ptr = w.pt_start; t.lists.view = w.g_pose; t.lists.perm = w.perm;
    t.lists.mask = mask.dev(ar);
    t.ref_view = rv.dev(ar); t.ref_level = rl.dev(ar); t.scale = scale.dev(ar);
    t.centres = at<double>(ar, o_ctr);
    out.bind(h->stage_dev, t);

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_point_normals(t, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    out.fetch(sg);
    return MOVBA_OK;
}

}  // extern "C"
