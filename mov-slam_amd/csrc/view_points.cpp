// movba_view_points (include/movba.h): Frame::isInFrustum, the gates at the head of MOVMatcher::Fuse and
// KeyFrame::ComputeSceneMedianDepth for many views in one call.  The device pass is view_points.hip (two kernels); this file
// checks the call, builds the chunk table (at most 256 consecutive items of one view per workgroup), packs views + chunks +
// item indices + the point table into the handle's staging buffer, sends them with ONE copy, queues the TWO launches and hands
// the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are written by the kernels
// themselves; others arrive in the staging buffer and are copied out.
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"
#include "view_points.h"

using namespace movba;

namespace {

constexpr int32_t kVpMaxItems = 1 << 28;

bool finite_all(const double *a, size_t count)
{
    for (size_t k = 0; k < count; ++k)
        if (!std::isfinite(a[k])) return false;
    return true;
}

// everything about the call that can be wrong, checked before anything is queued or written
bool vp_desc_ok(const movba_view_desc &d, const movba_view_result &r)
{
    if (d.n_points < 0 || d.n_views < 0 || d.n_views > MOVBA_MAX_VIEW_BATCH) return false;
    if (d.n_views == 0) return true;
    const size_t nv = (size_t)d.n_views;
    if (!d.mode || !d.poses || !d.cam || !d.view_ptr || !r.n_accepted || !r.median_depth) return false;
    if (d.view_ptr[0] != 0) return false;
    for (size_t v = 0; v < nv; ++v)
        if (d.view_ptr[v + 1] < d.view_ptr[v]) return false;
    const int32_t n = d.view_ptr[nv];
    if (n > kVpMaxItems) return false;
    bool frustum = false, fuse = false, depth = false;
    for (size_t v = 0; v < nv; ++v) {
        if (d.mode[v] == MOVBA_VIEW_FRUSTUM) frustum = true;
        else if (d.mode[v] == MOVBA_VIEW_FUSE) fuse = true;
        else if (d.mode[v] == MOVBA_VIEW_DEPTH) depth = true;
        else return false;
    }
    if ((frustum || fuse) && (!d.bounds || !d.normals || !d.max_distance || !d.min_distance)) return false;
    if (frustum && (!d.log_scale_factor || !d.n_levels || !d.cos_limit)) return false;
    if (depth && !d.q) return false;
    if (!finite_all(d.poses, 7 * nv) || !finite_all(d.cam, 4 * nv)) return false;
    if ((d.bf && !finite_all(d.bf, nv)) || (d.bounds && !finite_all(d.bounds, 4 * nv))) return false;
    if ((d.log_scale_factor && !finite_all(d.log_scale_factor, nv)) || (d.cos_limit && !finite_all(d.cos_limit, nv))) return false;
    for (size_t v = 0; v < nv; ++v) {
        const double *q = d.poses + 7 * v;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return false;
        if (!(d.cam[4 * v] > 0.0) || !(d.cam[4 * v + 1] > 0.0)) return false;
        if (d.n_levels && d.n_levels[v] < 1) return false;
        if (d.mode[v] == MOVBA_VIEW_DEPTH && d.q[v] < 1) return false;
        if (d.mode[v] == MOVBA_VIEW_FRUSTUM && !(d.log_scale_factor[v] > 0.0)) return false;
    }
    if (n > 0) {
        if (!d.item_point || !d.points || !r.code) return false;
        for (int32_t i = 0; i < n; ++i)
            if (d.item_point[i] < 0 || d.item_point[i] >= d.n_points) return false;
    }
    return true;
}

}  // namespace

extern "C" int movba_view_points(movba_handle *h, const movba_view_desc *desc, movba_view_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_view_desc &d = *desc;
    if (!vp_desc_ok(d, *res)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_views == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    const size_t nv = (size_t)d.n_views, n = (size_t)d.view_ptr[nv], np = (size_t)d.n_points;
    const double nan = std::nan("");
    if (n == 0) {           // (nothing for the device to do: every list is empty)
        for (size_t v = 0; v < nv; ++v) {
            res->n_accepted[v] = 0;
            res->median_depth[v] = d.mode[v] == MOVBA_VIEW_DEPTH ? -1.0 : nan;
        }
        res->status = MOVBA_OK;
        return MOVBA_OK;
    }

    // the views as the kernels read them, and the chunk table
    std::vector<VpView> views(nv);
    std::vector<VpChunk> chunks;
    chunks.reserve(n / kVpThreads + nv);
    size_t n_keys = 0;
    bool table = false;         // normals and distances are read
    for (size_t v = 0; v < nv; ++v) {
        VpView &w = views[v];
        std::memset(&w, 0, sizeof w);
        w.mode = d.mode[v]; w.n_levels = d.n_levels ? d.n_levels[v] : 1; w.q = d.q ? d.q[v] : 1;
        w.n = d.view_ptr[v + 1] - d.view_ptr[v]; w.item0 = d.view_ptr[v];
        for (int e = 0; e < 7; ++e) w.pose[e] = d.poses[7 * v + e];
        for (int e = 0; e < 4; ++e) { w.cam[e] = d.cam[4 * v + e]; w.bounds[e] = d.bounds ? d.bounds[4 * v + e] : 0.0; }
        w.bf = d.bf ? d.bf[v] : 0.0;
        w.log_scale = d.log_scale_factor ? d.log_scale_factor[v] : 1.0;
        w.cos_limit = d.cos_limit ? d.cos_limit[v] : 0.0;
        if (w.mode == MOVBA_VIEW_DEPTH) { w.key0 = (int64_t)n_keys; n_keys += (size_t)w.n; }
        else table = true;
        for (int32_t at = 0; at < w.n; at += kVpThreads) {
            VpChunk c;
            c.view = (int32_t)v; c.count = w.n - at < kVpThreads ? w.n - at : kVpThreads; c.first = w.item0 + at;
            chunks.push_back(c);
        }
    }
    const size_t nc = chunks.size();

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's pose scratch.  Behind them on the device: the select's keys
    // and the codes k_vp_views counts; behind them in the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<VpView> in_views;
    In<VpChunk> in_chunks;
    In<int32_t> item;
    In<double> pts, nrm, dmax, dmin;
    in_views.plan(nv, c); in_chunks.plan(nc, c); item.plan(n, c); pts.plan(3 * np, c);
    nrm.plan(table ? 3 * np : 0, c); dmax.plan(table ? np : 0, c); dmin.plan(table ? np : 0, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_keys = dv.take<uint64_t>(n_keys), o_cdev = dv.take<uint8_t>(n);
    Out<uint8_t> code;
    Out<double> z, uv, dist, vcos, ur, depth, median;
    Out<int32_t> level, nacc;
    code.plan(res->code, n, c); z.plan(res->z, n, c); uv.plan(res->uv, 2 * n, c); dist.plan(res->dist, n, c);
    vcos.plan(res->view_cos, n, c); level.plan(res->level, n, c); ur.plan(res->ur, n, c); depth.plan(res->track_depth, n, c);
    nacc.plan(res->n_accepted, nv, c); median.plan(res->median_depth, nv, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p, *sd = h->stage_dev;
    in_views.fill(sg, views.data()); in_chunks.fill(sg, chunks.data()); item.fill(sg, d.item_point);
    pts.fill(sg, d.points); nrm.fill(sg, d.normals); dmax.fill(sg, d.max_distance); dmin.fill(sg, d.min_distance);

    VpDev t{};
    t.n_views = d.n_views; t.n_chunks = (int32_t)nc;
    t.views = in_views.dev(ar); t.chunks = in_chunks.dev(ar); t.item_point = item.dev(ar);
    t.points = pts.dev(ar); t.normals = nrm.dev(ar); t.max_dist = dmax.dev(ar); t.min_dist = dmin.dev(ar);
    t.keys = at<uint64_t>(ar, o_keys); t.code_dev = at<uint8_t>(ar, o_cdev);
    code.bind(sd); z.bind(sd); uv.bind(sd); dist.bind(sd); vcos.bind(sd); level.bind(sd); ur.bind(sd); depth.bind(sd);
    nacc.bind(sd); median.bind(sd);
    t.code = code.dev; t.z = z.dev; t.uv = uv.dev; t.dist = dist.dev; t.view_cos = vcos.dev; t.level = level.dev; t.ur = ur.dev;
    t.track_depth = depth.dev; t.n_accepted = nacc.dev; t.median = median.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_view_points(t, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    code.fetch(sg); z.fetch(sg); uv.fetch(sg); dist.fetch(sg); vcos.fetch(sg); level.fetch(sg); ur.fetch(sg); depth.fetch(sg);
    nacc.fetch(sg); median.fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}
