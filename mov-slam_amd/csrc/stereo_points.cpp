// movba_stereo_points (include/movba.h): the stereo gates behind the left-to-right LK call, the median-distance pruning, the
// un-projection and the choice of new map points - Frame::ComputeStereoMatches, Frame::UnprojectStereo and the walks of
// Tracking::StereoInitialization, CreateNewKeyFrame and UpdateLastFrame - for the keypoints of many frames per call.  The device
// passes are stereo_points.hip (every rule: stereo_points.h); this file checks the call, packs the frames' table - each frame's
// Rwc and Ow derived here, once - and the points' arrays into the handle's staging buffer, sends them with ONE copy, queues the
// two launches and hands the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are
// written by the kernels themselves; others arrive in the staging buffer and are copied out.
#include <cmath>
#include <cstring>

#include "handle.h"
#include "stereo_points.h"

using namespace movba;

namespace {

constexpr float kStMaxCoord = 1048576.0f;           // 2^20

bool ascending(const int32_t *p, size_t n)
{
    if (!p || p[0] != 0) return false;
    for (size_t i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) return false;
    return true;
}

bool coord_ok(float v) { return std::fabs(v) <= kStMaxCoord; }       // (false for a NaN)

// everything about a call with frames that can be wrong, checked before anything is queued or written
bool st_desc_ok(const movba_stereo_desc &d, const movba_stereo_result &r, int32_t *max_close, int32_t *max_frame)
{
    const size_t nf = (size_t)d.n_frames;
    if (!ascending(d.pt_ptr, nf)) return false;
    if (!d.rows || !d.cols || !d.bf || !d.max_disparity || !d.th_depth || !d.cam || !d.select) return false;
    const size_t n_pt = (size_t)d.pt_ptr[nf];
    if (n_pt > MOVBA_MAX_EXPRESS_ITEMS || (n_pt && (!d.pt || !d.next_pt || !d.pt_status))) return false;
    if (!r.u_right || !r.depth || !r.code || !r.n_stereo || !r.median_dist || !r.th_dist) return false;
    if (!r.sel_ptr || !r.sel_src || !r.sel_new || !r.sel_cam || !r.sel_point) return false;
    if (d.max_point < 0 || !std::isfinite(d.max_row_diff) || !std::isfinite(d.min_disparity)) return false;
    *max_close = *max_frame = 0;
    for (size_t f = 0; f < nf; ++f) {
        const int32_t n = d.pt_ptr[f + 1] - d.pt_ptr[f];
        if (n > MOVBA_MAX_STEREO_POINTS) return false;
        if (d.rows[f] < 1 || d.cols[f] < 1) return false;
        if (d.select[f] < MOVBA_STEREO_SELECT_NONE || d.select[f] > MOVBA_STEREO_SELECT_CLOSE) return false;
        if (!std::isfinite(d.bf[f]) || !(d.bf[f] > 0.f) || !std::isfinite(d.max_disparity[f]) || !std::isfinite(d.th_depth[f])) return false;
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(d.cam[4 * f + k])) return false;
        if (!(d.cam[4 * f] > 0.f) || !(d.cam[4 * f + 1] > 0.f)) return false;
        if (d.poses) {
            const double *q = d.poses + 7 * f;
            for (int k = 0; k < 7; ++k)
                if (!std::isfinite(q[k])) return false;
            if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return false;
        }
        if (d.select[f] == MOVBA_STEREO_SELECT_CLOSE && n > *max_close) *max_close = n;
        if (n > *max_frame) *max_frame = n;
    }
    for (size_t i = 0; i < 2 * n_pt; ++i) {
        if (!coord_ok(d.pt[i]) || (d.pt_un && !coord_ok(d.pt_un[i]))) return false;
        if (d.pt_status[i / 2] && !coord_ok(d.next_pt[i])) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int movba_stereo_points(movba_handle *h, const movba_stereo_desc *desc, movba_stereo_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_stereo_desc &d = *desc;
    if (d.n_frames < 0 || d.n_frames > MOVBA_MAX_EXPRESS_IMAGES) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_frames == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    int32_t max_close = 0, max_frame = 0;
    if (!st_desc_ok(d, *res, &max_close, &max_frame)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t nf = (size_t)d.n_frames, n_pt = (size_t)d.pt_ptr[nf];

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's side-call scratch; behind them, on the device alone: the
    // distances, the depths as they stand, the frames' lists and counts (dv); in the staging buffer: the results (Out: those
    // that are staged).
    Carver c;
    In<StFrame> frames;
    In<int32_t> pptr;
    In<float> pt, next, un;
    In<uint8_t> stat, has;
    frames.plan(nf, c); pptr.plan(nf + 1, c); pt.plan(2 * n_pt, c); next.plan(2 * n_pt, c); un.plan(d.pt_un ? 2 * n_pt : 0, c);
    stat.plan(n_pt, c); has.plan(d.has_point ? n_pt : 0, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_dist = dv.take<int32_t>(n_pt), o_z = dv.take<float>(n_pt), o_list = dv.take<int32_t>(n_pt), o_counts = dv.take<int32_t>(nf);
    Out<float> ur, depth, th, cam;
    Out<uint8_t> code, snew;
    Out<int32_t> nst, med, sptr, ssrc;
    Out<double> point;
    ur.plan(res->u_right, n_pt, c); depth.plan(res->depth, n_pt, c); code.plan(res->code, n_pt, c);
    nst.plan(res->n_stereo, nf, c); med.plan(res->median_dist, nf, c); th.plan(res->th_dist, nf, c);
    sptr.plan(res->sel_ptr, nf + 1, c); ssrc.plan(res->sel_src, n_pt, c); snew.plan(res->sel_new, n_pt, c);
    cam.plan(res->sel_cam, 3 * n_pt, c); point.plan(res->sel_point, 3 * n_pt, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    pptr.fill(sg, d.pt_ptr); pt.fill(sg, d.pt); next.fill(sg, d.next_pt); un.fill(sg, d.pt_un); stat.fill(sg, d.pt_status); has.fill(sg, d.has_point);
    StFrame *table = frames.host(sg);
    for (size_t f = 0; f < nf; ++f) {
        StFrame &fr = table[f];
        std::memset(&fr, 0, sizeof fr);
        fr.rows = d.rows[f]; fr.cols = d.cols[f]; fr.select = d.select[f];
        fr.bf = d.bf[f]; fr.max_disparity = d.max_disparity[f]; fr.th_depth = d.th_depth[f];
        fr.fx = d.cam[4 * f]; fr.fy = d.cam[4 * f + 1]; fr.cx = d.cam[4 * f + 2]; fr.cy = d.cam[4 * f + 3];
        st_frame_pose(d.poses ? d.poses + 7 * f : nullptr, &fr);
    }

    StDev e{};
    e.n_frames = d.n_frames; e.n_pt = (int32_t)n_pt; e.max_point = d.max_point; e.max_close = max_close; e.max_frame = max_frame;
    e.max_row_diff = d.max_row_diff; e.min_disparity = d.min_disparity;
    e.frame = frames.dev(ar); e.pt_ptr = pptr.dev(ar); e.pt = pt.dev(ar); e.next_pt = next.dev(ar);
    e.pt_un = d.pt_un ? un.dev(ar) : e.pt;
    e.pt_status = stat.dev(ar); e.has_point = has.dev(ar);
    e.dist = at<int32_t>(ar, o_dist); e.z = at<float>(ar, o_z); e.list = at<int32_t>(ar, o_list); e.counts = at<int32_t>(ar, o_counts);
    for (Out<float> *o : { &ur, &depth, &th, &cam }) o->bind(h->stage_dev);
    for (Out<uint8_t> *o : { &code, &snew }) o->bind(h->stage_dev);
    for (Out<int32_t> *o : { &nst, &med, &sptr, &ssrc }) o->bind(h->stage_dev);
    point.bind(h->stage_dev);
    e.u_right = ur.dev; e.depth = depth.dev; e.code = code.dev; e.n_stereo = nst.dev; e.median_dist = med.dev; e.th_dist = th.dev;
    e.sel_ptr = sptr.dev; e.sel_src = ssrc.dev; e.sel_new = snew.dev; e.sel_cam = cam.dev; e.sel_point = point.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_stereo_points(e, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (const Out<float> *o : { &ur, &depth, &th, &cam }) o->fetch(sg);
    for (const Out<uint8_t> *o : { &code, &snew }) o->fetch(sg);
    for (const Out<int32_t> *o : { &nst, &med, &sptr, &ssrc }) o->fetch(sg);
    point.fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

}  // extern "C"
