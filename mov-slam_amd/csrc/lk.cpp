// movba_lk_track (include/movba.h): sparse pyramidal Lucas-Kanade - cv::calcOpticalFlowPyrLK as the reference calls it - for the
// points of many frames per call.  The device passes are lk.hip (the steps with a serial meaning: lk.h); this file checks the
// call, lays out both pyramids of every frame that has points, packs what has to cross the bus into the handle's staging
// buffer - level 0 of both images tightly, row by row without the stride's padding - sends it with ONE copy, queues the
// launches and hands the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are
// written by the kernels themselves; others arrive in the staging buffer and are copied out.
#include <cmath>
#include <cstring>

#include "handle.h"
#include "lk.h"

using namespace movba;

namespace {

constexpr float kLkMaxCoord = 1048576.0f;           // 2^20

bool ascending(const int32_t *p, size_t n)
{
    if (!p || p[0] != 0) return false;
    for (size_t i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) return false;
    return true;
}

// everything about a call with frames that can be wrong, checked before anything is queued or written
bool lk_desc_ok(const movba_lk_desc &d, const movba_lk_result &r)
{
    const size_t nf = (size_t)d.n_frames;
    if (!ascending(d.pt_ptr, nf)) return false;
    if (!d.prev_image || !d.next_image || !d.rows || !d.cols || !d.stride || !d.win) return false;
    const size_t n_pt = (size_t)d.pt_ptr[nf];
    if (n_pt > MOVBA_MAX_EXPRESS_ITEMS || (n_pt && !d.pt)) return false;
    if (!r.next_pt || !r.pt_status || !r.err || !r.exit_code || !r.keep || !r.kept_ptr || !r.kept_src) return false;
    if (d.max_level < 0 || d.max_level > MOVBA_LK_MAX_LEVEL || d.max_iter < 1 || d.max_iter > MOVBA_LK_MAX_ITER) return false;
    if (!std::isfinite(d.eps) || !(d.eps > 0.0) || d.eps > 10.0) return false;
    if (!std::isfinite(d.min_eig_threshold) || !(d.min_eig_threshold > 0.0)) return false;
    int64_t pixels = 0;
    for (size_t f = 0; f < nf; ++f) {
        if (d.win[f] < 3 || d.win[f] > MOVBA_LK_MAX_WIN || d.win[f] % 2 == 0) return false;
        if (d.rows[f] <= d.win[f] || d.cols[f] <= d.win[f] || d.stride[f] < d.cols[f]) return false;
        pixels += (int64_t)d.rows[f] * d.cols[f];
        if (pixels > MOVBA_LK_MAX_PIXELS) return false;
        if (d.pt_ptr[f + 1] > d.pt_ptr[f] && (!d.prev_image[f] || !d.next_image[f])) return false;
    }
    for (size_t i = 0; i < 2 * n_pt; ++i)
        if (!(std::fabs(d.pt[i]) <= kLkMaxCoord)) return false;        // (false for a NaN)
    return true;
}

}  // namespace

extern "C" {

int movba_lk_track(movba_handle *h, const movba_lk_desc *desc, movba_lk_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_lk_desc &d = *desc;
    if (d.n_frames < 0 || d.n_frames > MOVBA_MAX_EXPRESS_IMAGES) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_frames == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    if (!lk_desc_ok(d, *res)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t nf = (size_t)d.n_frames, n_pt = (size_t)d.pt_ptr[nf];

    // the pyramids' sizes: only frames that have points have pixels at any level
    size_t level0 = 0, upper = 0;
    for (size_t f = 0; f < nf; ++f) {
        if (d.pt_ptr[f + 1] == d.pt_ptr[f]) continue;
        LkFrame fr;
        lk_frame_levels(d.rows[f], d.cols[f], d.win[f], d.max_level, &fr);
        level0 += (size_t)fr.rows[0] * fr.cols[0];
        for (int l = 1; l <= fr.levels; ++l) upper += (size_t)fr.rows[l] * fr.cols[l];
    }

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's side-call scratch; behind them, on the device alone: the
    // frames' kept counts and levels 1 .. 3 of both pyramids (dv); in the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<LkFrame> frames;
    In<int32_t> pptr, lptr;
    In<float> pts;
    In<uint8_t> pix;
    frames.plan(nf, c); pptr.plan(nf + 1, c); lptr.plan((kLkLevels - 1) * (nf + 1), c); pts.plan(2 * n_pt, c); pix.plan(2 * level0, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_cnt = dv.take<int32_t>(nf), o_upper = dv.take<uint8_t>(2 * upper);
    Out<float> next, err;
    Out<uint8_t> stat, code, keep;
    Out<int32_t> kptr, ksrc;
    next.plan(res->next_pt, 2 * n_pt, c); stat.plan(res->pt_status, n_pt, c); err.plan(res->err, n_pt, c); code.plan(res->exit_code, n_pt, c);
    keep.plan(res->keep, n_pt, c); kptr.plan(res->kept_ptr, nf + 1, c); ksrc.plan(res->kept_src, n_pt, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    pptr.fill(sg, d.pt_ptr); pts.fill(sg, d.pt);
    LkFrame *table = frames.host(sg);
    int32_t *lvl = lptr.host(sg);
    uint8_t *pixels = pix.host(sg);
    LkDev e{};
    for (int l = 1; l < kLkLevels; ++l) lvl[(size_t)(l - 1) * (nf + 1)] = 0;
    size_t at0 = 0, at_up = 0;
    for (size_t f = 0; f < nf; ++f) {
        LkFrame &fr = table[f];
        std::memset(&fr, 0, sizeof fr);
        lk_frame_levels(d.rows[f], d.cols[f], d.win[f], d.max_level, &fr);
        const bool used = d.pt_ptr[f + 1] > d.pt_ptr[f];
        for (int l = 1; l < kLkLevels; ++l) {
            int32_t *p = lvl + (size_t)(l - 1) * (nf + 1) + f;
            p[1] = p[0] + (used && l <= fr.levels ? fr.rows[l] * fr.cols[l] : 0);
        }
        if (!used) continue;
        const size_t nc = (size_t)fr.cols[0], nr = (size_t)fr.rows[0];
        const uint8_t *const src[2] = { d.prev_image[f], d.next_image[f] };
        for (int i = 0; i < 2; ++i) {
            fr.off[i][0] = (int64_t)(pix.off + at0);
            for (size_t y = 0; y < nr; ++y, at0 += nc) std::memcpy(pixels + at0, src[i] + y * (size_t)d.stride[f], nc);
            for (int l = 1; l <= fr.levels; ++l) {
                fr.off[i][l] = (int64_t)(o_upper + at_up);
                at_up += (size_t)fr.rows[l] * fr.cols[l];
            }
        }
    }
    for (int l = 1; l < kLkLevels; ++l) e.level_pixels[l - 1] = lvl[(size_t)(l - 1) * (nf + 1) + nf];

    e.n_frames = d.n_frames; e.n_pt = (int32_t)n_pt; e.max_iter = d.max_iter;
    e.eps_sq = d.eps * d.eps; e.min_eig = d.min_eig_threshold;
    e.frame = frames.dev(ar); e.pt_ptr = pptr.dev(ar); e.lvl_ptr = lptr.dev(ar); e.pt = pts.dev(ar);
    e.pix = at<uint8_t>(ar, 0); e.kept_cnt = at<int32_t>(ar, o_cnt);
    next.bind(h->stage_dev); err.bind(h->stage_dev);
    for (Out<uint8_t> *o : { &stat, &code, &keep }) o->bind(h->stage_dev);
    kptr.bind(h->stage_dev); ksrc.bind(h->stage_dev);
    e.next_pt = next.dev; e.err = err.dev; e.pt_status = stat.dev; e.exit_code = code.dev; e.keep = keep.dev;
    e.kept_ptr = kptr.dev; e.kept_src = ksrc.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_lk(e, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    next.fetch(sg); err.fetch(sg);
    for (const Out<uint8_t> *o : { &stat, &code, &keep }) o->fetch(sg);
    kptr.fetch(sg); ksrc.fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

}  // extern "C"
