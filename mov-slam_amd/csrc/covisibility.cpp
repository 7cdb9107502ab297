// movba_covisibility (include/movba.h): the covisibility count, its threshold, maximum and ordering - the numeric body of
// KeyFrame::UpdateConnections and of the voting loop of Tracking::UpdateLocalKeyFrames - for many queries per call.  The device
// pass is covisibility.hip (one kernel, one workgroup per query; the steps with a serial meaning: covisibility.h); this file
// checks the call, packs what has to cross the bus into the handle's staging buffer, sends it with ONE copy, queues the ONE
// launch and hands the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are written by
// the kernel itself; others arrive in the staging buffer and are copied out.
#include <cstring>

#include "covisibility.h"
#include "handle.h"

using namespace movba;

namespace {

constexpr int32_t kCvMaxEntries = 1 << 28;

// a prefix array of n + 1 entries: starts at 0, ascends, ends at or below 2^28
bool cv_prefix_ok(const int32_t *ptr, size_t n)
{
    if (!ptr || ptr[0] != 0) return false;
    for (size_t k = 0; k < n; ++k)
        if (ptr[k + 1] < ptr[k]) return false;
    return ptr[n] <= kCvMaxEntries;
}

// the counts alone: what is checked before a call without queries is let through
bool cv_counts_ok(const movba_covis_desc &d)
{
    if (d.n_views < 0 || d.n_points < 0 || d.n_queries < 0 || d.max_out < 0) return false;
    if (d.n_views > MOVBA_MAX_COVIS_VIEWS || d.n_queries > MOVBA_MAX_COVIS_QUERIES) return false;
    if (d.min_weight < 1) return false;
    return (int64_t)d.n_queries * d.max_out <= kCvMaxEntries;
}

// everything else about the call that can be wrong, checked before anything is queued or written (n_queries > 0)
bool cv_desc_ok(const movba_covis_desc &d, const movba_covis_result &r)
{
    const size_t np = (size_t)d.n_points, nq = (size_t)d.n_queries;
    if (!r.n_counted || !r.n_connected || !r.best_view || !r.best_weight) return false;
    if (d.max_out > 0 && (!r.out_view || !r.out_weight)) return false;
    int32_t n_obs = 0;
    if (np) {
        if (!cv_prefix_ok(d.obs_ptr, np)) return false;
        n_obs = d.obs_ptr[np];
        if (n_obs > 0 && !d.obs_view) return false;
        for (int32_t k = 0; k < n_obs; ++k)
            if (d.obs_view[k] < 0 || d.obs_view[k] >= d.n_views) return false;
    }
    if (!cv_prefix_ok(d.query_ptr, nq)) return false;
    const int32_t n_items = d.query_ptr[nq];
    if (n_items > 0 && !d.query_point) return false;
    for (size_t q = 0; q < nq; ++q) {
        if (d.query_self && (d.query_self[q] < -1 || d.query_self[q] >= d.n_views)) return false;
        int64_t entries = 0;            // (an upper bound of every weight of the query: they are int32)
        for (int32_t i = d.query_ptr[q]; i < d.query_ptr[q + 1]; ++i) {
            const int32_t p = d.query_point[i];
            if (p < 0 || p >= d.n_points) return false;
            entries += d.obs_ptr[p + 1] - d.obs_ptr[p];
        }
        if (entries > INT32_MAX) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int movba_covisibility(movba_handle *h, const movba_covis_desc *desc, movba_covis_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_covis_desc &d = *desc;
    if (!cv_counts_ok(d)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_queries == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    if (!cv_desc_ok(d, *res)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t np = (size_t)d.n_points, nv = (size_t)d.n_views, nq = (size_t)d.n_queries;
    const size_t n_obs = np ? (size_t)d.obs_ptr[np] : 0, n_items = (size_t)d.query_ptr[nq], n_out = nq * (size_t)d.max_out;

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's side-call scratch; behind them in the staging buffer: the
    // results (Out: those that are staged).
    Carver c;
    In<int32_t> optr, oview, qptr, qpoint, qself;
    In<uint8_t> elig;
    optr.plan(np ? np + 1 : 0, c); oview.plan(n_obs, c); qptr.plan(nq + 1, c); qpoint.plan(n_items, c);
    qself.plan(d.query_self ? nq : 0, c); elig.plan(d.eligible ? nv : 0, c);
    const size_t h2d = c.off;
    Out<int32_t> counted, connected, bview, bweight, oview_out, oweight_out;
    counted.plan(res->n_counted, nq, c); connected.plan(res->n_connected, nq, c); bview.plan(res->best_view, nq, c);
    bweight.plan(res->best_weight, nq, c); oview_out.plan(res->out_view, n_out, c); oweight_out.plan(res->out_weight, n_out, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, h2d, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    optr.fill(sg, d.obs_ptr); oview.fill(sg, d.obs_view); qptr.fill(sg, d.query_ptr); qpoint.fill(sg, d.query_point);
    qself.fill(sg, d.query_self); elig.fill(sg, d.eligible);

    CvDev t{};
    t.n_views = d.n_views; t.n_queries = d.n_queries; t.min_weight = d.min_weight; t.max_out = d.max_out;
    t.obs_ptr = optr.dev(ar); t.obs_view = oview.dev(ar); t.eligible = elig.dev(ar);
    t.query_ptr = qptr.dev(ar); t.query_point = qpoint.dev(ar); t.query_self = qself.dev(ar);
    for (Out<int32_t> *o : { &counted, &connected, &bview, &bweight, &oview_out, &oweight_out }) o->bind(h->stage_dev);
    t.n_counted = counted.dev; t.n_connected = connected.dev; t.best_view = bview.dev; t.best_weight = bweight.dev;
    t.out_view = oview_out.dev; t.out_weight = oweight_out.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_covisibility(t, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (const Out<int32_t> *o : { &counted, &connected, &bview, &bweight, &oview_out, &oweight_out }) o->fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

}  // extern "C"
