// movba_triangulate (include/movba.h): the numeric body of LocalMapping::CreateNewMapPoints for many keyframe pairs in one
// call.  The device pass is triangulate.hip (one kernel); this file checks the call, packs views + pairs + matches into the
// handle's staging buffer, sends them with ONE copy, queues the ONE launch and hands the results over after ONE
// synchronisation.  Result arrays that lie in movba_host_alloc memory are written by the kernel itself; others arrive in the
// staging buffer and are copied out.  n_accepted is counted here from `code`, in order: two calls give the same number.
#include <cmath>
#include <cstring>

#include "handle.h"
#include "triangulate.h"

using namespace movba;

namespace {

constexpr int32_t kTriMaxMatches = 1 << 30;     // (match indices and the grid stay well inside int32)

// everything about the descriptor that can be wrong, checked before anything is queued or written
bool tri_desc_ok(const movba_tri_desc &d, const movba_tri_result &r)
{
    if (d.n_views < 0 || d.n_pairs < 0) return false;
    if (!std::isfinite(d.reproj_gate) || d.far_threshold != d.far_threshold) return false;
    if (d.n_pairs == 0) return true;
    if (!d.pair_ptr || !d.pair_view) return false;
    if (d.pair_ptr[0] != 0) return false;
    for (int p = 0; p < d.n_pairs; ++p)
        if (d.pair_ptr[p + 1] < d.pair_ptr[p]) return false;
    const int32_t n = d.pair_ptr[d.n_pairs];
    if (n > kTriMaxMatches) return false;
    if (d.n_views > 0 && (!d.poses || !d.cam)) return false;
    for (int k = 0; k < 2 * d.n_pairs; ++k)
        if (d.pair_view[k] < 0 || d.pair_view[k] >= d.n_views) return false;
    if ((d.ur1 || d.ur2) && (!d.bf || !d.b)) return false;
    if ((d.ur1 && !d.depth1) || (d.ur2 && !d.depth2)) return false;
    if (n > 0 && (!d.obs1 || !d.obs2 || !r.points || !r.code)) return false;
    return true;
}

}  // namespace

extern "C" int movba_triangulate(movba_handle *h, const movba_tri_desc *desc, movba_tri_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_tri_desc &d = *desc;
    if (!tri_desc_ok(d, *res)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t n = d.n_pairs > 0 ? (size_t)d.pair_ptr[d.n_pairs] : 0;
    if (n == 0) { res->n_accepted = 0; res->status = MOVBA_OK; return MOVBA_OK; }
    const size_t nv = (size_t)d.n_views, np = (size_t)d.n_pairs;
    const bool stereo_views = d.bf && d.b;

    // Layout.  [0, h2d): the inputs; behind them (staging buffer only) the results.
    Carver c;
    In<double> poses, cam, bf, b, obs1, obs2, ur1, d1, ur2, d2;
    In<int32_t> pv, pp;
    poses.plan(7 * nv, c); cam.plan(4 * nv, c); bf.plan(stereo_views ? nv : 0, c); b.plan(stereo_views ? nv : 0, c);
    pv.plan(2 * np, c); pp.plan(np + 1, c); obs1.plan(2 * n, c); obs2.plan(2 * n, c);
    ur1.plan(d.ur1 ? n : 0, c); d1.plan(d.ur1 ? n : 0, c); ur2.plan(d.ur2 ? n : 0, c); d2.plan(d.ur2 ? n : 0, c);
    const size_t h2d = c.off;
    Out<double> points;
    Out<uint8_t> code;
    points.plan(res->points, 3 * n, c); code.plan(res->code, n, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, h2d, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    poses.fill(sg, d.poses); cam.fill(sg, d.cam); bf.fill(sg, d.bf); b.fill(sg, d.b);
    pv.fill(sg, d.pair_view); pp.fill(sg, d.pair_ptr); obs1.fill(sg, d.obs1); obs2.fill(sg, d.obs2);
    ur1.fill(sg, d.ur1); d1.fill(sg, d.depth1); ur2.fill(sg, d.ur2); d2.fill(sg, d.depth2);

    TriDev t{};
    t.n_matches = (int32_t)n; t.n_pairs = d.n_pairs;
    t.poses = poses.dev(ar); t.cam = cam.dev(ar); t.bf = bf.dev(ar); t.b = b.dev(ar);
    t.pair_view = pv.dev(ar); t.pair_ptr = pp.dev(ar); t.obs1 = obs1.dev(ar); t.obs2 = obs2.dev(ar);
    t.ur1 = ur1.dev(ar); t.depth1 = d1.dev(ar); t.ur2 = ur2.dev(ar); t.depth2 = d2.dev(ar);
    t.gate = d.reproj_gate; t.far_th = d.far_threshold;
    points.bind(h->stage_dev); code.bind(h->stage_dev);
    t.points = points.dev; t.code = code.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_triangulate(t, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    points.fetch(sg); code.fetch(sg);
    int32_t acc = 0;
    for (size_t m = 0; m < n; ++m) acc += res->code[m] >= MOVBA_TRI_DLT && res->code[m] <= MOVBA_TRI_STEREO2;
    res->n_accepted = acc;
    res->status = MOVBA_OK;
    return MOVBA_OK;
}
