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

template <typename T> void put(char *stage, size_t off, const T *src, size_t count)
{
    std::memcpy(stage + off, src, sizeof(T) * count);
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

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's pose scratch; behind them (staging buffer only) the
    // results that do not go straight into the caller's pinned arrays.
    Carver c;
    const size_t o_poses = c.take<double>(7 * nv), o_cam = c.take<double>(4 * nv);
    const size_t o_bf = stereo_views ? c.take<double>(nv) : 0, o_b = stereo_views ? c.take<double>(nv) : 0;
    const size_t o_pv = c.take<int32_t>(2 * np), o_pp = c.take<int32_t>(np + 1);
    const size_t o_obs1 = c.take<double>(2 * n), o_obs2 = c.take<double>(2 * n);
    const size_t o_ur1 = d.ur1 ? c.take<double>(n) : 0, o_d1 = d.ur1 ? c.take<double>(n) : 0;
    const size_t o_ur2 = d.ur2 ? c.take<double>(n) : 0, o_d2 = d.ur2 ? c.take<double>(n) : 0;
    const size_t h2d = c.off;
    unsigned long long *user_points = host_block_view(res->points, sizeof(double) * 3 * n);
    unsigned long long *user_code = host_block_view(res->code, n);
    const size_t o_points = user_points ? 0 : c.take<double>(3 * n), o_code = user_code ? 0 : c.take<uint8_t>(n);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, h2d, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    put(sg, o_poses, d.poses, 7 * nv); put(sg, o_cam, d.cam, 4 * nv);
    if (stereo_views) { put(sg, o_bf, d.bf, nv); put(sg, o_b, d.b, nv); }
    put(sg, o_pv, d.pair_view, 2 * np); put(sg, o_pp, d.pair_ptr, np + 1);
    put(sg, o_obs1, d.obs1, 2 * n); put(sg, o_obs2, d.obs2, 2 * n);
    if (d.ur1) { put(sg, o_ur1, d.ur1, n); put(sg, o_d1, d.depth1, n); }
    if (d.ur2) { put(sg, o_ur2, d.ur2, n); put(sg, o_d2, d.depth2, n); }

    auto dbl = [&](size_t off) { return reinterpret_cast<const double *>(ar + off); };
    TriDev t{};
    t.n_matches = (int32_t)n; t.n_pairs = d.n_pairs;
    t.poses = dbl(o_poses); t.cam = dbl(o_cam);
    t.bf = stereo_views ? dbl(o_bf) : nullptr; t.b = stereo_views ? dbl(o_b) : nullptr;
    t.pair_view = reinterpret_cast<const int32_t *>(ar + o_pv); t.pair_ptr = reinterpret_cast<const int32_t *>(ar + o_pp);
    t.obs1 = dbl(o_obs1); t.obs2 = dbl(o_obs2);
    t.ur1 = d.ur1 ? dbl(o_ur1) : nullptr; t.depth1 = d.ur1 ? dbl(o_d1) : nullptr;
    t.ur2 = d.ur2 ? dbl(o_ur2) : nullptr; t.depth2 = d.ur2 ? dbl(o_d2) : nullptr;
    t.gate = d.reproj_gate; t.far_th = d.far_threshold;
    t.points = user_points ? reinterpret_cast<double *>(user_points) : reinterpret_cast<double *>(h->stage_dev + o_points);
    t.code = user_code ? reinterpret_cast<uint8_t *>(user_code) : reinterpret_cast<uint8_t *>(h->stage_dev + o_code);

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_triangulate(t, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    if (!user_points) std::memcpy(res->points, sg + o_points, sizeof(double) * 3 * n);
    if (!user_code) std::memcpy(res->code, sg + o_code, n);
    int32_t acc = 0;
    for (size_t m = 0; m < n; ++m) acc += res->code[m] >= MOVBA_TRI_DLT && res->code[m] <= MOVBA_TRI_STEREO2;
    res->n_accepted = acc;
    res->status = MOVBA_OK;
    return MOVBA_OK;
}
