// movba_mv_raster (include/movba.h): the loop of VideoDecoder::NextImage over a frame's motion-vector records - keep test, kps
// and mvs, the source blocks' slots at the queried pixels, coverage - for many frames per call, without the 4-channel image.  The
// device passes are mv_raster.hip (the steps with a serial meaning: mv_raster.h); this file checks the call, packs what has to
// cross the bus into the handle's staging buffer - `source` and `ref` are checked here and stay behind - sends it with ONE
// copy, queues the launches and hands the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc
// memory are written by the kernels themselves; others arrive in the staging buffer and are copied out.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handle.h"
#include "mv_raster.h"

using namespace movba;

namespace {

constexpr int64_t kMvrMaxPixels = 1 << 28;
constexpr float kMvrMaxCoord = 1048576.0f;          // 2^20
constexpr int32_t kMvrMaxExtent = 32767;

bool ascending(const int32_t *p, size_t n)
{
    if (!p || p[0] != 0) return false;
    for (size_t i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) return false;
    return true;
}

struct Sizes { size_t n_rec, n_q, n_grid, n_tiles; int32_t max_rec; };

// everything about a call with frames that can be wrong, checked before anything is queued or written
bool mvr_desc_ok(const movba_mv_raster_desc &d, const movba_mv_raster_result &r, Sizes *sz)
{
    const size_t nf = (size_t)d.n_frames;
    if (!ascending(d.rec_ptr, nf) || !ascending(d.q_ptr, nf)) return false;
    if (!d.rows || !d.cols || !d.coverage_threshold || !d.want_grid) return false;
    const size_t n_rec = (size_t)d.rec_ptr[nf], n_q = (size_t)d.q_ptr[nf];
    if (n_rec > MOVBA_MAX_EXPRESS_ITEMS || n_q > MOVBA_MAX_EXPRESS_ITEMS) return false;
    if (n_rec && (!d.src_x || !d.src_y || !d.dst_x || !d.dst_y || !d.w || !d.h || !d.source || !d.ref)) return false;
    if (n_q && !d.q_pt) return false;
    if (!r.kept_ptr || !r.kp_rect || !r.mv_pt || !r.mv_dindx || !r.rec_kept || !r.cand || !r.grid_ptr || !r.grid_covered || !r.cover_px ||
        !r.coverage_area || !r.force_grid) return false;
    int64_t pixels = 0, n_grid = 0, n_tiles = 0;
    int32_t max_rec = 0;
    for (size_t f = 0; f < nf; ++f) {
        if (d.rows[f] < 1 || d.cols[f] < 1 || d.rows[f] > kMvrMaxExtent || d.cols[f] > kMvrMaxExtent) return false;
        if (!std::isfinite(d.coverage_threshold[f])) return false;
        if (d.rec_ptr[f + 1] - d.rec_ptr[f] > kMvrMaxFrameRecords) return false;
        max_rec = std::max(max_rec, d.rec_ptr[f + 1] - d.rec_ptr[f]);
        pixels += (int64_t)d.rows[f] * d.cols[f];
        if (pixels > kMvrMaxPixels) return false;
        n_grid += adv_lattice(d.rows[f], d.cols[f]);
        n_tiles += mvr_tiles(d.rows[f], d.cols[f]);
        if ((int64_t)n_rec + (int64_t)n_q + n_grid > MOVBA_MAX_EXPRESS_ITEMS) return false;
    }
    for (size_t i = 0; i < n_rec; ++i)
        if (!mvr_size_ok(d.w[i]) || !mvr_size_ok(d.h[i]) || d.ref[i] != 0 || d.source[i] >= 0) return false;
    for (size_t i = 0; i < 2 * n_q; ++i)
        if (!(std::fabs(d.q_pt[i]) <= kMvrMaxCoord)) return false;     // (false for a NaN)
    *sz = Sizes{ n_rec, n_q, (size_t)n_grid, (size_t)n_tiles, max_rec };
    return true;
}

}  // namespace

extern "C" {

int movba_mv_raster(movba_handle *h, const movba_mv_raster_desc *desc, movba_mv_raster_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_mv_raster_desc &d = *desc;
    if (d.n_frames < 0 || d.n_frames > MOVBA_MAX_EXPRESS_IMAGES) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_frames == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    Sizes sz{};
    if (!mvr_desc_ok(d, *res, &sz)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t nf = (size_t)d.n_frames, n_rec = sz.n_rec, n_q = sz.n_q, n_grid = sz.n_grid, n_tiles = sz.n_tiles;

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's side-call scratch; behind them, on the device alone: the
    // kernels' scratch (dv); in the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<int32_t> rows, cols, rptr, qptr, gptr, tptr;
    In<double> thr;
    In<uint8_t> want, bw, bh;
    In<int16_t> sx, sy, dx, dy;
    In<float> qpt;
    rows.plan(nf, c); cols.plan(nf, c); rptr.plan(nf + 1, c); qptr.plan(nf + 1, c); gptr.plan(nf + 1, c); tptr.plan(nf + 1, c);
    thr.plan(nf, c); want.plan(nf, c);
    sx.plan(n_rec, c); sy.plan(n_rec, c); dx.plan(n_rec, c); dy.plan(n_rec, c); bw.plan(n_rec, c); bh.plan(n_rec, c);
    qpt.plan(2 * n_q, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_rec = dv.take<int32_t>(n_rec), o_chunk = dv.take<int32_t>(mvr_chunk_slots(n_rec, nf)), o_cnt = dv.take<int32_t>(nf), o_base = dv.take<int32_t>(nf + 1);
    // (cleared by one memset: the frames' coverage sums, then the tile counts)
    const size_t o_zero = dv.take<int32_t>(nf + n_tiles + 1), o_cur = dv.take<int32_t>(n_tiles), o_m = dv.take<int32_t>(4 * n_rec), o_ext = dv.take<uint64_t>(4 * n_rec);
    Out<int32_t> kept, rect, dindx, rkept, cand, grid, cover;
    Out<float> mvpt;
    Out<double> area;
    Out<uint8_t> covered, force;
    kept.plan(res->kept_ptr, nf + 1, c); rect.plan(res->kp_rect, 4 * n_rec, c); mvpt.plan(res->mv_pt, 2 * n_rec, c); dindx.plan(res->mv_dindx, n_rec, c);
    rkept.plan(res->rec_kept, n_rec, c); cand.plan(res->cand, 4 * n_q, c); grid.plan(res->grid_ptr, nf + 1, c); covered.plan(res->grid_covered, n_grid, c);
    cover.plan(res->cover_px, nf, c); area.plan(res->coverage_area, nf, c); force.plan(res->force_grid, nf, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    rows.fill(sg, d.rows); cols.fill(sg, d.cols); rptr.fill(sg, d.rec_ptr); qptr.fill(sg, d.q_ptr); thr.fill(sg, d.coverage_threshold);
    want.fill(sg, d.want_grid);
    sx.fill(sg, d.src_x); sy.fill(sg, d.src_y); dx.fill(sg, d.dst_x); dy.fill(sg, d.dst_y); bw.fill(sg, d.w); bh.fill(sg, d.h);
    qpt.fill(sg, d.q_pt);
    int32_t *g_ptr = gptr.host(sg), *t_ptr = tptr.host(sg);
    g_ptr[0] = t_ptr[0] = 0;
    for (size_t f = 0; f < nf; ++f) {
        g_ptr[f + 1] = g_ptr[f] + (int32_t)adv_lattice(d.rows[f], d.cols[f]);
        t_ptr[f + 1] = t_ptr[f] + (int32_t)mvr_tiles(d.rows[f], d.cols[f]);
    }

    MvrDev e{};
    e.n_frames = d.n_frames; e.n_records = (int32_t)n_rec; e.n_q = (int32_t)n_q; e.n_grid = (int32_t)n_grid; e.n_tiles = (int32_t)n_tiles; e.max_records = sz.max_rec;
    e.rows = rows.dev(ar); e.cols = cols.dev(ar); e.rec_ptr = rptr.dev(ar); e.q_ptr = qptr.dev(ar); e.g_ptr = gptr.dev(ar); e.tile_ptr = tptr.dev(ar);
    e.threshold = thr.dev(ar); e.want_grid = want.dev(ar);
    e.src_x = sx.dev(ar); e.src_y = sy.dev(ar); e.dst_x = dx.dev(ar); e.dst_y = dy.dev(ar); e.w = bw.dev(ar); e.h = bh.dev(ar); e.q_pt = qpt.dev(ar);
    e.kept_rec = at<int32_t>(ar, o_rec); e.chunk_cnt = at<int32_t>(ar, o_chunk); e.kept_cnt = at<int32_t>(ar, o_cnt); e.kept_base = at<int32_t>(ar, o_base);
    e.cover = at<int32_t>(ar, o_zero); e.tile_off = e.cover + nf; e.tile_cur = at<int32_t>(ar, o_cur); e.list_m = at<int32_t>(ar, o_m); e.list_ext = at<uint64_t>(ar, o_ext);
    for (Out<int32_t> *o : { &kept, &rect, &dindx, &rkept, &cand, &grid, &cover }) o->bind(h->stage_dev);
    mvpt.bind(h->stage_dev); area.bind(h->stage_dev); covered.bind(h->stage_dev); force.bind(h->stage_dev);
    e.kept_ptr = kept.dev; e.kp_rect = rect.dev; e.mv_dindx = dindx.dev; e.rec_kept = rkept.dev; e.cand = cand.dev; e.grid_ptr = grid.dev; e.cover_px = cover.dev;
    e.mv_pt = mvpt.dev; e.coverage_area = area.dev; e.grid_covered = covered.dev; e.force_grid = force.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_mv_raster(e, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (const Out<int32_t> *o : { &kept, &rect, &dindx, &rkept, &cand, &grid, &cover }) o->fetch(sg);
    mvpt.fetch(sg); area.fetch(sg); covered.fetch(sg); force.fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

}  // extern "C"
