// movba_advance (include/movba.h): the inter-frame walk of MOVExtractor::operator() - sort, vector choice, claims, gate, new
// macroblocks, grid, track ids - for many frames per call.  The device passes are advance.hip (the steps with a serial meaning:
// advance.h); this file checks the call, packs what has to cross the bus into the handle's staging buffer - the pixels of the
// frames that have items tightly, the claim words filled - sends it with ONE copy, queues the four launches and hands the
// results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are written by the kernels
// themselves; others arrive in the staging buffer and are copied out.
#include <cmath>
#include <cstring>

#include "advance.h"
#include "handle.h"

using namespace movba;

namespace {

constexpr int64_t kAdvMaxPixels = 1 << 28;
constexpr float kAdvMaxCoord = 1048576.0f;          // 2^20

bool ascending(const int32_t *p, size_t n)
{
    if (!p || p[0] != 0) return false;
    for (size_t i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) return false;
    return true;
}

bool coord_ok(float v) { return std::fabs(v) <= kAdvMaxCoord; }      // (false for a NaN)

struct Sizes { size_t n_prev, n_mv, n_kps, n_grid, pixel_bytes; int32_t max_prev; };

// everything about a call with frames that can be wrong, checked before anything is queued or written
bool adv_desc_ok(const movba_advance_desc &d, const movba_advance_result &r, Sizes *sz)
{
    const size_t nf = (size_t)d.n_frames;
    if (!ascending(d.prev_ptr, nf) || !ascending(d.mv_ptr, nf) || !ascending(d.kp_ptr, nf) || (d.grid_ptr && !ascending(d.grid_ptr, nf))) return false;
    if (!d.rows || !d.cols || !d.stride || !d.threshold || !d.force_grid || !d.first_id || !d.image) return false;
    const size_t n_prev = (size_t)d.prev_ptr[nf], n_mv = (size_t)d.mv_ptr[nf], n_kps = (size_t)d.kp_ptr[nf];
    if (n_prev > MOVBA_MAX_EXPRESS_ITEMS || n_kps > MOVBA_MAX_EXPRESS_ITEMS) return false;
    if (n_prev && (!d.prev_pt || !d.prev_mb || !d.prev_age || !d.prev_track || !d.prev_desc || !d.prev_coverage || !d.prev_cand)) return false;
    if (n_mv && (!d.mv_pt || !d.mv_dindx)) return false;
    if (n_kps && !d.kp_rect) return false;
    if (d.grid_ptr && d.grid_ptr[nf] > 0 && !d.grid_covered) return false;
    if (!r.order || !r.fate || !r.chosen_mv || !r.distance || !r.kp_found || !r.kp_code || !r.mov_cnt || !r.grid_ran || !r.next_id || !r.seg_ptr) return false;
    if (!r.feat_src || !r.feat_track || !r.feat_pt || !r.feat_rect || !r.feat_age || !r.feat_desc) return false;
    int64_t all = 0, packed = 0, n_grid = 0;
    int32_t max_prev = 0;
    for (size_t f = 0; f < nf; ++f) {
        if (d.rows[f] < 1 || d.cols[f] < 1 || d.stride[f] < d.cols[f]) return false;
        if (d.threshold[f] < 0 || d.threshold[f] > 255) return false;
        all += (int64_t)d.rows[f] * d.cols[f];
        if (all > kAdvMaxPixels) return false;
        const int32_t np = d.prev_ptr[f + 1] - d.prev_ptr[f], nm = d.mv_ptr[f + 1] - d.mv_ptr[f], nk = d.kp_ptr[f + 1] - d.kp_ptr[f];
        const int64_t ng = adv_lattice(d.rows[f], d.cols[f]);
        if (np > MOVBA_MAX_ADVANCE_PREV) return false;
        if (d.grid_ptr && d.grid_ptr[f + 1] - d.grid_ptr[f] != ng) return false;
        if (d.first_id[f] < 0 || (int64_t)d.first_id[f] + nk + ng > INT32_MAX) return false;
        n_grid += ng;
        if ((int64_t)n_prev + (int64_t)n_kps + n_grid > MOVBA_MAX_EXPRESS_ITEMS) return false;
        max_prev = np > max_prev ? np : max_prev;
        if (np + nk + ng > 0) {
            if (!d.image[f]) return false;
            packed += (int64_t)d.rows[f] * d.cols[f];
        }
        for (size_t g = (size_t)d.prev_ptr[f]; g < (size_t)d.prev_ptr[f + 1]; ++g) {
            if ((d.prev_mb[2 * g] != 8 && d.prev_mb[2 * g] != 16) || (d.prev_mb[2 * g + 1] != 8 && d.prev_mb[2 * g + 1] != 16)) return false;
            if (d.prev_age[g] < 0 || d.prev_age[g] > INT32_MAX - 1) return false;
            if (!coord_ok(d.prev_pt[2 * g]) || !coord_ok(d.prev_pt[2 * g + 1])) return false;
            for (int c = 0; c < 4; ++c)
                if (d.prev_cand[4 * g + c] < -1 || d.prev_cand[4 * g + c] >= nm) return false;
        }
        for (size_t m = (size_t)d.mv_ptr[f]; m < (size_t)d.mv_ptr[f + 1]; ++m) {
            if (d.mv_dindx[m] < -1 || d.mv_dindx[m] >= nk) return false;
            if (!coord_ok(d.mv_pt[2 * m]) || !coord_ok(d.mv_pt[2 * m + 1])) return false;
        }
    }
    *sz = Sizes{ n_prev, n_mv, n_kps, (size_t)n_grid, (size_t)packed, max_prev };
    return true;
}

}  // namespace

extern "C" {

int movba_advance(movba_handle *h, const movba_advance_desc *desc, movba_advance_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_advance_desc &d = *desc;
    if (d.n_frames < 0 || d.n_frames > MOVBA_MAX_EXPRESS_IMAGES) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_frames == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    Sizes sz{};
    if (!adv_desc_ok(d, *res, &sz)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t nf = (size_t)d.n_frames, n_prev = sz.n_prev, n_mv = sz.n_mv, n_kps = sz.n_kps, n_grid = sz.n_grid;
    const size_t n_items = n_prev + n_kps + n_grid;

    // Layout.  [0, h2d): the inputs and the filled claim words, one H2D copy into the handle's side-call scratch; behind them,
    // on the device alone: the kernels' scratch (dv); in the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<int32_t> off, rows, cols, thr, force, first, pptr, mptr, kptr, gptr, mb, age, track, cand, dindx, rect, claim;
    In<float> ppt, mpt;
    In<uint64_t> pdesc;
    In<uint8_t> pcov, covered, pix;
    off.plan(nf, c); rows.plan(nf, c); cols.plan(nf, c); thr.plan(nf, c); force.plan(nf, c); first.plan(nf, c);
    pptr.plan(nf + 1, c); mptr.plan(nf + 1, c); kptr.plan(nf + 1, c); gptr.plan(nf + 1, c);
    ppt.plan(2 * n_prev, c); mb.plan(2 * n_prev, c); age.plan(n_prev, c); track.plan(n_prev, c); pdesc.plan(4 * n_prev, c);
    pcov.plan(n_prev, c); cand.plan(4 * n_prev, c);
    mpt.plan(2 * n_mv, c); dindx.plan(n_mv, c); rect.plan(4 * n_kps, c); covered.plan(n_grid, c); claim.plan(n_kps, c);
    pix.plan(sz.pixel_bytes, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_pos = dv.take<int32_t>(n_prev), o_ord = dv.take<int32_t>(n_prev), o_desc = dv.take<uint64_t>(4 * n_items), o_code = dv.take<int32_t>(n_items);
    const size_t o_rank = dv.take<int32_t>(n_items), o_pt = dv.take<float>(2 * n_prev), o_xy = dv.take<int32_t>(2 * n_prev);
    const size_t o_d = dv.take<int32_t>(n_prev), o_dist = dv.take<int32_t>(n_prev), o_counts = dv.take<int32_t>(3 * nf);
    Out<int32_t> order, chosen, dist, movs, next, seg, fsrc, ftrack, frect, fage;
    Out<uint8_t> fate, found, code, ran;
    Out<float> fpt;
    Out<uint64_t> fdesc;
    order.plan(res->order, n_prev, c); fate.plan(res->fate, n_prev, c); chosen.plan(res->chosen_mv, n_prev, c); dist.plan(res->distance, n_prev, c);
    found.plan(res->kp_found, n_kps, c); code.plan(res->kp_code, n_kps, c);
    movs.plan(res->mov_cnt, nf, c); ran.plan(res->grid_ran, nf, c); next.plan(res->next_id, nf, c); seg.plan(res->seg_ptr, 4 * nf + 1, c);
    fsrc.plan(res->feat_src, n_items, c); ftrack.plan(res->feat_track, n_items, c); fpt.plan(res->feat_pt, 2 * n_items, c);
    frect.plan(res->feat_rect, 4 * n_items, c); fage.plan(res->feat_age, n_items, c); fdesc.plan(res->feat_desc, 4 * n_items, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    rows.fill(sg, d.rows); cols.fill(sg, d.cols); thr.fill(sg, d.threshold); first.fill(sg, d.first_id);
    pptr.fill(sg, d.prev_ptr); mptr.fill(sg, d.mv_ptr); kptr.fill(sg, d.kp_ptr);
    ppt.fill(sg, d.prev_pt); mb.fill(sg, d.prev_mb); age.fill(sg, d.prev_age); track.fill(sg, d.prev_track); pdesc.fill(sg, d.prev_desc);
    pcov.fill(sg, d.prev_coverage); cand.fill(sg, d.prev_cand); mpt.fill(sg, d.mv_pt); dindx.fill(sg, d.mv_dindx); rect.fill(sg, d.kp_rect);
    if (d.grid_ptr) covered.fill(sg, d.grid_covered);
    else if (n_grid) std::memset(covered.host(sg), 0, n_grid);
    if (n_kps) std::memset(claim.host(sg), kAdvNoClaim & 0xff, sizeof(int32_t) * n_kps);
    int32_t *img_off = off.host(sg), *g_ptr = gptr.host(sg), *force_grid = force.host(sg);
    uint8_t *pixels = pix.host(sg);
    size_t px = 0;
    g_ptr[0] = 0;
    for (size_t f = 0; f < nf; ++f) {
        const int64_t ng = adv_lattice(d.rows[f], d.cols[f]);
        g_ptr[f + 1] = g_ptr[f] + (int32_t)ng;
        force_grid[f] = d.force_grid[f] != 0;
        img_off[f] = 0;
        if (d.prev_ptr[f + 1] - d.prev_ptr[f] + d.kp_ptr[f + 1] - d.kp_ptr[f] + ng == 0) continue;
        img_off[f] = (int32_t)px;
        const size_t nc = (size_t)d.cols[f];
        for (size_t y = 0; y < (size_t)d.rows[f]; ++y, px += nc) std::memcpy(pixels + px, d.image[f] + y * (size_t)d.stride[f], nc);
    }

    AdvDev e{};
    e.n_frames = d.n_frames; e.n_items = (int32_t)n_items; e.max_prev = sz.max_prev;
    e.pixels = pix.dev(ar); e.img_off = off.dev(ar); e.rows = rows.dev(ar); e.cols = cols.dev(ar); e.threshold = thr.dev(ar);
    e.force_grid = force.dev(ar); e.first_id = first.dev(ar);
    e.prev_ptr = pptr.dev(ar); e.mv_ptr = mptr.dev(ar); e.kp_ptr = kptr.dev(ar); e.g_ptr = gptr.dev(ar);
    e.prev_pt = ppt.dev(ar); e.mv_pt = mpt.dev(ar); e.prev_mb = mb.dev(ar); e.prev_age = age.dev(ar); e.prev_track = track.dev(ar);
    e.prev_cand = cand.dev(ar); e.prev_desc = pdesc.dev(ar); e.prev_coverage = pcov.dev(ar); e.covered = covered.dev(ar);
    e.mv_dindx = dindx.dev(ar); e.kp_rect = rect.dev(ar);
    e.claim = const_cast<int32_t *>(claim.dev(ar));
    e.pos = at<int32_t>(ar, o_pos); e.ord = at<int32_t>(ar, o_ord); e.it_desc = at<uint64_t>(ar, o_desc); e.it_code = at<int32_t>(ar, o_code); e.it_rank = at<int32_t>(ar, o_rank);
    e.pf_pt = at<float>(ar, o_pt); e.pf_xy = at<int32_t>(ar, o_xy); e.pf_d = at<int32_t>(ar, o_d); e.pf_dist = at<int32_t>(ar, o_dist);
    e.counts = at<int32_t>(ar, o_counts);
    for (Out<int32_t> *o : { &order, &chosen, &dist, &movs, &next, &seg, &fsrc, &ftrack, &frect, &fage }) o->bind(h->stage_dev);
    for (Out<uint8_t> *o : { &fate, &found, &code, &ran }) o->bind(h->stage_dev);
    fpt.bind(h->stage_dev); fdesc.bind(h->stage_dev);
    e.order = order.dev; e.chosen_mv = chosen.dev; e.distance = dist.dev; e.mov_cnt = movs.dev; e.next_id = next.dev; e.seg_ptr = seg.dev;
    e.fate = fate.dev; e.kp_found = found.dev; e.kp_code = code.dev; e.grid_ran = ran.dev;
    e.feat_src = fsrc.dev; e.feat_track = ftrack.dev; e.feat_rect = frect.dev; e.feat_age = fage.dev; e.feat_pt = fpt.dev; e.feat_desc = fdesc.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_advance(e, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (const Out<int32_t> *o : { &order, &chosen, &dist, &movs, &next, &seg, &fsrc, &ftrack, &frect, &fage }) o->fetch(sg);
    for (const Out<uint8_t> *o : { &fate, &found, &code, &ran }) o->fetch(sg);
    fpt.fetch(sg); fdesc.fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

}  // extern "C"
