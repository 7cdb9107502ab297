// movba_track_match (include/movba.h): the track-id joins of MOVMatcher - SearchForTriangulation's double loop and the mvVFMap
// lookups of SearchByVideoFeature, SearchForInitialization and Fuse - for many queries per call.  The device passes are
// track_match.hip (two kernels, one workgroup per query; the steps with a serial meaning: track_match.h); this file checks the
// call, packs what has to cross the bus into the handle's staging buffer, sends it with ONE copy, queues the two launches and
// hands the results over after ONE synchronisation.  Result arrays that lie in movba_host_alloc memory are written by the
// kernels themselves; others arrive in the staging buffer and are copied out.
#include <cstring>

#include "handle.h"
#include "track_match.h"

using namespace movba;

namespace {

constexpr int32_t kTmMaxEntries = 1 << 28;

// a prefix array of n + 1 entries: starts at 0, ascends, ends at or below 2^28
bool tm_prefix_ok(const int32_t *ptr, size_t n)
{
    if (!ptr || ptr[0] != 0) return false;
    for (size_t k = 0; k < n; ++k)
        if (ptr[k + 1] < ptr[k]) return false;
    return ptr[n] <= kTmMaxEntries;
}

// the counts alone: what is checked before a call without queries is let through
bool tm_counts_ok(const movba_track_desc &d)
{
    return d.n_views >= 0 && d.n_queries >= 0 && d.n_queries <= MOVBA_MAX_TRACK_QUERIES;
}

// everything else about the call that can be wrong, checked before anything is queued or written (n_queries > 0); match_cap
// and the largest view a query searches come out of the same walk
bool tm_desc_ok(const movba_track_desc &d, const movba_track_result &r, int32_t *match_cap, int32_t *max_slots)
{
    const size_t nv = (size_t)d.n_views, nq = (size_t)d.n_queries;
    if (!d.query_mode || !d.query_view || !d.query_ptr || !r.pair_ptr || !r.n_found) return false;
    if (!tm_prefix_ok(d.view_ptr, nv)) return false;
    for (size_t v = 0; v < nv; ++v)
        if (d.view_ptr[v + 1] - d.view_ptr[v] > MOVBA_MAX_TRACK_SLOTS) return false;
    if (d.view_ptr[nv] > 0 && !d.slot_track) return false;
    if (!tm_prefix_ok(d.query_ptr, nq)) return false;
    if (d.query_ptr[nq] > 0 && (!d.item_track || !r.item_slot)) return false;
    int64_t cap = 0;
    int32_t widest = 0;
    for (size_t q = 0; q < nq; ++q) {
        const int32_t mode = d.query_mode[q], v1 = d.query_view[2 * q], v2 = d.query_view[2 * q + 1];
        if (mode != MOVBA_TM_TRIANGULATION && mode != MOVBA_TM_LOOKUP) return false;
        if (v2 < 0 || v2 >= d.n_views) return false;
        if (mode == MOVBA_TM_LOOKUP) {
            if (v1 != -1) return false;
        } else {
            if (v1 < 0 || v1 >= d.n_views || d.query_ptr[q + 1] != d.query_ptr[q]) return false;
            cap += d.view_ptr[v1 + 1] - d.view_ptr[v1];
        }
        const int32_t n2 = d.view_ptr[v2 + 1] - d.view_ptr[v2];
        if (n2 > widest) widest = n2;
    }
    if (cap > kTmMaxEntries) return false;
    if (cap > 0 && (!r.match_slot1 || !r.match_slot2)) return false;
    if (((r.obs1 || r.obs2) && !d.slot_obs) || ((r.ur1 || r.ur2) && !d.slot_ur) || ((r.depth1 || r.depth2) && !d.slot_depth)) return false;
    *match_cap = (int32_t)cap;
    *max_slots = widest;
    return true;
}

const uint64_t *bits(const double *p) { return reinterpret_cast<const uint64_t *>(p); }
uint64_t *bits(double *p) { return reinterpret_cast<uint64_t *>(p); }

}  // namespace

extern "C" {

int movba_track_match(movba_handle *h, const movba_track_desc *desc, movba_track_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_track_desc &d = *desc;
    if (!tm_counts_ok(d)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_queries == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    int32_t match_cap = 0, max_slots = 0;
    if (!tm_desc_ok(d, *res, &match_cap, &max_slots)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t nv = (size_t)d.n_views, nq = (size_t)d.n_queries, ns = (size_t)d.view_ptr[nv], n_items = (size_t)d.query_ptr[nq];
    const size_t cap = (size_t)match_cap;
    // (a payload array crosses the bus only if one of its outputs was asked for)
    const bool want_obs = cap && (res->obs1 || res->obs2), want_ur = cap && (res->ur1 || res->ur2), want_depth = cap && (res->depth1 || res->depth2);

    // Layout.  [0, h2d): the inputs, one H2D copy into the handle's side-call scratch.  Behind them on the device: the queries'
    // rows and counts; behind them in the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<int32_t> vptr, track, qmode, qview, qptr, items, rbase;
    In<uint8_t> taken;
    In<uint64_t> sobs, sur, sdepth;
    vptr.plan(nv + 1, c); track.plan(ns, c); taken.plan(d.slot_taken ? ns : 0, c);
    sobs.plan(want_obs ? 2 * ns : 0, c); sur.plan(want_ur ? ns : 0, c); sdepth.plan(want_depth ? ns : 0, c);
    qmode.plan(nq, c); qview.plan(2 * nq, c); qptr.plan(nq + 1, c); items.plan(n_items, c); rbase.plan(nq + 1, c);
    const size_t h2d = c.off;
    Carver dv = c;
    const size_t o_row1 = dv.take<int32_t>(cap), o_row2 = dv.take<int32_t>(cap), o_count = dv.take<int32_t>(nq);
    Out<int32_t> pptr, slot1, slot2, islot, found;
    Out<uint64_t> obs1, obs2, ur1, ur2, depth1, depth2;
    pptr.plan(res->pair_ptr, nq + 1, c); slot1.plan(res->match_slot1, cap, c); slot2.plan(res->match_slot2, cap, c);
    obs1.plan(bits(res->obs1), 2 * cap, c); obs2.plan(bits(res->obs2), 2 * cap, c); ur1.plan(bits(res->ur1), cap, c); ur2.plan(bits(res->ur2), cap, c);
    depth1.plan(bits(res->depth1), cap, c); depth2.plan(bits(res->depth2), cap, c);
    islot.plan(res->item_slot, n_items, c); found.plan(res->n_found, nq, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, dv.off, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    vptr.fill(sg, d.view_ptr); track.fill(sg, d.slot_track); taken.fill(sg, d.slot_taken);
    sobs.fill(sg, bits(d.slot_obs)); sur.fill(sg, bits(d.slot_ur)); sdepth.fill(sg, bits(d.slot_depth));
    qmode.fill(sg, d.query_mode); qview.fill(sg, d.query_view); qptr.fill(sg, d.query_ptr); items.fill(sg, d.item_track);
    int32_t *row_base = rbase.host(sg);
    row_base[0] = 0;
    for (size_t q = 0; q < nq; ++q) {
        const int32_t v1 = d.query_view[2 * q];
        row_base[q + 1] = row_base[q] + (d.query_mode[q] == MOVBA_TM_TRIANGULATION ? d.view_ptr[v1 + 1] - d.view_ptr[v1] : 0);
    }

    TmDev t{};
    t.n_queries = d.n_queries; t.match_cap = match_cap;
    t.view_ptr = vptr.dev(ar); t.slot_track = track.dev(ar); t.slot_taken = taken.dev(ar);
    t.slot_obs = sobs.dev(ar); t.slot_ur = sur.dev(ar); t.slot_depth = sdepth.dev(ar);
    t.query_mode = qmode.dev(ar); t.query_view = qview.dev(ar); t.query_ptr = qptr.dev(ar); t.item_track = items.dev(ar);
    t.row_base = rbase.dev(ar);
    t.row_slot1 = at<int32_t>(ar, o_row1); t.row_slot2 = at<int32_t>(ar, o_row2); t.count = at<int32_t>(ar, o_count);
    for (Out<int32_t> *o : { &pptr, &slot1, &slot2, &islot, &found }) o->bind(h->stage_dev);
    for (Out<uint64_t> *o : { &obs1, &obs2, &ur1, &ur2, &depth1, &depth2 }) o->bind(h->stage_dev);
    t.pair_ptr = pptr.dev; t.match_slot1 = slot1.dev; t.match_slot2 = slot2.dev; t.item_slot = islot.dev; t.n_found = found.dev;
    t.obs1 = obs1.dev; t.obs2 = obs2.dev; t.ur1 = ur1.dev; t.ur2 = ur2.dev; t.depth1 = depth1.dev; t.depth2 = depth2.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_track_match(t, max_slots, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (const Out<int32_t> *o : { &pptr, &slot1, &slot2, &islot, &found }) o->fetch(sg);
    for (const Out<uint64_t> *o : { &obs1, &obs2, &ur1, &ur2, &depth1, &depth2 }) o->fetch(sg);
    res->n_matches = res->pair_ptr[nq];
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

}  // extern "C"
