// The fake device's side of movba_view_points (mov-slam_amd/csrc/view_points.cpp): the launch wrapper of view_points.h as a
// closure on the fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the library's own per-item arithmetic
// (view_points.h) chunk by chunk as k_vp_items does and the serial form of the radix select view by view as k_vp_views does,
// reading every input through the pointers the host laid out, checking that the chunk table covers every view's items exactly
// once, and writing results where the host said - so that the sanitizers see the host's layout and hand-offs and the driver can
// check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <vector>

#include "movba.h"
#include "view_points.h"

namespace {
std::atomic<int> g_vp_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_view_points: %s\n", what);
    g_vp_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_view_points_errors() { return g_vp_errors.load(); }

namespace movba {

static void fake_chunk(const VpDev &d, const VpChunk &ch)
{
    const VpView &pv = d.views[ch.view];
    double view[kVpViewDoubles];
    vp_view(pv, view);
    for (int tid = 0; tid < ch.count; ++tid) {
        const size_t i = (size_t)ch.first + (size_t)tid;
        const size_t p = (size_t)d.item_point[i];
        const double P[3] = { d.points[3 * p], d.points[3 * p + 1], d.points[3 * p + 2] };
        double Pn[3] = { 0.0, 0.0, 0.0 }, dmax = 0.0, dmin = 0.0;
        if (pv.mode != MOVBA_VIEW_DEPTH) {
            Pn[0] = d.normals[3 * p]; Pn[1] = d.normals[3 * p + 1]; Pn[2] = d.normals[3 * p + 2];
            dmax = d.max_dist[p]; dmin = d.min_dist[p];
        }
        const VpItem r = vp_item(pv.mode, pv.n_levels, view, P, Pn, dmax, dmin);
        d.code[i] = r.code;
        d.code_dev[i] = r.code;
        if (d.z) d.z[i] = r.z;
        if (d.uv) { d.uv[2 * i] = r.u; d.uv[2 * i + 1] = r.v; }
        if (d.dist) d.dist[i] = r.dist;
        if (d.view_cos) d.view_cos[i] = r.view_cos;
        if (d.level) d.level[i] = r.level;
        if (d.ur) d.ur[i] = r.ur;
        if (d.track_depth) d.track_depth[i] = r.track_depth;
        if (pv.mode == MOVBA_VIEW_DEPTH) d.keys[pv.key0 + (int64_t)(i - (size_t)pv.item0)] = im_order_key(r.z);
    }
}

static void fake_view(const VpDev &d, int v)
{
    const VpView &pv = d.views[v];
    if (pv.mode != MOVBA_VIEW_DEPTH) {
        int32_t acc = 0;
        for (int32_t i = 0; i < pv.n; ++i) acc += d.code_dev[pv.item0 + i] < MOVBA_VP_REJ_BEHIND;
        d.n_accepted[v] = acc; d.median[v] = __builtin_nan("");
        return;
    }
    d.n_accepted[v] = pv.n;
    d.median[v] = pv.n ? vp_key_value(vp_select_serial(d.keys + pv.key0, pv.n, (pv.n - 1) / pv.q)) : -1.0;
}

hipError_t launch_view_points(const VpDev &dev, hipStream_t s)
{
    const VpDev d = dev;
    fake_enqueue(s, [=] {
        // the chunk table: the views in order, every view's items in order, no chunk longer than a workgroup
        int64_t at = 0, keys = 0;
        int c = 0;
        for (int v = 0; v < d.n_views; ++v) {
            const VpView &pv = d.views[v];
            if (pv.item0 != at) { bad("a view's first item does not follow the view before it"); return; }
            if (pv.mode == MOVBA_VIEW_DEPTH) { if (pv.key0 != keys) { bad("key offsets do not follow the DEPTH views"); return; } keys += pv.n; }
            for (int32_t done = 0; done < pv.n;) {
                if (c >= d.n_chunks) { bad("too few chunks"); return; }
                const VpChunk &ch = d.chunks[c++];
                if (ch.view != v || ch.first != at + done || ch.count < 1 || ch.count > kVpThreads || done + ch.count > pv.n) { bad("a chunk out of place"); return; }
                done += ch.count;
            }
            at += pv.n;
        }
        if (c != d.n_chunks) { bad("too many chunks"); return; }
        for (int k = 0; k < d.n_chunks; ++k) fake_chunk(d, d.chunks[k]);
        for (int v = 0; v < d.n_views; ++v) fake_view(d, v);
    });
    return hipSuccess;
}

}  // namespace movba
