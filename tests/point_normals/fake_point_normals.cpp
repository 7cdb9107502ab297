// The fake device's side of movba_point_normals and movba_lba_point_normals (mov-slam_amd/csrc/point_normals.cpp): the launch
// wrapper of point_normals.h as a closure on the fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the
// library's own arithmetic (point_normals.h) view by view as k_pn_centres does and point by point as k_pn_points does, reading
// every input through the pointers the host laid out - checking every index on the way, so that a list the host packed wrongly is
// reported rather than followed - and writing results where the host said: the sanitizers see the host's layout and hand-offs,
// and the driver can check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "movba.h"
#include "point_normals.h"

namespace {
std::atomic<int> g_pn_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_point_normals: %s\n", what);
    g_pn_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_point_normals_errors() { return g_pn_errors.load(); }

namespace movba {

hipError_t launch_point_normals(const PnDev &dev, hipStream_t s)
{
    const PnDev d = dev;
    fake_enqueue(s, [=] {
        if (d.cur && (*d.cur < 0 || *d.cur > 1)) { bad("the window's current state is neither 0 nor 1"); return; }
        const double *poses = d.cur ? d.pose_st[*d.cur] : d.poses, *points = d.cur ? d.point_st[*d.cur] : d.points;
        const PnLists &L = d.lists;
        if (d.n_points > 0 && L.ptr[0] != 0) { bad("the lists do not start at 0"); return; }
        for (int32_t p = 0; p < d.n_points; ++p) {
            if (L.ptr[p + 1] < L.ptr[p]) { bad("the lists' prefix descends"); return; }
            if (d.ref_level[p] < 0 || d.ref_level[p] >= d.n_levels) { bad("an octave out of range"); return; }
            bool any = false;
            for (int32_t k = L.ptr[p]; k < L.ptr[p + 1]; ++k) {
                if (L.view[k] < 0 || L.view[k] >= d.n_views) { bad("an observer out of range"); return; }
                if (L.perm && (L.perm[k] < 0 || L.perm[k] >= L.ptr[d.n_points])) { bad("a grouped position maps to no edge"); return; }
                any = any || !(L.mask && L.mask[L.perm ? L.perm[k] : k]);
            }
            if (any && (d.ref_view[p] < 0 || d.ref_view[p] >= d.n_views)) { bad("a reference view that is read is out of range"); return; }
        }
        for (int32_t v = 0; v < d.n_views; ++v) pn_centre(poses + 7 * (size_t)v, d.centres + 3 * (size_t)v);
        for (int32_t p = 0; p < d.n_points; ++p) {
            const PnPoint r = pn_point(points + 3 * (size_t)p, L, (size_t)p, d.centres, d.ref_view[p], d.ref_level[p], d.scale, d.n_levels);
            for (int k = 0; k < 3; ++k) d.normals[3 * (size_t)p + k] = r.normal[k];
            d.max_dist[p] = r.max_distance; d.min_dist[p] = r.min_distance;
        }
    });
    return hipSuccess;
}

}  // namespace movba
