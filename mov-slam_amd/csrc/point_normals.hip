// The two kernels of movba_point_normals and movba_lba_point_normals (include/movba.h).
//
// k_pn_centres: one thread per view.  The camera centre Ow = -Rcw^T tcw is computed ONCE per view (point_normals.h: pn_centre,
// through view_points.h's vp_view) and left in device memory, 24 bytes a view: no limit on the number of views, and at any
// window a map has the table stays in L2 (60 keyframes: 1.4 KB).
//
// k_pn_points: one thread per map point, one wave per workgroup (20 000 points are 313 workgroups: every CU gets one).  The
// thread walks its point's list front to back - the sum is sequential by contract, so there is nothing for a second lane to do
// on one point - through pn_point, the one per-point function of both entry points; the two differ only in the PnLists the
// host hands over (the call's own obs_ptr / obs_view, or the resident window's pt_start / g_pose / perm with this call's copy
// of the outlier flags) and in where the estimate lies.  Neighbouring lanes own neighbouring points, whose lists are
// neighbouring runs of ONE array: a wave's 64 lists (350 indices at the 5.5 observations a point of the headline window has)
// span a few consecutive cache lines that its lanes share from step to step, so the uncoalesced walk costs no extra traffic
// - the call moves 2 MB at that window and is bound by its launches, not by memory; staging the lists through LDS would add a
// barrier and save nothing measurable.  What does serialise is a hub point: a list of thousands of observers is walked by one
// lane while the other 63 of its wave wait.  A point's result is written by its own thread and depends on nothing
// but its list in its order, the views it names, its reference entries and the table.  No atomics of any kind.
#include <hip/hip_runtime.h>

#include "point_normals.h"

namespace movba {

namespace {

__global__ __launch_bounds__(kPnThreads) void k_pn_centres(const PnDev d)
{
    const int v = blockIdx.x * kPnThreads + threadIdx.x;
    if (v >= d.n_views) return;
    const double *poses = d.cur ? d.pose_st[*d.cur & 1] : d.poses;
    double Ow[3];
    pn_centre(poses + 7 * (size_t)v, Ow);
    d.centres[3 * (size_t)v] = Ow[0]; d.centres[3 * (size_t)v + 1] = Ow[1]; d.centres[3 * (size_t)v + 2] = Ow[2];
}

__global__ __launch_bounds__(kPnThreads) void k_pn_points(const PnDev d)
{
    const size_t p = (size_t)blockIdx.x * kPnThreads + threadIdx.x;
    if (p >= (size_t)d.n_points) return;
    const double *points = d.cur ? d.point_st[*d.cur & 1] : d.points;
    const double P[3] = { points[3 * p], points[3 * p + 1], points[3 * p + 2] };
    const PnPoint r = pn_point(P, d.lists, p, d.centres, d.ref_view[p], d.ref_level[p], d.scale, d.n_levels);
    d.normals[3 * p] = r.normal[0]; d.normals[3 * p + 1] = r.normal[1]; d.normals[3 * p + 2] = r.normal[2];
    d.max_dist[p] = r.max_distance;
    d.min_dist[p] = r.min_distance;
}

}  // namespace

hipError_t launch_point_normals(const PnDev &d, hipStream_t s)
{
    if (d.n_views > 0) hipLaunchKernelGGL(k_pn_centres, dim3((d.n_views + kPnThreads - 1) / kPnThreads), dim3(kPnThreads), 0, s, d);
    if (d.n_points > 0) hipLaunchKernelGGL(k_pn_points, dim3((d.n_points + kPnThreads - 1) / kPnThreads), dim3(kPnThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
