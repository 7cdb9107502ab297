// Device view + launch wrapper of movba_point_normals and movba_lba_point_normals (point_normals.hip; host side:
// point_normals.cpp), and the arithmetic of one map point as plain C++ (what k_pn_points inlines for both entry points, and
// what a host build can run point by point): the numeric body of MapPoint::UpdateNormalAndDepth (MapPoint.cc:362-435), as
// include/movba.h restates it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "movba.h"
#include "view_points.h"    // vp_view: the camera centre both calls agree on to the bit

namespace movba {

// Where the observation lists of the points come from.  Point p's observers are view[k] for k in [ptr[p], ptr[p + 1]), in that
// order; entry k is skipped when mask[perm ? perm[k] : k] is non-zero.
//   movba_point_normals:      ptr = obs_ptr, view = obs_view, perm = mask = nullptr
//   movba_lba_point_normals:  ptr = DevWindow::pt_start, view = DevWindow::g_pose (the uploaded edges grouped by point, stable:
//                             caller order inside a point), perm = DevWindow::perm (grouped position -> caller edge; nullptr:
//                             identity), mask = this call's copy of the caller's outlier flags, caller edge order, or nullptr
struct PnLists {
    const int32_t *ptr, *view, *perm;
    const uint8_t *mask;
};

// Everything the two kernels read and write.  Inputs lie in device memory; every out pointer is device memory or a device view
// of pinned host memory (the staging buffer, or the caller's movba_host_alloc arrays).
struct PnDev {
    int32_t n_views, n_points, n_levels, pad;
    // the estimate: poses n_views x 7 and points n_points x 3 of this call's packed copy, or (cur != nullptr) those of a
    // resident window's current state: pose_st[*cur], point_st[*cur] (DevState::pose / point, Ctrl::cur)
    const double *poses, *points;
    const int32_t *cur;
    const double *pose_st[2], *point_st[2];
    PnLists lists;
    const int32_t *ref_view, *ref_level;    // n_points each, every entry that is read checked by the host
    const double *scale;                    // n_levels
    double *centres;                        // scratch, n_views x 3: Ow of every view, written by k_pn_centres
    double *normals, *max_dist, *min_dist;  // out: n_points x 3, n_points, n_points
};

constexpr int kPnThreads = 64;

// k_pn_centres over all views, then k_pn_points over all points, on the stream
hipError_t launch_point_normals(const PnDev &d, hipStream_t s);

// ---- the arithmetic ----

// Ow = -Rcw^T tcw of one pose (qx qy qz qw tx ty tz, quaternion normalised first): KeyFrame::GetCameraCenter, through the very
// function movba_view_points derives a view's centre with
__host__ __device__ inline void pn_centre(const double pose[7], double Ow[3])
{
    VpView w{};
    for (int e = 0; e < 7; ++e) w.pose[e] = pose[e];
    double v[kVpViewDoubles];
    vp_view(w, v);
    Ow[0] = v[12]; Ow[1] = v[13]; Ow[2] = v[14];
}

struct PnPoint { double normal[3], max_distance, min_distance; };

// Point p at world position P: the mean of the unit vectors from its observers' centres, summed strictly in list order
// (MapPoint.cc:383-396, :433), and the distance to its reference keyframe's centre scaled by the pyramid (:406-407, :426-432).
// ref_view is not read when the list is empty (or every entry of it is masked): the five numbers are NaN then (:377).
__host__ __device__ inline PnPoint pn_point(const double P[3], const PnLists &L, size_t p, const double *centres, int32_t ref_view,
                                            int32_t ref_level, const double *scale, int32_t n_levels)
{
    PnPoint r;
    double ax = 0.0, ay = 0.0, az = 0.0;
    int32_t n = 0;
    const int32_t k1 = L.ptr[p + 1];
    for (int32_t k = L.ptr[p]; k < k1; ++k) {
        if (L.mask && L.mask[L.perm ? L.perm[k] : k]) continue;
        const double *O = centres + 3 * (size_t)L.view[k];
        const double dx = P[0] - O[0], dy = P[1] - O[1], dz = P[2] - O[2];
        const double len = sqrt(dx * dx + dy * dy + dz * dz);
        ax = ax + dx / len;
        ay = ay + dy / len;
        az = az + dz / len;
        ++n;
    }
    if (n == 0) {
        const double nan = __builtin_nan("");
        r.normal[0] = r.normal[1] = r.normal[2] = r.max_distance = r.min_distance = nan;
        return r;
    }
    const double cnt = (double)n;
    r.normal[0] = ax / cnt; r.normal[1] = ay / cnt; r.normal[2] = az / cnt;
    const double *O = centres + 3 * (size_t)ref_view;
    const double dx = P[0] - O[0], dy = P[1] - O[1], dz = P[2] - O[2];
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);
    r.max_distance = dist * scale[ref_level];
    r.min_distance = r.max_distance / scale[n_levels - 1];
    return r;
}

}  // namespace movba
