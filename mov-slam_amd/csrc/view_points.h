// Device view + launch wrappers of movba_view_points (view_points.hip; host side: view_points.cpp), and the arithmetic of one
// item as plain C++ (what k_vp_items inlines, and what a host build can run item by item): Frame::isInFrustum's monocular
// branch, the gates at the head of MOVMatcher::Fuse and the depth of KeyFrame::ComputeSceneMedianDepth, as include/movba.h
// restates them.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "init_map.h"       // im_order_key: the total order the median is selected in
#include "movba.h"

namespace movba {

// One view as the host packs it (checked there: a known mode, finite numbers, fx fy > 0, a quaternion that is not zero).
struct VpView {
    int32_t mode, n_levels, q, n;   // n: items of the view
    int64_t item0;                  // its first item in the call's flat item arrays
    int64_t key0;                   // DEPTH: its first slot in the order-key scratch (the DEPTH views' items, in view order)
    double pose[7], cam[4], bf, bounds[4], log_scale, cos_limit;
};

// At most kVpThreads consecutive items of one view: what one workgroup of k_vp_items takes.
struct VpChunk {
    int32_t view, count;
    int64_t first;                  // first item, flat
};

// Everything the two kernels read and write.  Inputs lie in device memory (one packed copy); every out pointer is device memory,
// or a device view of pinned host memory (the staging buffer, or the caller's movba_host_alloc arrays), or nullptr for an
// optional array the caller left out.
struct VpDev {
    int32_t n_views, n_chunks;
    const VpView *views;
    const VpChunk *chunks;
    const int32_t *item_point;      // n_items, every index checked by the host
    const double *points, *normals, *max_dist, *min_dist;       // the point table (the last three nullptr: DEPTH views only)
    uint64_t *keys;                 // scratch: order keys of the DEPTH views' z
    uint8_t *code_dev;              // scratch, n_items: the codes once more, where k_vp_views counts them
    uint8_t *code;                  // n_items out
    double *z, *uv, *dist, *view_cos, *ur, *track_depth;        // n_items (uv: x 2) out or nullptr
    int32_t *level;                 // n_items out or nullptr
    int32_t *n_accepted;            // n_views out
    double *median;                 // n_views out
};

constexpr int kVpThreads = 256;
// a view as the item arithmetic reads it: Rcw row-major [0..8], tcw [9..11], Ow = -Rcw^T tcw [12..14], fx fy cx cy [15..18],
// bf [19], minX maxX minY maxY [20..23], log_scale [24], cos_limit [25]
constexpr int kVpViewDoubles = 26;

// k_vp_items over all chunks, then k_vp_views over all views, on the stream
hipError_t launch_view_points(const VpDev &d, hipStream_t s);

// ---- the arithmetic of one item ----

__host__ __device__ inline void vp_view(const VpView &p, double *v)
{
    double x = p.pose[0], y = p.pose[1], z = p.pose[2], w = p.pose[3];
    const double n = sqrt(x * x + y * y + z * z + w * w);
    x = x / n; y = y / n; z = z / n; w = w / n;
    v[0] = 1.0 - 2.0 * (y * y + z * z); v[1] = 2.0 * (x * y - z * w);       v[2] = 2.0 * (x * z + y * w);
    v[3] = 2.0 * (x * y + z * w);       v[4] = 1.0 - 2.0 * (x * x + z * z); v[5] = 2.0 * (y * z - x * w);
    v[6] = 2.0 * (x * z - y * w);       v[7] = 2.0 * (y * z + x * w);       v[8] = 1.0 - 2.0 * (x * x + y * y);
    const double tx = p.pose[4], ty = p.pose[5], tz = p.pose[6];
    v[9] = tx; v[10] = ty; v[11] = tz;
    v[12] = -(v[0] * tx + v[3] * ty + v[6] * tz);
    v[13] = -(v[1] * tx + v[4] * ty + v[7] * tz);
    v[14] = -(v[2] * tx + v[5] * ty + v[8] * tz);
    for (int k = 0; k < 4; ++k) { v[15 + k] = p.cam[k]; v[20 + k] = p.bounds[k]; }
    v[19] = p.bf; v[24] = p.log_scale; v[25] = p.cos_limit;
}

// What an item gives back: NaN (level -1) where the reference had not computed the value by the time it returned.
struct VpItem {
    double z, u, v, dist, view_cos, ur, track_depth;
    int32_t level;
    uint8_t code;
};

// MapPoint::PredictScale (MapPoint.cc:472-487) with the clamp taken before the conversion: NaN -> 0, +inf -> n_levels - 1
__host__ __device__ inline int32_t vp_level(double max_distance, double dist, double log_scale, int32_t n_levels)
{
    const double s = ceil(log(max_distance / dist) / log_scale);
    if (!(s >= 0.0)) return 0;
    if (s >= (double)n_levels) return n_levels - 1;
    return (int32_t)s;
}

// One item of a view in `mode`: P world position, Pn normal, dmax / dmin the raw mfMaxDistance / mfMinDistance (Pn, dmax, dmin
// are not read for a DEPTH view).
__host__ __device__ inline VpItem vp_item(int32_t mode, int32_t n_levels, const double *v, const double P[3], const double Pn[3],
                                          double dmax, double dmin)
{
    const double nan = __builtin_nan("");
    VpItem r;
    r.u = r.v = r.dist = r.view_cos = r.ur = r.track_depth = nan;
    r.level = -1;
    const double z = v[6] * P[0] + v[7] * P[1] + v[8] * P[2] + v[11];
    r.z = z;
    if (mode == MOVBA_VIEW_DEPTH) { r.code = MOVBA_VP_DEPTH_ITEM; return r; }
    if (z < 0.0) { r.code = MOVBA_VP_REJ_BEHIND; return r; }
    const double x = v[0] * P[0] + v[1] * P[1] + v[2] * P[2] + v[9];
    const double y = v[3] * P[0] + v[4] * P[1] + v[5] * P[2] + v[10];
    const double uu = v[15] * x / z + v[17], vv = v[16] * y / z + v[18];
    r.u = uu; r.v = vv;
    if (mode == MOVBA_VIEW_FRUSTUM) {
        if (uu < v[20] || uu > v[21]) { r.code = MOVBA_VP_REJ_U; return r; }
        if (vv < v[22] || vv > v[23]) { r.code = MOVBA_VP_REJ_V; return r; }
    } else if (!(uu >= v[20] && uu < v[21] && vv >= v[22] && vv < v[23])) {
        r.code = MOVBA_VP_REJ_IMAGE; return r;
    }
    const double po[3] = { P[0] - v[12], P[1] - v[13], P[2] - v[14] };
    const double dist = sqrt(po[0] * po[0] + po[1] * po[1] + po[2] * po[2]);
    r.dist = dist;
    if (dist < 0.8 * dmin || dist > 1.2 * dmax) { r.code = MOVBA_VP_REJ_DIST; return r; }
    const double dot = po[0] * Pn[0] + po[1] * Pn[1] + po[2] * Pn[2];
    if (mode == MOVBA_VIEW_FUSE) {
        r.code = dot < 0.5 * dist ? MOVBA_VP_REJ_ANGLE : MOVBA_VP_FUSE_CANDIDATE;
        return r;
    }
    const double vc = dot / dist;
    r.view_cos = vc;
    if (vc < v[25]) { r.code = MOVBA_VP_REJ_ANGLE; return r; }
    r.level = vp_level(dmax, dist, v[24], n_levels);
    r.ur = uu - v[19] / z;
    r.track_depth = sqrt(x * x + y * y + z * z);
    r.code = MOVBA_VP_VISIBLE;
    return r;
}

// the double whose im_order_key is `key`
__host__ __device__ inline double vp_key_value(uint64_t key)
{
    union { double d; uint64_t u; } c;
    c.u = (key >> 63) ? key & 0x7fffffffffffffffull : ~key;
    return c.d;
}

// The select of k_vp_views, serially: the key of rank `rank` (0-based, rank < n) in the ascending order of keys[0..n), found in
// eight passes of eight bits, most significant first - a 256-bin count of the keys that carry the prefix found so far, then
// the bin that holds the rank.
inline uint64_t vp_select_serial(const uint64_t *keys, int64_t n, int64_t rank)
{
    uint64_t prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        int64_t hist[256] = {};
        for (int64_t i = 0; i < n; ++i)
            if ((keys[i] & mask) == prefix) ++hist[(keys[i] >> shift) & 255];
        int b = 0;
        while (rank >= hist[b]) rank -= hist[b++];
        prefix |= (uint64_t)b << shift;
        mask |= 0xffull << shift;
    }
    return prefix;
}

}  // namespace movba
