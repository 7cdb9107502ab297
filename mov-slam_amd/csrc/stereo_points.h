// Device view + launch wrapper of movba_stereo_points (stereo_points.hip; host side: stereo_points.cpp), and every rule of the call
// as plain C++ - the gates behind the stereo LK call with the integer distance, the threshold of the median rule, the selection
// key, the length of the depth-ordered walk, the un-projection - once, for both sides: what the kernels call, and what a host
// build runs frame by frame (st_frames), as lk.h does with lk_frames.  Frame::ComputeStereoMatches behind its LK call
// (Frame.cc:306-353), Frame::UnprojectStereo (:836-851) and the walks of Tracking::StereoInitialization (Tracking.cc:532-547),
// CreateNewKeyFrame (:1022-1098) and UpdateLastFrame (:828-887), as include/movba.h restates them.
//
// Everything up to sel_cam is fp32, one operation per statement, and contraction is off for all of this file on both sides;
// sel_point is fp64 without FMA.  The order of a frame's candidates is decided on integers alone: the distances are ints, the
// selection keys are the depths' bits above the index.
//
// Out of scope: cv::undistortPoints for non-zero distortion (the caller passes pt_un; every shipped stereo configuration has
// zero distortion), the N > 500 test of StereoInitialization, MapPoint / KeyFrame construction, track ids and
// UpdateNormalAndDepth (movba_point_normals), AssignFeaturesToGrid, and the fisheye branches (Nleft != -1), which never run.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "movba.h"
#include "view_points.h"    // vp_view: the pose -> rotation, centre that movba_view_points and pn_centre use

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace movba {

constexpr int kStThreads = 1024;                    // k_st_frame: one workgroup per frame
constexpr int kStWaves = kStThreads / 64;
constexpr int kStEmitThreads = 256;                 // k_st_emit
constexpr int kStEmitWaves = kStEmitThreads / 64;
constexpr int kStEmitChunks = 64;                   // k_st_emit: at most that many workgroups per frame
constexpr int kStMinLds = 2048;                     // k_st_frame: 256 bins and the waves' partial sums, where nothing is sorted
constexpr int32_t kStNoDist = -1;                   // the distance of a point the gates did not accept

// One frame as the host packs it (checked there).  Rwc and Ow are derived on the host, once per frame, by vp_view - the function
// behind movba_view_points' views and pn_centre - so the kernels and the serial walk read the same twelve doubles; without
// poses they are the identity and zero (SetPose(SE3f()), Tracking.cc:524).  The host has no FMA where view_points.hip and
// point_normals.hip, built with -ffp-contract=on, may fuse vp_view's products on the device: a centre can differ from theirs in
// the last bit.
struct StFrame {
    int32_t rows, cols, select, pad;
    float bf, max_disparity, th_depth, fx, fy, cx, cy, pad2;
    double Rwc[9], Ow[3];
};

// Everything the kernels read and write.  Inputs and scratch lie in device memory; every out pointer is device memory or a device
// view of pinned host memory, written once or twice and never read.
struct StDev {
    int32_t n_frames, n_pt, max_point, max_close;   // max_close: the points of the largest MOVBA_STEREO_SELECT_CLOSE frame
    int32_t max_frame, pad;                         // max_frame: the points of the largest frame
    float max_row_diff, min_disparity;
    const StFrame *frame;                           // n_frames
    const int32_t *pt_ptr;                          // n_frames + 1
    const float *pt, *next_pt, *pt_un;              // n_pt x 2 (pt_un: the caller's, or pt)
    const uint8_t *pt_status, *has_point;           // n_pt (has_point: nullptr = all 0)
    // scratch
    int32_t *dist;                                  // n_pt: the int distance, kStNoDist where the gates refused
    float *z;                                       // n_pt: depth as it stands (what the selection and the emit read back)
    int32_t *list;                                  // n_pt: a frame's selected points in walk order, at the frame's own offset
    int32_t *counts;                                // n_frames: how many
    // out
    float *u_right, *depth;
    uint8_t *code;
    int32_t *n_stereo, *median_dist;
    float *th_dist;
    int32_t *sel_ptr, *sel_src;
    uint8_t *sel_new;
    float *sel_cam;
    double *sel_point;
};

// k_st_frame over the frames, then k_st_emit, on the stream
hipError_t launch_stereo_points(const StDev &d, hipStream_t s);

// ---- the steps ----

__host__ __device__ inline int32_t st_pow2ceil(int32_t n)
{
    int32_t m = 1;
    while (m < n) m <<= 1;
    return m;
}

struct StGate { float u_right, depth; int32_t dist; uint8_t code; };

// Frame.cc:312-337 for one keypoint: L = mvKeys[i].pt, R = pts_out[i].  rows and cols are the right image's.
__host__ __device__ inline StGate st_gate(float lx, float ly, float rx, float ry, uint8_t status, int32_t rows, int32_t cols, float bf,
                                          float max_row_diff, float min_disparity, float max_disparity)
{
    StGate g{ -1.f, -1.f, kStNoDist, MOVBA_STEREO_REJ_STATUS };
    if (status == 0 || rx < 0.f || ry < 0.f || rx >= (float)cols || ry >= (float)rows) return g;
    const float row = ry - ly;
    if (fabsf(row) > max_row_diff) { g.code = MOVBA_STEREO_REJ_ROW; return g; }
    float disparity = lx - rx;
    if (!(disparity >= min_disparity && disparity < max_disparity)) { g.code = MOVBA_STEREO_REJ_DISPARITY; return g; }
    float best = rx;
    if (disparity <= 0.f) {
        disparity = (float)0.01;
        const double moved = (double)lx - 0.01;     // (the source subtracts a double literal)
        best = (float)moved;
    }
    g.depth = bf / disparity;
    g.u_right = best;
    // cv::norm(Point2f) [opencv-upstream]: the difference in fp32, its length in fp64, stored through a float into an int
    const float dx = lx - rx, dy = ly - ry;
    const double xx = (double)dx * (double)dx, yy = (double)dy * (double)dy, sum = xx + yy;
    const float len = (float)sqrt(sum);
    g.dist = (int32_t)len;
    g.code = MOVBA_STEREO_OK;
    return g;
}

// thDist of Frame.cc:342, left to right
__host__ __device__ inline float st_threshold(int32_t median)
{
    const float a = 1.5f * 1.4f;
    return a * (float)median;
}

// pruned by Frame.cc:344-353: sorted pairs walked from the back until the first below thDist = every pair at or above it
__host__ __device__ inline bool st_far(int32_t dist, float th_dist) { return (float)dist >= th_dist; }

// the rank of the upper median among n sorted values: pairs[size / 2]
__host__ __device__ inline int32_t st_median_rank(int32_t n) { return n / 2; }

// The order of the depth-sorted walk: a positive float's bits order as an unsigned int, the index breaks ties and makes the
// keys distinct; all-ones pads.
__host__ __device__ inline uint64_t st_key(float z, int32_t i)
{
    union { float f; uint32_t u; } c;
    c.f = z;
    return ((uint64_t)c.u << 32) | (uint32_t)i;
}
__host__ __device__ inline int32_t st_key_index(uint64_t key) { return (int32_t)(uint32_t)key; }

// How many entries Tracking.cc:1050-1093 and :850-884 list: entry j is listed, then the walk stops if z_j > mThDepth and
// nPoints (= j + 1) > max_point.  n_close of the n_cand sorted candidates have z <= mThDepth.
__host__ __device__ inline int32_t st_list_len(int32_t n_cand, int32_t n_close, int32_t max_point)
{
    const int32_t last = n_close > max_point ? n_close : max_point;
    return n_cand <= last ? n_cand : last + 1;
}

// Frame.cc:843-845, left to right
__host__ __device__ inline void st_unproject(float u, float v, float z, const StFrame &fr, float cam[3])
{
    const float invfx = 1.0f / fr.fx, invfy = 1.0f / fr.fy;
    const float du = u - fr.cx, dv = v - fr.cy;
    const float xz = du * z, yz = dv * z;
    cam[0] = xz * invfx; cam[1] = yz * invfy; cam[2] = z;
}

// x3D = Rwc * cam + Ow in fp64: each row's products summed left to right, then the centre
__host__ __device__ inline void st_world(const float cam[3], const StFrame &fr, double world[3])
{
    const double x = (double)cam[0], y = (double)cam[1], z = (double)cam[2];
    for (int k = 0; k < 3; ++k) {
        const double a = fr.Rwc[3 * k] * x, b = fr.Rwc[3 * k + 1] * y, c = fr.Rwc[3 * k + 2] * z;
        const double ab = a + b, abc = ab + c;
        world[k] = abc + fr.Ow[k];
    }
}

// Rwc and Ow of a frame from Tcw (qx qy qz qw tx ty tz), or the identity for pose == nullptr
__host__ __device__ inline void st_frame_pose(const double *pose, StFrame *fr)
{
    for (int k = 0; k < 9; ++k) fr->Rwc[k] = k % 4 == 0 ? 1.0 : 0.0;
    fr->Ow[0] = fr->Ow[1] = fr->Ow[2] = 0.0;
    if (!pose) return;
    VpView w{};
    for (int e = 0; e < 7; ++e) w.pose[e] = pose[e];
    double v[kVpViewDoubles];
    vp_view(w, v);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) fr->Rwc[3 * r + c] = v[3 * c + r];
    fr->Ow[0] = v[12]; fr->Ow[1] = v[13]; fr->Ow[2] = v[14];
}

// ---- the passes over a frame's points, a point at a time (the kernels stride over them, the host walks them) ----

// the gates of point i (flat) of frame fr: scratch and the provisional u_right and code
__host__ __device__ inline void st_gate_point(const StDev &d, const StFrame &fr, size_t i)
{
    const StGate g = st_gate(d.pt[2 * i], d.pt[2 * i + 1], d.next_pt[2 * i], d.next_pt[2 * i + 1], d.pt_status[i], fr.rows, fr.cols, fr.bf,
                             d.max_row_diff, d.min_disparity, fr.max_disparity);
    d.dist[i] = g.dist; d.z[i] = g.depth;
    d.u_right[i] = g.u_right; d.code[i] = g.code;
}

// the median rule on point i (a frame without a candidate has no point with a distance) -> the depth that stands
__host__ __device__ inline float st_prune_point(const StDev &d, size_t i, float th_dist)
{
    const int32_t dist = d.dist[i];
    float z = d.z[i];
    if (dist != kStNoDist && st_far(dist, th_dist)) {
        z = -1.f;
        d.z[i] = z; d.u_right[i] = -1.f; d.code[i] = MOVBA_STEREO_REJ_FAR;
    }
    d.depth[i] = z;
    return z;
}

// selected entry j of a frame (points from p0, the frame's first entry of the dense lists at `before`)
__host__ __device__ inline void st_emit_item(const StDev &d, const StFrame &fr, int32_t p0, int32_t before, int32_t j)
{
    const int32_t idx = d.list[p0 + j];
    const size_t i = (size_t)p0 + idx, o = (size_t)before + j;
    float cam[3];
    double world[3];
    st_unproject(d.pt_un[2 * i], d.pt_un[2 * i + 1], d.z[i], fr, cam);
    st_world(cam, fr, world);
    d.sel_src[o] = idx;
    d.sel_new[o] = d.has_point && d.has_point[i] ? 0 : 1;
    for (int k = 0; k < 3; ++k) { d.sel_cam[3 * o + k] = cam[k]; d.sel_point[3 * o + k] = world[k]; }
}

// entry o of the dense lists behind the call's total
__host__ __device__ inline void st_pad(const StDev &d, size_t o)
{
    const float nanf_ = __builtin_nanf("");
    const double nan = __builtin_nan("");
    d.sel_src[o] = -1; d.sel_new[o] = 0;
    for (int k = 0; k < 3; ++k) { d.sel_cam[3 * o + k] = nanf_; d.sel_point[3 * o + k] = nan; }
}

// The select of k_st_frame, serially: the value of rank `rank` (0-based, below the number of candidates) among the distances
// that are not kStNoDist, in four passes of eight bits, most significant first - a 256-bin count of the values that carry the
// prefix found so far, then the bin that holds the rank.
inline int32_t st_select_serial(const int32_t *dist, int32_t n, int32_t rank)
{
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        int32_t hist[256] = {};
        for (int32_t i = 0; i < n; ++i)
            if (dist[i] != kStNoDist && ((uint32_t)dist[i] & mask) == prefix) ++hist[((uint32_t)dist[i] >> shift) & 255];
        int b = 0;
        while (rank >= hist[b]) rank -= hist[b++];
        prefix |= (uint32_t)b << shift;
        mask |= 0xffu << shift;
    }
    return (int32_t)prefix;
}

// the whole call, serially, in the kernels' order (host builds: the fake launch of tests/stereo_points and stereo_main.cpp,
// which tests/dev/stereo_time.py times).  The keys are distinct, so the sort's method cannot change the outcome.
inline void st_frames(const StDev &d)
{
    int32_t total = 0;
    std::vector<uint64_t> keys;
    for (int32_t f = 0; f < d.n_frames; ++f) {
        const StFrame &fr = d.frame[f];
        const int32_t p0 = d.pt_ptr[f], n = d.pt_ptr[f + 1] - p0;
        int32_t n_cand = 0;
        for (int32_t i = 0; i < n; ++i) {
            st_gate_point(d, fr, (size_t)p0 + i);
            if (d.dist[p0 + i] != kStNoDist) ++n_cand;
        }
        const int32_t median = n_cand ? st_select_serial(d.dist + p0, n, st_median_rank(n_cand)) : -1;
        const float th = n_cand ? st_threshold(median) : 0.f;
        int32_t n_stereo = 0, n_close = 0;
        for (int32_t i = 0; i < n; ++i) {
            const float z = st_prune_point(d, (size_t)p0 + i, th);
            if (z > 0.f) { ++n_stereo; if (z <= fr.th_depth) ++n_close; }
        }
        d.n_stereo[f] = n_stereo; d.median_dist[f] = median; d.th_dist[f] = th;
        int32_t count = 0;
        if (fr.select == MOVBA_STEREO_SELECT_ALL) {
            for (int32_t i = 0; i < n; ++i)
                if (d.z[p0 + i] > 0.f) d.list[p0 + count++] = i;
        } else if (fr.select == MOVBA_STEREO_SELECT_CLOSE && n_stereo > 0) {
            keys.clear();
            for (int32_t i = 0; i < n; ++i)
                if (d.z[p0 + i] > 0.f) keys.push_back(st_key(d.z[p0 + i], i));
            std::sort(keys.begin(), keys.end());
            count = st_list_len(n_stereo, n_close, d.max_point);
            for (int32_t j = 0; j < count; ++j) d.list[p0 + j] = st_key_index(keys[j]);
        }
        d.counts[f] = count;
        d.sel_ptr[f] = total;
        for (int32_t j = 0; j < count; ++j) st_emit_item(d, fr, p0, total, j);
        total += count;
    }
    d.sel_ptr[d.n_frames] = total;
    for (int32_t o = total; o < d.n_pt; ++o) st_pad(d, (size_t)o);
}

}  // namespace movba
