// movba_view_points' two kernels (include/movba.h).
//
// k_vp_items: one thread per item, flat over all items of the call, 256 per workgroup; the arithmetic of an item is
// view_points.h.  A workgroup takes one chunk of the host's table - at most 256 consecutive items of ONE view - so the view
// (rotation from the quaternion, translation, camera centre, camera, bounds: 26 doubles) is computed once per workgroup into
// LDS and every lane reads it from there (same address in every lane: a broadcast).  An item's result is written by its own
// thread and depends on nothing but the item and its view.  The code goes out twice: to the caller (pinned host memory) and
// to a device array that k_vp_views counts; a DEPTH item's z also goes, as its 64-bit order key, into the select's scratch.
//
// k_vp_views: one workgroup of 256 threads per view.  n_accepted is an integer count over the view's codes.  The median of a
// DEPTH view is found exactly by a radix select on the order keys: eight passes of eight bits, most significant first; in
// each the threads stride over the list and count the keys that carry the prefix found so far into a 256-bin LDS histogram
// (integer atomics: the counts do not depend on arrival order), then wave 0 scans the bins, picks the one that holds the wanted
// rank and fixes eight more bits.  After the last pass the key is known completely and the value is its inverse; equal keys
// are equal bit patterns, so there is no tie to break.  O(n) per view, read eight times (from L2 at any list a frame has).
// No floating-point atomics anywhere.
#include <hip/hip_runtime.h>

#include "view_points.h"

namespace movba {

namespace {

__global__ __launch_bounds__(kVpThreads) void k_vp_items(const VpDev d)
{
    __shared__ double view[kVpViewDoubles];
    __shared__ int32_t meta[2];
    const int tid = threadIdx.x;
    const VpChunk ch = d.chunks[blockIdx.x];
    const VpView *pv = d.views + ch.view;
    if (tid == 0) { vp_view(*pv, view); meta[0] = pv->mode; meta[1] = pv->n_levels; }
    __syncthreads();
    if (tid >= ch.count) return;
    const int32_t mode = meta[0];
    const size_t i = (size_t)ch.first + (size_t)tid;
    const size_t p = (size_t)d.item_point[i];
    const double P[3] = { d.points[3 * p], d.points[3 * p + 1], d.points[3 * p + 2] };
    double Pn[3] = { 0.0, 0.0, 0.0 }, dmax = 0.0, dmin = 0.0;
    if (mode != MOVBA_VIEW_DEPTH) {
        Pn[0] = d.normals[3 * p]; Pn[1] = d.normals[3 * p + 1]; Pn[2] = d.normals[3 * p + 2];
        dmax = d.max_dist[p]; dmin = d.min_dist[p];
    }
    const VpItem r = vp_item(mode, meta[1], view, P, Pn, dmax, dmin);
    d.code[i] = r.code;
    d.code_dev[i] = r.code;
    if (d.z) d.z[i] = r.z;
    if (d.uv) { d.uv[2 * i] = r.u; d.uv[2 * i + 1] = r.v; }
    if (d.dist) d.dist[i] = r.dist;
    if (d.view_cos) d.view_cos[i] = r.view_cos;
    if (d.level) d.level[i] = r.level;
    if (d.ur) d.ur[i] = r.ur;
    if (d.track_depth) d.track_depth[i] = r.track_depth;
    if (mode == MOVBA_VIEW_DEPTH) d.keys[pv->key0 + (i - (size_t)pv->item0)] = im_order_key(r.z);
}

__global__ __launch_bounds__(kVpThreads) void k_vp_views(const VpDev d)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_rank;
    const int tid = threadIdx.x;
    const VpView *pv = d.views + blockIdx.x;
    const int32_t n = pv->n, mode = pv->mode;
    const double nan = __builtin_nan("");

    if (mode != MOVBA_VIEW_DEPTH) {
        // the accepted codes lie below the first reject
        const uint8_t *code = d.code_dev + pv->item0;
        unsigned mine = 0;
        for (int32_t i = tid; i < n; i += kVpThreads) mine += code[i] < MOVBA_VP_REJ_BEHIND;
        if (tid == 0) hist[0] = 0;
        __syncthreads();
        if (mine) atomicAdd(&hist[0], mine);
        __syncthreads();
        if (tid == 0) { d.n_accepted[blockIdx.x] = (int32_t)hist[0]; d.median[blockIdx.x] = nan; }
        return;
    }
    if (n == 0) {
        if (tid == 0) { d.n_accepted[blockIdx.x] = 0; d.median[blockIdx.x] = -1.0; }
        return;
    }

    const uint64_t *keys = d.keys + pv->key0;
    unsigned long long prefix = 0, mask = 0;
    unsigned rank = (unsigned)((n - 1) / pv->q);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;                                  // (256 threads, 256 bins)
        __syncthreads();
        for (int32_t i = tid; i < n; i += kVpThreads) {
            const unsigned long long k = keys[i];
            if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            // lane l holds bins 4 l .. 4 l + 3; an inclusive scan over the 64 lanes, then the one lane whose span holds the rank
            const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            unsigned incl = h0 + h1 + h2 + h3;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned up = __shfl_up(incl, off, 64);
                if (tid >= off) incl += up;
            }
            const unsigned excl = incl - (h0 + h1 + h2 + h3);
            if (rank >= excl && rank < incl) {
                unsigned r = rank - excl;
                int b = 0;
                if (r >= h0) { r -= h0; b = 1; if (r >= h1) { r -= h1; b = 2; if (r >= h2) { r -= h2; b = 3; } } }
                s_prefix = prefix | ((unsigned long long)(4 * tid + b) << shift);
                s_rank = r;
            }
        }
        __syncthreads();
        prefix = s_prefix; rank = s_rank;
        mask |= 0xffull << shift;
    }
    if (tid == 0) { d.n_accepted[blockIdx.x] = n; d.median[blockIdx.x] = vp_key_value(prefix); }
}

}  // namespace

hipError_t launch_view_points(const VpDev &d, hipStream_t s)
{
    if (d.n_chunks > 0) hipLaunchKernelGGL(k_vp_items, dim3(d.n_chunks), dim3(kVpThreads), 0, s, d);
    if (d.n_views > 0) hipLaunchKernelGGL(k_vp_views, dim3(d.n_views), dim3(kVpThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
