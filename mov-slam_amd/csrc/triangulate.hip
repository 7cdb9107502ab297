// k_triangulate: movba_triangulate's one kernel (include/movba.h).  One thread per match, 256 per workgroup; the arithmetic of
// a match is triangulate_math.h.  A thread finds its pair by binary search over pair_ptr (as k_pose_hyp_b finds its frame).
// The two views of a pair - rotation from the quaternion, translation, camera centre, camera, bf, b: 21 doubles each - are
// the same for every match of the pair, and a workgroup's 256 consecutive matches almost always lie in one or two pairs: the
// views are computed once per workgroup into LDS, kTriPairCache pairs at a time (a workgroup that spans more pairs - many
// tiny or empty ones - goes round again), and every lane reads them from there (same address in every lane of a pair: a
// broadcast).  No atomics, no reductions: a match's result is written by its own thread and depends on nothing else.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "triangulate.h"
#include "triangulate_math.h"

namespace movba {

namespace {

__global__ __launch_bounds__(kTriThreads) void k_triangulate(const TriDev d)
{
    __shared__ double views[kTriPairCache * 2 * kTriViewDoubles];
    const int tid = threadIdx.x;
    const int n = d.n_matches;
    const int m0 = blockIdx.x * kTriThreads;            // (the grid covers [0, n): m0 < n)
    const int m = m0 + tid;
    const bool live = m < n;
    const int m_last = min(m0 + kTriThreads - 1, n - 1);
    const int p_lo = prefix_find(d.pair_ptr, d.n_pairs, m0), p_hi = prefix_find(d.pair_ptr, d.n_pairs, m_last);
    const int p = live ? prefix_find(d.pair_ptr, d.n_pairs, m) : -1;

    double u1 = 0.0, w1 = 0.0, u2 = 0.0, w2 = 0.0, ur1 = -1.0, ur2 = -1.0, d1 = 0.0, d2 = 0.0;
    if (live) {
        const double2 o1 = reinterpret_cast<const double2 *>(d.obs1)[m], o2 = reinterpret_cast<const double2 *>(d.obs2)[m];
        u1 = o1.x; w1 = o1.y; u2 = o2.x; w2 = o2.y;
        if (d.ur1) { ur1 = d.ur1[m]; d1 = d.depth1[m]; }
        if (d.ur2) { ur2 = d.ur2[m]; d2 = d.depth2[m]; }
    }

    for (int base = p_lo; base <= p_hi; base += kTriPairCache) {
        __syncthreads();                                // (the round before has read its views)
        if (tid < 2 * kTriPairCache) {
            const int q = base + (tid >> 1);
            if (q <= p_hi && d.pair_ptr[q] < d.pair_ptr[q + 1]) {
                const int v = d.pair_view[2 * q + (tid & 1)];
                tri_view(d.poses + 7 * (size_t)v, d.cam + 4 * (size_t)v, d.bf ? d.bf[v] : 0.0, d.b ? d.b[v] : 0.0,
                         views + tid * kTriViewDoubles);
            }
        }
        __syncthreads();
        if (live && p >= base && p < base + kTriPairCache) {
            const double *v1 = views + (p - base) * 2 * kTriViewDoubles, *v2 = v1 + kTriViewDoubles;
            double X[3];
            const uint8_t code = tri_match(v1, v2, u1, w1, u2, w2, ur1, d1, ur2, d2, d.gate, d.far_th, X);
            double *out = d.points + 3 * (size_t)m;
            out[0] = X[0]; out[1] = X[1]; out[2] = X[2];
            d.code[m] = code;
        }
    }
}

}  // namespace

hipError_t launch_triangulate(const TriDev &d, hipStream_t s)
{
    if (d.n_matches <= 0) return hipGetLastError();
    const int blocks = (d.n_matches + kTriThreads - 1) / kTriThreads;
    hipLaunchKernelGGL(k_triangulate, dim3(blocks), dim3(kTriThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
