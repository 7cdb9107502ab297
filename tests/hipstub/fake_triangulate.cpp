// The fake device's side of movba_triangulate (mov-slam_amd/csrc/triangulate.cpp): the launch wrapper of triangulate.h as a
// closure on the fake stream (fake_hip.cpp).  It runs the library's own per-match arithmetic (triangulate_math.h: plain C++,
// the code the kernel inlines) match by match on the CPU, reading every input array through the pointers the host laid out
// and writing points and codes where the host said, so the sanitizers see the host's layout and hand-offs and a driver can
// check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "triangulate.h"
#include "triangulate_math.h"

namespace {
std::atomic<int> g_tri_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_triangulate: %s\n", what);
    g_tri_errors.fetch_add(1);
}
}  // namespace

// layout errors the fake device saw (the driver fails on any)
extern "C" int fake_triangulate_errors() { return g_tri_errors.load(); }

namespace movba {

hipError_t launch_triangulate(const TriDev &dev, hipStream_t s)
{
    const TriDev d = dev;
    fake_enqueue(s, [=] {
        if (d.pair_ptr[0] != 0 || d.pair_ptr[d.n_pairs] != d.n_matches) { bad("pair_ptr does not span the matches"); return; }
        for (int p = 0; p < d.n_pairs; ++p) {
            if (d.pair_ptr[p + 1] < d.pair_ptr[p]) { bad("pair_ptr not ascending"); return; }
            double v1[kTriViewDoubles], v2[kTriViewDoubles];
            const int a = d.pair_view[2 * p], b = d.pair_view[2 * p + 1];
            tri_view(d.poses + 7 * (size_t)a, d.cam + 4 * (size_t)a, d.bf ? d.bf[a] : 0.0, d.b ? d.b[a] : 0.0, v1);
            tri_view(d.poses + 7 * (size_t)b, d.cam + 4 * (size_t)b, d.bf ? d.bf[b] : 0.0, d.b ? d.b[b] : 0.0, v2);
            for (int m = d.pair_ptr[p]; m < d.pair_ptr[p + 1]; ++m) {
                double X[3];
                d.code[m] = tri_match(v1, v2, d.obs1[2 * m], d.obs1[2 * m + 1], d.obs2[2 * m], d.obs2[2 * m + 1],
                                      d.ur1 ? d.ur1[m] : -1.0, d.ur1 ? d.depth1[m] : 0.0, d.ur2 ? d.ur2[m] : -1.0,
                                      d.ur2 ? d.depth2[m] : 0.0, d.gate, d.far_th, X);
                d.points[3 * (size_t)m] = X[0]; d.points[3 * (size_t)m + 1] = X[1]; d.points[3 * (size_t)m + 2] = X[2];
            }
        }
    });
    return hipSuccess;
}

}  // namespace movba
