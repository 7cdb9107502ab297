// The fake device's side of movba_covisibility (mov-slam_amd/csrc/covisibility.cpp): the launch wrapper of covisibility.h as a
// closure on the fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the library's own per-query steps
// (covisibility.h: cv_query, serially, in the kernel's order) query by query, reading every input through the pointers the host
// laid out - checking every index on the way, so that an array the host packed wrongly is reported rather than followed - and
// writing results where the host said: the sanitizers see the host's layout and hand-offs, and the driver can check the values
// that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <vector>

#include "covisibility.h"
#include "movba.h"

namespace {
std::atomic<int> g_cv_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_covisibility: %s\n", what);
    g_cv_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_covisibility_errors() { return g_cv_errors.load(); }

namespace movba {

hipError_t launch_covisibility(const CvDev &dev, hipStream_t s)
{
    const CvDev d = dev;
    fake_enqueue(s, [=] {
        if (d.n_queries <= 0) return;
        if (d.n_views < 0 || d.n_views > MOVBA_MAX_COVIS_VIEWS) { bad("more views than a workgroup's LDS holds"); return; }
        if (d.query_ptr[0] != 0) { bad("the queries do not start at 0"); return; }
        for (int32_t q = 0; q < d.n_queries; ++q) {
            if (d.query_ptr[q + 1] < d.query_ptr[q]) { bad("the queries' prefix descends"); return; }
            if (d.query_self && (d.query_self[q] < -1 || d.query_self[q] >= d.n_views)) { bad("a self entry out of range"); return; }
            for (int32_t i = d.query_ptr[q]; i < d.query_ptr[q + 1]; ++i) {
                if (!d.obs_ptr) { bad("an item without lists"); return; }
                const int32_t p = d.query_point[i];
                if (p < 0 || d.obs_ptr[p + 1] < d.obs_ptr[p] || d.obs_ptr[p] < 0) { bad("an item's list is no list"); return; }
                for (int32_t k = d.obs_ptr[p]; k < d.obs_ptr[p + 1]; ++k)
                    if (d.obs_view[k] < 0 || d.obs_view[k] >= d.n_views) { bad("an observer out of range"); return; }
            }
        }
        if (d.max_out > 0 && (!d.out_view || !d.out_weight)) { bad("a hand-out without arrays"); return; }
        // (exactly as long as they must be: the sanitizer sees an index one past the end)
        std::vector<int32_t> counters((size_t)d.n_views);
        std::vector<uint64_t> keys((size_t)cv_pow2ceil(d.n_views));
        for (int32_t q = 0; q < d.n_queries; ++q)
            cv_query(d, q, counters.data(), keys.data());
    });
    return hipSuccess;
}

}  // namespace movba
