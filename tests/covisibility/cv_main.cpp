// movba_covisibility's per-query steps on the CPU: cv_query of mov-slam_amd/csrc/covisibility.h - the count, the compaction, the
// bitonic network pair by pair, best, connected and the hand-out, the functions k_covis calls from its lanes - query by query,
// and the network's order against std::sort.  Built stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (no library
// source is linked); tests/test_covisibility_cpu.py writes the call to a file, runs this and compares with the restatement.
//   cv_main <in> <out>
//   in:  int32 n_views n_points n_queries min_weight max_out n_obs n_items has_self has_eligible; int32 obs_ptr[np + 1]
//        obs_view[n_obs] query_ptr[nq + 1] query_point[n_items]; if has_self: int32 query_self[nq]; if has_eligible: uint8
//        eligible[n_views]
//   out: int32 n_counted[nq] n_connected[nq] best_view[nq] best_weight[nq] out_view[nq max_out] out_weight[nq max_out]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "covisibility.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "cv_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "cv_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: cv_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 9);
    const size_t nv = (size_t)hd[0], np = (size_t)hd[1], nq = (size_t)hd[2], max_out = (size_t)hd[4], n_obs = (size_t)hd[5], n_items = (size_t)hd[6];
    const auto obs_ptr = rd<int32_t>(f, np + 1), obs_view = rd<int32_t>(f, n_obs), query_ptr = rd<int32_t>(f, nq + 1), query_point = rd<int32_t>(f, n_items);
    const auto query_self = rd<int32_t>(f, hd[7] ? nq : 0);
    const auto eligible = rd<uint8_t>(f, hd[8] ? nv : 0);
    std::fclose(f);

    // (exactly as long as they must be: the sanitizer sees an index one past the end)
    std::vector<int32_t> n_counted(nq), n_connected(nq), best_view(nq), best_weight(nq), out_view(nq * max_out), out_weight(nq * max_out);
    std::vector<int32_t> counters(nv);
    std::vector<uint64_t> keys((size_t)cv_pow2ceil((int32_t)nv));
    CvDev d{};
    d.n_views = hd[0]; d.n_queries = hd[2]; d.min_weight = hd[3]; d.max_out = hd[4];
    d.obs_ptr = obs_ptr.data(); d.obs_view = obs_view.data(); d.query_ptr = query_ptr.data(); d.query_point = query_point.data();
    d.query_self = hd[7] ? query_self.data() : nullptr; d.eligible = hd[8] ? eligible.data() : nullptr;
    d.n_counted = n_counted.data(); d.n_connected = n_connected.data(); d.best_view = best_view.data(); d.best_weight = best_weight.data();
    d.out_view = out_view.data(); d.out_weight = out_weight.data();
    for (size_t q = 0; q < nq; ++q) {
        cv_query(d, (int32_t)q, counters.data(), keys.data());
        // the network's order is the order: the same keys through std::sort
        std::vector<uint64_t> again;
        const int32_t self = d.query_self ? d.query_self[q] : -1;
        for (int32_t v = 0; v < d.n_views; ++v) {
            const int32_t w = cv_weight(counters.data(), v, d.eligible, self);
            if (w > 0) again.push_back(cv_key(w, v));
        }
        std::sort(again.begin(), again.end(), std::greater<uint64_t>());
        if ((size_t)n_counted[q] != again.size() || !std::equal(again.begin(), again.end(), keys.begin())) {
            std::fprintf(stderr, "cv_main: query %zu: the network's order is not the sorted order\n", q);
            return 1;
        }
    }

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, n_counted); wr(o, n_connected); wr(o, best_view); wr(o, best_weight); wr(o, out_view); wr(o, out_weight);
    std::fclose(o);
    std::printf("cv_main: ok\n");
    return 0;
}
