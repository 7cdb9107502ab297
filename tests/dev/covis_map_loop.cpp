// The loop movba_covisibility replaces, as a caller without it writes it: one thread, one std::map<int, int> per query, the
// threshold and maximum pass and the sort of KeyFrame::UpdateConnections - over index arrays, which spares it the reference's
// pointer chasing through MapPoint::GetObservations (a copy of a std::map per point): a lower bound of the caller's cost.
// Built and run by tests/dev/covis_time.py; prints the median and minimum time of `reps` passes over all queries and a checksum
// of the results (the tool compares it with the device's).
//   covis_map_loop <in> <reps>      in: the format of tests/covisibility/cv_main.cpp
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

template <typename T> static std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "covis_map_loop: short input\n"); std::exit(2); }
    return a;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: covis_map_loop <in> <reps>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int reps = std::atoi(argv[2]);
    const std::vector<int32_t> hd = rd<int32_t>(f, 9);
    const size_t nv = (size_t)hd[0], np = (size_t)hd[1], nq = (size_t)hd[2];
    const int32_t th = hd[3];
    const auto obs_ptr = rd<int32_t>(f, np + 1), obs_view = rd<int32_t>(f, (size_t)hd[5]), query_ptr = rd<int32_t>(f, nq + 1), query_point = rd<int32_t>(f, (size_t)hd[6]);
    const auto query_self = rd<int32_t>(f, hd[7] ? nq : 0);
    const auto eligible = rd<uint8_t>(f, hd[8] ? nv : 0);
    std::fclose(f);

    std::vector<double> ms;
    uint64_t checksum = 0;
    for (int rep = 0; rep < reps; ++rep) {
        checksum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t q = 0; q < nq; ++q) {
            std::map<int32_t, int> counter;
            const int32_t self = hd[7] ? query_self[q] : -1;
            for (int32_t i = query_ptr[q]; i < query_ptr[q + 1]; ++i) {
                const int32_t p = query_point[i];
                for (int32_t k = obs_ptr[p]; k < obs_ptr[p + 1]; ++k) {
                    const int32_t v = obs_view[k];
                    if (v == self || (hd[8] && !eligible[v])) continue;
                    counter[v]++;
                }
            }
            int nmax = 0, vmax = -1;
            std::vector<std::pair<int, int32_t>> pairs;
            pairs.reserve(counter.size());
            for (const auto &kv : counter) {
                if (kv.second > nmax) { nmax = kv.second; vmax = kv.first; }
                if (kv.second >= th) pairs.push_back({ kv.second, kv.first });
            }
            if (pairs.empty() && vmax >= 0) pairs.push_back({ nmax, vmax });
            std::sort(pairs.begin(), pairs.end());
            // (what the device's n_counted, n_connected, best_view, best_weight and the connected front of its order add up to)
            checksum += counter.size() + 3 * pairs.size() + 5 * (uint64_t)(vmax + 1) + 7 * (uint64_t)nmax;
            for (size_t k = 0; k < pairs.size(); ++k) checksum += (uint64_t)(pairs.size() - k) * (uint64_t)(pairs[k].second + 1);
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("{\"median_ms\": %.6f, \"min_ms\": %.6f, \"checksum\": %llu}\n", ms[ms.size() / 2], ms[0], (unsigned long long)checksum);
    return 0;
}
