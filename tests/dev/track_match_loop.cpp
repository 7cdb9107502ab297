// The joins movba_track_match replaces, as a caller without it writes them, on one thread, twice: the double loop over the slots
// of two keyframes as the reference writes it (MOVMatcher.h:139-168; LOOKUP: the ascending scan with `break` of Fuse, :249-273),
// and a join through one std::unordered_map per searched view, filled in slot order, the first insertion kept.  Both go on to
// gather the matched slots' payload into the arrays movba_triangulate takes, as the call does - over index arrays, which spares
// them the reference's copies of GetMapPointMatches() and of a VideoFeature per comparison: a lower bound of the caller's cost.
// Built and run by tests/dev/track_match_time.py; prints the median and minimum time of `reps` passes over all queries for each
// and a checksum of the results (the tool compares it with the device's).
//   track_match_loop <in> <reps>      in: the format of tests/track_match/tm_main.cpp
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

template <typename T> static std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "track_match_loop: short input\n"); std::exit(2); }
    return a;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: track_match_loop <in> <reps>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int reps = std::atoi(argv[2]);
    const std::vector<int32_t> hd = rd<int32_t>(f, 8);
    const size_t nv = (size_t)hd[0], nq = (size_t)hd[1], ns = (size_t)hd[2], n_items = (size_t)hd[3];
    const auto view_ptr = rd<int32_t>(f, nv + 1), track = rd<int32_t>(f, ns), mode = rd<int32_t>(f, nq), qview = rd<int32_t>(f, 2 * nq);
    const auto query_ptr = rd<int32_t>(f, nq + 1), items = rd<int32_t>(f, n_items);
    const auto taken = rd<uint8_t>(f, hd[4] ? ns : 0);
    const auto obs = rd<uint64_t>(f, hd[5] ? 2 * ns : 0), ur = rd<uint64_t>(f, hd[6] ? ns : 0), depth = rd<uint64_t>(f, hd[7] ? ns : 0);
    std::fclose(f);
    size_t cap = 0;
    for (size_t q = 0; q < nq; ++q)
        if (mode[q] == 0) cap += (size_t)(view_ptr[qview[2 * q] + 1] - view_ptr[qview[2 * q]]);
    std::vector<int32_t> slot1(cap), slot2(cap), item_slot(n_items);
    std::vector<uint64_t> obs1(hd[5] ? 2 * cap : 0), obs2(obs1.size()), ur1(hd[6] ? cap : 0), ur2(ur1.size()), depth1(hd[7] ? cap : 0), depth2(depth1.size());
    auto is_free = [&](int32_t g) { return !hd[4] || !taken[(size_t)g]; };

    double med[2], low[2];
    uint64_t checksum[2];
    for (int method = 0; method < 2; ++method) {
        std::vector<double> ms;
        for (int rep = 0; rep < reps; ++rep) {
            const auto t0 = std::chrono::steady_clock::now();
            size_t at = 0;
            auto match = [&](int32_t b1, int32_t i, int32_t b2, int32_t j) {
                slot1[at] = i; slot2[at] = j;
                const size_t g1 = (size_t)(b1 + i), g2 = (size_t)(b2 + j);
                if (hd[5]) { obs1[2 * at] = obs[2 * g1]; obs1[2 * at + 1] = obs[2 * g1 + 1]; obs2[2 * at] = obs[2 * g2]; obs2[2 * at + 1] = obs[2 * g2 + 1]; }
                if (hd[6]) { ur1[at] = ur[g1]; ur2[at] = ur[g2]; }
                if (hd[7]) { depth1[at] = depth[g1]; depth2[at] = depth[g2]; }
                ++at;
            };
            for (size_t q = 0; q < nq; ++q) {
                const int32_t v1 = qview[2 * q], v2 = qview[2 * q + 1], b2 = view_ptr[v2], n2 = view_ptr[v2 + 1] - b2;
                const bool lookup = mode[q] == 1;
                if (method == 0) {
                    if (lookup) {
                        for (int32_t i = query_ptr[q]; i < query_ptr[q + 1]; ++i) {
                            item_slot[i] = -1;
                            for (int32_t j = 0; j < n2; ++j)
                                if (track[b2 + j] == items[i]) { item_slot[i] = j; break; }
                        }
                        continue;
                    }
                    const int32_t b1 = view_ptr[v1], n1 = view_ptr[v1 + 1] - b1;
                    for (int32_t i = 0; i < n1; ++i) {
                        if (!is_free(b1 + i)) continue;
                        for (int32_t j = 0; j < n2; ++j) {
                            if (!is_free(b2 + j)) continue;
                            if (track[b1 + i] == track[b2 + j]) { match(b1, i, b2, j); break; }
                        }
                    }
                } else {
                    std::unordered_map<int32_t, int32_t> first;
                    first.reserve((size_t)n2);
                    for (int32_t j = 0; j < n2; ++j)
                        if (lookup || is_free(b2 + j)) first.insert({ track[b2 + j], j });
                    if (lookup) {
                        for (int32_t i = query_ptr[q]; i < query_ptr[q + 1]; ++i) {
                            const auto it = first.find(items[i]);
                            item_slot[i] = it == first.end() ? -1 : it->second;
                        }
                        continue;
                    }
                    const int32_t b1 = view_ptr[v1], n1 = view_ptr[v1 + 1] - b1;
                    for (int32_t i = 0; i < n1; ++i) {
                        if (!is_free(b1 + i)) continue;
                        const auto it = first.find(track[b1 + i]);
                        if (it != first.end()) match(b1, i, b2, it->second);
                    }
                }
            }
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            // (what the device's match_slot1, match_slot2, item_slot and the first payload word of each match add up to)
            uint64_t sum = at;
            for (size_t k = 0; k < at; ++k) sum += (uint64_t)(slot1[k] + 1) + 3 * (uint64_t)(slot2[k] + 1) + (hd[5] ? obs2[2 * k] >> 40 : 0);
            for (size_t i = 0; i < n_items; ++i) sum += 5 * (uint64_t)(item_slot[i] + 2);
            checksum[method] = sum;
        }
        std::sort(ms.begin(), ms.end());
        med[method] = ms[ms.size() / 2]; low[method] = ms[0];
    }
    std::printf("{\"double_loop\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"checksum\": %llu}, \"unordered_map\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"checksum\": %llu}}\n",
                med[0], low[0], (unsigned long long)checksum[0], med[1], low[1], (unsigned long long)checksum[1]);
    return 0;
}
