// movba_track_match's steps on the CPU: tm_query and tm_pack of mov-slam_amd/csrc/track_match.h - the table with its hash, its
// probe order and its rule for the lowest slot, the order of a query's matches, the dense prefix, the gather and the padding, the
// functions k_tm_match and k_tm_pack call from their lanes - query by query, and every TRIANGULATION query against the double
// loop as the reference writes it.  Built stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (no library source is
// linked); tests/test_track_match_cpu.py writes the call to a file, runs this and compares with the restatement.
//   tm_main <in> <out>
//   in:  int32 n_views n_queries n_slots n_items has_taken has_obs has_ur has_depth; int32 view_ptr[nv + 1] slot_track[n_slots]
//        query_mode[nq] query_view[2 nq] query_ptr[nq + 1] item_track[n_items]; if has_taken: uint8 slot_taken[n_slots]; 64-bit
//        words: if has_obs slot_obs[2 n_slots], if has_ur slot_ur[n_slots], if has_depth slot_depth[n_slots]
//   out: int32 match_cap pair_ptr[nq + 1] match_slot1[cap] match_slot2[cap] item_slot[n_items] n_found[nq]; 64-bit words: if
//        has_obs obs1[2 cap] obs2[2 cap], if has_ur ur1[cap] ur2[cap], if has_depth depth1[cap] depth2[cap]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "track_match.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "tm_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "tm_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: tm_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 8);
    const size_t nv = (size_t)hd[0], nq = (size_t)hd[1], ns = (size_t)hd[2], n_items = (size_t)hd[3];
    const auto view_ptr = rd<int32_t>(f, nv + 1), slot_track = rd<int32_t>(f, ns), query_mode = rd<int32_t>(f, nq), query_view = rd<int32_t>(f, 2 * nq);
    const auto query_ptr = rd<int32_t>(f, nq + 1), item_track = rd<int32_t>(f, n_items);
    const auto slot_taken = rd<uint8_t>(f, hd[4] ? ns : 0);
    const auto slot_obs = rd<uint64_t>(f, hd[5] ? 2 * ns : 0), slot_ur = rd<uint64_t>(f, hd[6] ? ns : 0), slot_depth = rd<uint64_t>(f, hd[7] ? ns : 0);
    std::fclose(f);

    std::vector<int32_t> row_base(nq + 1, 0);
    for (size_t q = 0; q < nq; ++q) {
        const int32_t v1 = query_view[2 * q];
        row_base[q + 1] = row_base[q] + (query_mode[q] == MOVBA_TM_TRIANGULATION ? view_ptr[v1 + 1] - view_ptr[v1] : 0);
    }
    const size_t cap = (size_t)row_base[nq];
    // (exactly as long as they must be: the sanitizer sees an index one past the end)
    std::vector<int32_t> row1(cap), row2(cap), count(nq), pair_ptr(nq + 1), slot1(cap), slot2(cap), item_slot(n_items), n_found(nq);
    std::vector<uint64_t> obs1(hd[5] ? 2 * cap : 0), obs2(obs1.size()), ur1(hd[6] ? cap : 0), ur2(ur1.size()), depth1(hd[7] ? cap : 0), depth2(depth1.size());
    TmDev d{};
    d.n_queries = hd[1]; d.match_cap = (int32_t)cap;
    d.view_ptr = view_ptr.data(); d.slot_track = slot_track.data(); d.slot_taken = hd[4] ? slot_taken.data() : nullptr;
    d.slot_obs = hd[5] ? slot_obs.data() : nullptr; d.slot_ur = hd[6] ? slot_ur.data() : nullptr; d.slot_depth = hd[7] ? slot_depth.data() : nullptr;
    d.query_mode = query_mode.data(); d.query_view = query_view.data(); d.query_ptr = query_ptr.data(); d.item_track = item_track.data();
    d.row_base = row_base.data(); d.row_slot1 = row1.data(); d.row_slot2 = row2.data(); d.count = count.data();
    d.pair_ptr = pair_ptr.data(); d.match_slot1 = slot1.data(); d.match_slot2 = slot2.data(); d.item_slot = item_slot.data(); d.n_found = n_found.data();
    d.obs1 = hd[5] ? obs1.data() : nullptr; d.obs2 = hd[5] ? obs2.data() : nullptr; d.ur1 = hd[6] ? ur1.data() : nullptr; d.ur2 = hd[6] ? ur2.data() : nullptr;
    d.depth1 = hd[7] ? depth1.data() : nullptr; d.depth2 = hd[7] ? depth2.data() : nullptr;

    for (size_t q = 0; q < nq; ++q) {
        const int32_t v1 = query_view[2 * q], v2 = query_view[2 * q + 1];
        std::vector<int32_t> table((size_t)tm_table_entries(view_ptr[v2 + 1] - view_ptr[v2]));
        tm_query(d, (int32_t)q, table.data());
        if (query_mode[q] != MOVBA_TM_TRIANGULATION) continue;
        // the table's answer is the double loop's answer
        const int32_t b1 = view_ptr[v1], n1 = view_ptr[v1 + 1] - b1, b2 = view_ptr[v2], n2 = view_ptr[v2 + 1] - b2;
        int32_t n = 0;
        bool same = true;
        for (int32_t i = 0; i < n1; ++i) {
            if (hd[4] && slot_taken[b1 + i]) continue;
            for (int32_t j = 0; j < n2; ++j) {
                if (hd[4] && slot_taken[b2 + j]) continue;
                if (slot_track[b1 + i] == slot_track[b2 + j]) {
                    same &= n < count[q] && row1[row_base[q] + n] == i && row2[row_base[q] + n] == j;
                    ++n;
                    break;
                }
            }
        }
        if (!same || n != count[q]) { std::fprintf(stderr, "tm_main: query %zu: the table's matches are not the double loop's\n", q); return 1; }
    }
    tm_pack(d);

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, std::vector<int32_t>(1, (int32_t)cap));
    wr(o, pair_ptr); wr(o, slot1); wr(o, slot2); wr(o, item_slot); wr(o, n_found);
    wr(o, obs1); wr(o, obs2); wr(o, ur1); wr(o, ur2); wr(o, depth1); wr(o, depth2);
    std::fclose(o);
    std::printf("tm_main: ok\n");
    return 0;
}
