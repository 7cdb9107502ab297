// The fake device's side of movba_track_match (mov-slam_amd/csrc/track_match.cpp): the launch wrapper of track_match.h as a
// closure on the fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the library's own steps (track_match.h:
// tm_query query by query, then tm_pack, serially, in the kernels' order), reading every input through the pointers the host laid
// out - checking every index on the way, so that an array the host packed wrongly is reported rather than followed - and writing
// results where the host said: the sanitizers see the host's layout and hand-offs, and the driver can check the values that come
// back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <vector>

#include "movba.h"
#include "track_match.h"

namespace {
std::atomic<int> g_tm_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_track_match: %s\n", what);
    g_tm_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_track_match_errors() { return g_tm_errors.load(); }

namespace movba {

hipError_t launch_track_match(const TmDev &dev, int32_t max_slots, hipStream_t s)
{
    const TmDev d = dev;
    fake_enqueue(s, [=] {
        if (d.n_queries <= 0) return;
        if (max_slots < 0 || max_slots > MOVBA_MAX_TRACK_SLOTS) { bad("more slots than a workgroup's LDS holds"); return; }
        if (d.query_ptr[0] != 0 || d.row_base[0] != 0) { bad("a prefix does not start at 0"); return; }
        for (int32_t q = 0; q < d.n_queries; ++q) {
            const int32_t mode = d.query_mode[q], v1 = d.query_view[2 * q], v2 = d.query_view[2 * q + 1];
            if (d.query_ptr[q + 1] < d.query_ptr[q]) { bad("the queries' prefix descends"); return; }
            if (v2 < 0 || d.view_ptr[v2 + 1] < d.view_ptr[v2] || d.view_ptr[v2] < 0) { bad("a searched view is no view"); return; }
            if (d.view_ptr[v2 + 1] - d.view_ptr[v2] > max_slots) { bad("a searched view is larger than the launch was told"); return; }
            if (mode == MOVBA_TM_TRIANGULATION) {
                if (v1 < 0 || d.view_ptr[v1 + 1] < d.view_ptr[v1]) { bad("view 1 is no view"); return; }
                if (d.row_base[q + 1] - d.row_base[q] != d.view_ptr[v1 + 1] - d.view_ptr[v1]) { bad("a row is not as long as view 1"); return; }
            } else if (mode == MOVBA_TM_LOOKUP) {
                if (d.row_base[q + 1] != d.row_base[q]) { bad("a lookup with a row"); return; }
                if (d.query_ptr[q + 1] > d.query_ptr[q] && (!d.item_track || !d.item_slot)) { bad("items without arrays"); return; }
            } else { bad("an unknown mode"); return; }
        }
        if (d.row_base[d.n_queries] != d.match_cap) { bad("the rows do not add up to match_cap"); return; }
        if (d.match_cap > 0 && (!d.match_slot1 || !d.match_slot2)) { bad("matches without arrays"); return; }
        if (((d.obs1 || d.obs2) && !d.slot_obs) || ((d.ur1 || d.ur2) && !d.slot_ur) || ((d.depth1 || d.depth2) && !d.slot_depth)) { bad("a gather without its source"); return; }
        // (exactly as long as it must be for each query: the sanitizer sees an index one past the end)
        for (int32_t q = 0; q < d.n_queries; ++q) {
            const int32_t v2 = d.query_view[2 * q + 1];
            std::vector<int32_t> table((size_t)tm_table_entries(d.view_ptr[v2 + 1] - d.view_ptr[v2]));
            tm_query(d, q, table.data());
        }
        tm_pack(d);
    });
    return hipSuccess;
}

}  // namespace movba
