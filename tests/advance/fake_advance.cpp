// The fake device's side of movba_advance (mov-slam_amd/csrc/advance.cpp): the launch wrapper of advance.h as a closure on the
// fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the library's own steps (advance.h: adv_frames, serially,
// in the kernels' order), reading every input through the pointers the host laid out - checking every index on the way, so that
// an array the host packed wrongly is reported rather than followed - and writing results where the host said: the sanitizers
// see the host's layout and hand-offs, and the driver can check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "advance.h"
#include "movba.h"

namespace {
std::atomic<int> g_adv_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_advance: %s\n", what);
    g_adv_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_advance_errors() { return g_adv_errors.load(); }

namespace movba {

hipError_t launch_advance(const AdvDev &dev, hipStream_t s)
{
    const AdvDev d = dev;
    fake_enqueue(s, [=] {
        if (d.n_frames <= 0) return;
        if (!d.img_off || !d.rows || !d.cols || !d.threshold || !d.force_grid || !d.first_id || !d.prev_ptr || !d.mv_ptr || !d.kp_ptr || !d.g_ptr) { bad("a per-frame input is missing"); return; }
        if (!d.mov_cnt || !d.grid_ran || !d.next_id || !d.seg_ptr || !d.counts) { bad("a per-frame output is missing"); return; }
        if (d.prev_ptr[0] || d.mv_ptr[0] || d.kp_ptr[0] || d.g_ptr[0]) { bad("a pointer array does not start at 0"); return; }
        int64_t end = 0;
        int32_t max_prev = 0;
        for (int32_t f = 0; f < d.n_frames; ++f) {
            const int32_t np = d.prev_ptr[f + 1] - d.prev_ptr[f], nm = d.mv_ptr[f + 1] - d.mv_ptr[f], nk = d.kp_ptr[f + 1] - d.kp_ptr[f], ng = d.g_ptr[f + 1] - d.g_ptr[f];
            if (np < 0 || nm < 0 || nk < 0 || ng < 0 || np > MOVBA_MAX_ADVANCE_PREV) { bad("a pointer array descends, or a frame has too many features"); return; }
            if (d.rows[f] < 1 || d.cols[f] < 1 || d.threshold[f] < 0 || d.threshold[f] > 255 || d.first_id[f] < 0) { bad("a frame's record is out of range"); return; }
            if (ng != adv_lattice(d.rows[f], d.cols[f])) { bad("g_ptr is not the lattices' prefix"); return; }
            if (d.force_grid[f] != 0 && d.force_grid[f] != 1) { bad("force_grid is neither 0 nor 1"); return; }
            max_prev = np > max_prev ? np : max_prev;
            if (np + nk + ng == 0) continue;
            if (!d.pixels || d.img_off[f] != end) { bad("the frames that have items do not lie tightly, one behind the other"); return; }
            end += (int64_t)d.rows[f] * d.cols[f];
            for (int32_t g = d.prev_ptr[f]; g < d.prev_ptr[f + 1]; ++g)
                for (int c = 0; c < 4; ++c)
                    if (d.prev_cand[4 * (size_t)g + c] < -1 || d.prev_cand[4 * (size_t)g + c] >= nm) { bad("a candidate is no vector of its frame"); return; }
            for (int32_t m = d.mv_ptr[f]; m < d.mv_ptr[f + 1]; ++m)
                if (d.mv_dindx[m] < -1 || d.mv_dindx[m] >= nk) { bad("a dindx is no macroblock of its frame"); return; }
        }
        if (adv_item_base(d, d.n_frames) != d.n_items || max_prev != d.max_prev) { bad("the counts do not match the pointer arrays"); return; }
        for (int32_t m = 0; m < d.kp_ptr[d.n_frames]; ++m)
            if (d.claim[m] != kAdvNoClaim) { bad("a claim word does not arrive filled"); return; }
        adv_frames(d);
    });
    return hipSuccess;
}

}  // namespace movba
