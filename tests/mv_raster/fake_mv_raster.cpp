// The fake device's side of movba_mv_raster (mov-slam_amd/csrc/mv_raster.cpp): the launch wrapper of mv_raster.h as a closure on
// the fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the library's own steps (mv_raster.h: mvr_frames,
// serially, in the kernels' order), reading every input through the pointers the host laid out - checking the layout on the
// way, so that an array the host packed wrongly is reported rather than followed - and writing results where the host said: the
// sanitizers see the host's layout and hand-offs, and the driver can check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>

#include "movba.h"
#include "mv_raster.h"

namespace {
std::atomic<int> g_mvr_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_mv_raster: %s\n", what);
    g_mvr_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_mv_raster_errors() { return g_mvr_errors.load(); }

namespace movba {

hipError_t launch_mv_raster(const MvrDev &dev, hipStream_t s)
{
    const MvrDev d = dev;
    fake_enqueue(s, [=] {
        if (d.n_frames <= 0) return;
        if (!d.rows || !d.cols || !d.rec_ptr || !d.q_ptr || !d.g_ptr || !d.tile_ptr || !d.threshold || !d.want_grid) { bad("a per-frame input is missing"); return; }
        if (!d.kept_ptr || !d.grid_ptr || !d.cover_px || !d.coverage_area || !d.force_grid || !d.kept_cnt || !d.cover || !d.kept_base || !d.tile_off) { bad("a per-frame output is missing"); return; }
        if (d.tile_off != d.cover + d.n_frames || !d.chunk_cnt) { bad("cover and tile_off are not one block, or the chunk counts are missing"); return; }
        int32_t max_records = 0;
        if (d.rec_ptr[0] || d.q_ptr[0] || d.g_ptr[0] || d.tile_ptr[0]) { bad("a pointer array does not start at 0"); return; }
        for (int32_t f = 0; f < d.n_frames; ++f) {
            const int32_t nr = d.rec_ptr[f + 1] - d.rec_ptr[f], nq = d.q_ptr[f + 1] - d.q_ptr[f];
            if (nr < 0 || nq < 0 || nr > kMvrMaxFrameRecords) { bad("a pointer array descends, or a frame has too many records"); return; }
            max_records = nr > max_records ? nr : max_records;
            if (d.rows[f] < 1 || d.cols[f] < 1 || d.rows[f] > 32767 || d.cols[f] > 32767) { bad("a frame's size is out of range"); return; }
            if (d.g_ptr[f + 1] - d.g_ptr[f] != adv_lattice(d.rows[f], d.cols[f])) { bad("g_ptr is not the lattices' prefix"); return; }
            if (d.tile_ptr[f + 1] - d.tile_ptr[f] != mvr_tiles(d.rows[f], d.cols[f])) { bad("tile_ptr is not the tiles' prefix"); return; }
        }
        if (d.rec_ptr[d.n_frames] != d.n_records || d.q_ptr[d.n_frames] != d.n_q || d.g_ptr[d.n_frames] != d.n_grid || d.tile_ptr[d.n_frames] != d.n_tiles || max_records != d.max_records) {
            bad("the counts do not match the pointer arrays");
            return;
        }
        for (int32_t i = 0; i < d.n_records; ++i)
            if (!mvr_size_ok(d.w[i]) || !mvr_size_ok(d.h[i])) { bad("a block size is none of 4, 8, 16"); return; }
        std::memset(d.cover, 0, sizeof(int32_t) * ((size_t)d.n_frames + (size_t)d.n_tiles + 1));
        mvr_frames(d);
    });
    return hipSuccess;
}

}  // namespace movba
