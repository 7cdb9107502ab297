// movba_mv_raster's steps on the CPU: mvr_frames of mov-slam_amd/csrc/mv_raster.h - the keep test, the rect and the extent with
// their clamps, the tiles' lists, the slots of a pixel, the coverage, the functions the kernels call - over one call, serially.
// Every array is exactly as long as the kernels', so an index past an end is seen.  Built stand-alone under AddressSanitizer +
// UndefinedBehaviorSanitizer (no library source is linked); the test writes the call to a file, runs this and compares with the
// restatement.
//   mvr_main <in> <out>
//   in:  int32 n_frames n_records n_q; int32 rows[nf] cols[nf]; double threshold[nf]; uint8 want_grid[nf]; int32 rec_ptr[nf + 1]
//        q_ptr[nf + 1]; int16 src_x[nr] src_y[nr] dst_x[nr] dst_y[nr]; uint8 w[nr] h[nr]; float q_pt[2 nq]
//   out: int32 kept_ptr[nf + 1] kp_rect[4 nr]; float mv_pt[2 nr]; int32 mv_dindx[nr] rec_kept[nr] cand[4 nq] grid_ptr[nf + 1];
//        uint8 grid_covered[ng]; int32 cover_px[nf]; double coverage_area[nf]; uint8 force_grid[nf]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mv_raster.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "mvr_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "mvr_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: mvr_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 3);
    const size_t nf = (size_t)hd[0], nr = (size_t)hd[1], nq = (size_t)hd[2];
    const auto rows = rd<int32_t>(f, nf), cols = rd<int32_t>(f, nf);
    const auto threshold = rd<double>(f, nf);
    const auto want = rd<uint8_t>(f, nf);
    const auto rec_ptr = rd<int32_t>(f, nf + 1), q_ptr = rd<int32_t>(f, nf + 1);
    const auto sx = rd<int16_t>(f, nr), sy = rd<int16_t>(f, nr), dx = rd<int16_t>(f, nr), dy = rd<int16_t>(f, nr);
    const auto bw = rd<uint8_t>(f, nr), bh = rd<uint8_t>(f, nr);
    const auto q_pt = rd<float>(f, 2 * nq);
    std::fclose(f);
    if (rec_ptr[nf] != (int32_t)nr || q_ptr[nf] != (int32_t)nq) { std::fprintf(stderr, "mvr_main: the counts do not match\n"); return 2; }
    std::vector<int32_t> g_ptr(nf + 1, 0), tile_ptr(nf + 1, 0);
    for (size_t i = 0; i < nf; ++i) {
        g_ptr[i + 1] = g_ptr[i] + (int32_t)adv_lattice(rows[i], cols[i]);
        tile_ptr[i + 1] = tile_ptr[i] + (int32_t)mvr_tiles(rows[i], cols[i]);
    }
    const size_t ng = (size_t)g_ptr[nf], nt = (size_t)tile_ptr[nf];

    // scratch, exactly as long as the kernels' (the sanitizer sees an index past an end)
    std::vector<int32_t> kept_rec(nr), kept_cnt(nf), cover(nf), kept_base(nf + 1), tile_off(nt + 1, 0), tile_cur(nt), list_m(4 * nr);
    std::vector<uint64_t> list_ext(4 * nr);
    std::vector<int32_t> kept_ptr(nf + 1), kp_rect(4 * nr), mv_dindx(nr), rec_kept(nr), cand(4 * nq), grid_ptr(nf + 1), cover_px(nf);
    std::vector<float> mv_pt(2 * nr);
    std::vector<double> area(nf);
    std::vector<uint8_t> covered(ng), force(nf);

    MvrDev d{};
    d.n_frames = (int32_t)nf; d.n_records = (int32_t)nr; d.n_q = (int32_t)nq; d.n_grid = (int32_t)ng; d.n_tiles = (int32_t)nt;
    d.rows = rows.data(); d.cols = cols.data(); d.rec_ptr = rec_ptr.data(); d.q_ptr = q_ptr.data(); d.g_ptr = g_ptr.data(); d.tile_ptr = tile_ptr.data();
    d.threshold = threshold.data(); d.want_grid = want.data();
    d.src_x = sx.data(); d.src_y = sy.data(); d.dst_x = dx.data(); d.dst_y = dy.data(); d.w = bw.data(); d.h = bh.data(); d.q_pt = q_pt.data();
    d.kept_rec = kept_rec.data(); d.kept_cnt = kept_cnt.data(); d.cover = cover.data(); d.kept_base = kept_base.data();
    d.tile_off = tile_off.data(); d.tile_cur = tile_cur.data(); d.list_m = list_m.data(); d.list_ext = list_ext.data();
    d.kept_ptr = kept_ptr.data(); d.kp_rect = kp_rect.data(); d.mv_dindx = mv_dindx.data(); d.rec_kept = rec_kept.data(); d.cand = cand.data();
    d.grid_ptr = grid_ptr.data(); d.cover_px = cover_px.data(); d.mv_pt = mv_pt.data(); d.coverage_area = area.data();
    d.grid_covered = covered.data(); d.force_grid = force.data();
    mvr_frames(d);

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, kept_ptr); wr(o, kp_rect); wr(o, mv_pt); wr(o, mv_dindx); wr(o, rec_kept); wr(o, cand); wr(o, grid_ptr); wr(o, covered);
    wr(o, cover_px); wr(o, area); wr(o, force);
    std::fclose(o);
    std::printf("mvr_main: ok\n");
    return 0;
}
