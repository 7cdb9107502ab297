// movba_advance's steps on the CPU: adv_frames of mov-slam_amd/csrc/advance.h - the sort key, the rect of a vector with its fp32
// operations and its truncation, the candidate loop, the claims, the gate, the prefix sums and the id arithmetic, the functions
// the kernels call - over one call, serially.  The pixels lie in a buffer of exactly the frames' bytes, so a read behind the last
// frame is seen (tests/test_advance_cpu.py also hands every frame over alone).  Built stand-alone under AddressSanitizer +
// UndefinedBehaviorSanitizer (no library source is linked); the test writes the call to a file, runs this and compares with the
// restatement.
//   adv_main <in> <out>
//   in:  int32 n_frames n_prev n_mv n_kps n_grid; int32 rows[nf] cols[nf] threshold[nf] force_grid[nf] first_id[nf];
//        int32 prev_ptr[nf + 1] mv_ptr[nf + 1] kp_ptr[nf + 1] g_ptr[nf + 1]; float prev_pt[2 np]; int32 prev_mb[2 np] prev_age[np]
//        prev_track[np] prev_cand[4 np]; uint64 prev_desc[4 np]; uint8 prev_coverage[np]; float mv_pt[2 nm]; int32 mv_dindx[nm]
//        kp_rect[4 nk]; uint8 covered[ng]; uint8 the frames' pixels, rows tight, frame after frame
//   out: int32 order[np] chosen_mv[np] distance[np] mov_cnt[nf] next_id[nf] seg_ptr[4 nf + 1] feat_src[cap] feat_track[cap]
//        feat_rect[4 cap] feat_age[cap]; float feat_pt[2 cap]; uint64 feat_desc[4 cap]; uint8 fate[np] kp_found[nk] kp_code[nk]
//        grid_ran[nf]                                                     (cap = np + nk + ng)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "advance.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "adv_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "adv_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: adv_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 5);
    const size_t nf = (size_t)hd[0], np = (size_t)hd[1], nm = (size_t)hd[2], nk = (size_t)hd[3], ng = (size_t)hd[4], cap = np + nk + ng;
    const auto rows = rd<int32_t>(f, nf), cols = rd<int32_t>(f, nf), threshold = rd<int32_t>(f, nf), force_grid = rd<int32_t>(f, nf), first_id = rd<int32_t>(f, nf);
    const auto prev_ptr = rd<int32_t>(f, nf + 1), mv_ptr = rd<int32_t>(f, nf + 1), kp_ptr = rd<int32_t>(f, nf + 1), g_ptr = rd<int32_t>(f, nf + 1);
    const auto prev_pt = rd<float>(f, 2 * np);
    const auto prev_mb = rd<int32_t>(f, 2 * np), prev_age = rd<int32_t>(f, np), prev_track = rd<int32_t>(f, np), prev_cand = rd<int32_t>(f, 4 * np);
    const auto prev_desc = rd<uint64_t>(f, 4 * np);
    const auto prev_coverage = rd<uint8_t>(f, np);
    const auto mv_pt = rd<float>(f, 2 * nm);
    const auto mv_dindx = rd<int32_t>(f, nm), kp_rect = rd<int32_t>(f, 4 * nk);
    const auto covered = rd<uint8_t>(f, ng);
    std::vector<int32_t> img_off(nf);
    size_t bytes = 0;
    for (size_t i = 0; i < nf; ++i) { img_off[i] = (int32_t)bytes; bytes += (size_t)rows[i] * (size_t)cols[i]; }
    const auto pixels = rd<uint8_t>(f, bytes);
    std::fclose(f);
    if (prev_ptr[nf] != (int32_t)np || mv_ptr[nf] != (int32_t)nm || kp_ptr[nf] != (int32_t)nk || g_ptr[nf] != (int32_t)ng) { std::fprintf(stderr, "adv_main: the counts do not match\n"); return 2; }

    // scratch, exactly as long as the kernels' (the sanitizer sees an index past an end)
    std::vector<int32_t> claim(nk, kAdvNoClaim), pos(np), ord(np), it_code(cap), it_rank(cap), pf_xy(2 * np), pf_d(np), pf_dist(np), counts(3 * nf);
    std::vector<uint64_t> it_desc(4 * cap);
    std::vector<float> pf_pt(2 * np);
    std::vector<int32_t> order(np), chosen(np), distance(np), mov_cnt(nf), next_id(nf), seg_ptr(4 * nf + 1), feat_src(cap), feat_track(cap), feat_rect(4 * cap), feat_age(cap);
    std::vector<float> feat_pt(2 * cap);
    std::vector<uint64_t> feat_desc(4 * cap);
    std::vector<uint8_t> fate(np), kp_found(nk), kp_code(nk), grid_ran(nf);

    AdvDev d{};
    d.n_frames = (int32_t)nf; d.n_items = (int32_t)cap;
    for (size_t i = 0; i < nf; ++i) d.max_prev = std::max(d.max_prev, prev_ptr[i + 1] - prev_ptr[i]);
    d.pixels = pixels.data(); d.img_off = img_off.data(); d.rows = rows.data(); d.cols = cols.data(); d.threshold = threshold.data();
    d.force_grid = force_grid.data(); d.first_id = first_id.data();
    d.prev_ptr = prev_ptr.data(); d.mv_ptr = mv_ptr.data(); d.kp_ptr = kp_ptr.data(); d.g_ptr = g_ptr.data();
    d.prev_pt = prev_pt.data(); d.mv_pt = mv_pt.data(); d.prev_mb = prev_mb.data(); d.prev_age = prev_age.data(); d.prev_track = prev_track.data();
    d.prev_cand = prev_cand.data(); d.prev_desc = prev_desc.data(); d.prev_coverage = prev_coverage.data(); d.covered = covered.data();
    d.mv_dindx = mv_dindx.data(); d.kp_rect = kp_rect.data();
    d.claim = claim.data(); d.pos = pos.data(); d.ord = ord.data(); d.it_desc = it_desc.data(); d.it_code = it_code.data(); d.it_rank = it_rank.data();
    d.pf_pt = pf_pt.data(); d.pf_xy = pf_xy.data(); d.pf_d = pf_d.data(); d.pf_dist = pf_dist.data(); d.counts = counts.data();
    d.order = order.data(); d.chosen_mv = chosen.data(); d.distance = distance.data(); d.mov_cnt = mov_cnt.data(); d.next_id = next_id.data();
    d.seg_ptr = seg_ptr.data(); d.fate = fate.data(); d.kp_found = kp_found.data(); d.kp_code = kp_code.data(); d.grid_ran = grid_ran.data();
    d.feat_src = feat_src.data(); d.feat_track = feat_track.data(); d.feat_rect = feat_rect.data(); d.feat_age = feat_age.data();
    d.feat_pt = feat_pt.data(); d.feat_desc = feat_desc.data();
    adv_frames(d);

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, order); wr(o, chosen); wr(o, distance); wr(o, mov_cnt); wr(o, next_id); wr(o, seg_ptr); wr(o, feat_src); wr(o, feat_track);
    wr(o, feat_rect); wr(o, feat_age); wr(o, feat_pt); wr(o, feat_desc); wr(o, fate); wr(o, kp_found); wr(o, kp_code); wr(o, grid_ran);
    std::fclose(o);
    std::printf("adv_main: ok\n");
    return 0;
}
