// movba_stereo_points' steps on the CPU: st_frames of mov-slam_amd/csrc/stereo_points.h - the gates, the int distance, the select
// of the upper median, the pruning, the selection keys and the walk's length, the un-projection, the functions the kernels call -
// over one call, serially.  Every buffer is exactly as long as the kernels', so an index past an end is seen.  Built stand-alone
// under AddressSanitizer + UndefinedBehaviorSanitizer (no library source is linked); the test writes the call to a file, runs
// this and compares with the restatement.
//   stereo_main <in> <out> [reps]      reps: the walk runs that often more, timed (tests/dev/stereo_time.py, an -O2 build without
//                                     sanitizers), and a line {"median_ms": .., "min_ms": ..} follows
//   in:  int32 n_frames n_pt max_point flags (1: pt_un, 2: poses, 4: has_point); float max_row_diff min_disparity;
//        int32 rows[nf] cols[nf] select[nf] pt_ptr[nf + 1]; float bf[nf] max_disparity[nf] th_depth[nf] cam[4 nf];
//        float pt[2 n_pt] next_pt[2 n_pt]; uint8 pt_status[n_pt]; then, where flagged: float pt_un[2 n_pt]; double poses[7 nf];
//        uint8 has_point[n_pt]
//   out: float u_right[n_pt] depth[n_pt]; uint8 code[n_pt]; int32 n_stereo[nf] median_dist[nf]; float th_dist[nf];
//        int32 sel_ptr[nf + 1] sel_src[n_pt]; uint8 sel_new[n_pt]; float sel_cam[3 n_pt]; double sel_point[3 n_pt]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stereo_points.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "stereo_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "stereo_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: stereo_main <in> <out> [reps]\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 4);
    const std::vector<float> par = rd<float>(f, 2);
    const size_t nf = (size_t)hd[0], np = (size_t)hd[1];
    const auto rows = rd<int32_t>(f, nf), cols = rd<int32_t>(f, nf), select = rd<int32_t>(f, nf), pt_ptr = rd<int32_t>(f, nf + 1);
    const auto bf = rd<float>(f, nf), max_disparity = rd<float>(f, nf), th_depth = rd<float>(f, nf), cam = rd<float>(f, 4 * nf);
    const auto pt = rd<float>(f, 2 * np), next_pt = rd<float>(f, 2 * np);
    const auto status = rd<uint8_t>(f, np);
    const auto pt_un = rd<float>(f, hd[3] & 1 ? 2 * np : 0);
    const auto poses = rd<double>(f, hd[3] & 2 ? 7 * nf : 0);
    const auto has = rd<uint8_t>(f, hd[3] & 4 ? np : 0);
    std::fclose(f);
    if (pt_ptr[nf] != (int32_t)np) { std::fprintf(stderr, "stereo_main: the counts do not match\n"); return 2; }

    std::vector<StFrame> frames(nf);
    int32_t max_close = 0;
    for (size_t i = 0; i < nf; ++i) {
        StFrame &fr = frames[i];
        fr = StFrame{};
        fr.rows = rows[i]; fr.cols = cols[i]; fr.select = select[i];
        fr.bf = bf[i]; fr.max_disparity = max_disparity[i]; fr.th_depth = th_depth[i];
        fr.fx = cam[4 * i]; fr.fy = cam[4 * i + 1]; fr.cx = cam[4 * i + 2]; fr.cy = cam[4 * i + 3];
        st_frame_pose(hd[3] & 2 ? poses.data() + 7 * i : nullptr, &fr);
        if (select[i] == MOVBA_STEREO_SELECT_CLOSE && pt_ptr[i + 1] - pt_ptr[i] > max_close) max_close = pt_ptr[i + 1] - pt_ptr[i];
    }
    std::vector<int32_t> dist(np), list(np), counts(nf), n_stereo(nf), median(nf), sel_ptr(nf + 1), sel_src(np);
    std::vector<float> z(np), u_right(np), depth(np), th(nf), sel_cam(3 * np);
    std::vector<uint8_t> code(np), sel_new(np);
    std::vector<double> sel_point(3 * np);
    StDev d{};
    d.n_frames = (int32_t)nf; d.n_pt = (int32_t)np; d.max_point = hd[2]; d.max_close = max_close;
    d.max_row_diff = par[0]; d.min_disparity = par[1];
    d.frame = frames.data(); d.pt_ptr = pt_ptr.data(); d.pt = pt.data(); d.next_pt = next_pt.data();
    d.pt_un = hd[3] & 1 ? pt_un.data() : pt.data();
    d.pt_status = status.data(); d.has_point = hd[3] & 4 ? has.data() : nullptr;
    d.dist = dist.data(); d.z = z.data(); d.list = list.data(); d.counts = counts.data();
    d.u_right = u_right.data(); d.depth = depth.data(); d.code = code.data(); d.n_stereo = n_stereo.data(); d.median_dist = median.data();
    d.th_dist = th.data(); d.sel_ptr = sel_ptr.data(); d.sel_src = sel_src.data(); d.sel_new = sel_new.data(); d.sel_cam = sel_cam.data();
    d.sel_point = sel_point.data();
    st_frames(d);

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, u_right); wr(o, depth); wr(o, code); wr(o, n_stereo); wr(o, median); wr(o, th); wr(o, sel_ptr); wr(o, sel_src); wr(o, sel_new);
    wr(o, sel_cam); wr(o, sel_point);
    std::fclose(o);
    std::printf("stereo_main: ok\n");
    if (argc == 4) {
        std::vector<double> ms;
        for (int rep = 0; rep < std::atoi(argv[3]); ++rep) {
            const auto t0 = std::chrono::steady_clock::now();
            st_frames(d);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        if (!ms.empty()) std::printf("{\"median_ms\": %.6f, \"min_ms\": %.6f}\n", ms[ms.size() / 2], ms[0]);
    }
    return 0;
}
