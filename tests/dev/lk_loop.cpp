// Developer tool (tests/dev/lk_time.py): movba_lk_track's work on ONE host thread - lk_frames of mov-slam_amd/csrc/lk.h: both
// pyramids, then every point's walk, the same statements the kernels run - timed over a call in the format of
// tests/lk/lk_main.cpp.  It is the library's own arithmetic, not OpenCV's SIMD path: what it measures is what this code costs
// serially, compiled with -O2.  Prints one JSON line: median and minimum over the repetitions and a checksum of the results.
//   lk_loop <in> <reps>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lk.h"

using namespace movba;

template <typename T> static std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "lk_loop: short input\n"); std::exit(2); }
    return a;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: lk_loop <in> <reps>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int reps = std::max(1, std::atoi(argv[2]));
    const std::vector<int32_t> hd = rd<int32_t>(f, 4);
    const std::vector<double> par = rd<double>(f, 2);
    const size_t nf = (size_t)hd[0], np = (size_t)hd[1];
    const auto rows = rd<int32_t>(f, nf), cols = rd<int32_t>(f, nf), win = rd<int32_t>(f, nf), pt_ptr = rd<int32_t>(f, nf + 1);
    const auto pt = rd<float>(f, 2 * np);
    std::vector<LkFrame> frames(nf);
    std::vector<int32_t> lvl((kLkLevels - 1) * (nf + 1), 0);
    size_t bytes = 0;
    for (size_t i = 0; i < nf; ++i) {
        lk_frame_levels(rows[i], cols[i], win[i], hd[2], &frames[i]);
        const bool used = pt_ptr[i + 1] > pt_ptr[i];
        for (int l = 1; l < kLkLevels; ++l) {
            int32_t *p = lvl.data() + (size_t)(l - 1) * (nf + 1) + i;
            p[1] = p[0] + (used && l <= frames[i].levels ? frames[i].rows[l] * frames[i].cols[l] : 0);
        }
        for (int img = 0; img < 2; ++img)
            for (int l = 0; l < kLkLevels; ++l) {
                frames[i].off[img][l] = 0;
                if (!used || l > frames[i].levels) continue;
                frames[i].off[img][l] = (int64_t)bytes;
                bytes += (size_t)frames[i].rows[l] * frames[i].cols[l];
            }
    }
    std::vector<uint8_t> pix(bytes);
    for (size_t i = 0; i < nf; ++i) {
        if (pt_ptr[i + 1] == pt_ptr[i]) continue;
        for (int img = 0; img < 2; ++img) {
            const size_t n = (size_t)rows[i] * cols[i];
            if (std::fread(pix.data() + frames[i].off[img][0], 1, n, f) != n) { std::fprintf(stderr, "lk_loop: short image\n"); return 2; }
        }
    }
    std::fclose(f);
    std::vector<int32_t> kept_cnt(nf), kept_ptr(nf + 1), kept_src(np);
    std::vector<float> next_pt(2 * np), err(np);
    std::vector<uint8_t> status(np), code(np), keep(np);
    LkDev d{};
    d.n_frames = (int32_t)nf; d.n_pt = (int32_t)np; d.max_iter = hd[3];
    for (int l = 1; l < kLkLevels; ++l) d.level_pixels[l - 1] = lvl[(size_t)(l - 1) * (nf + 1) + nf];
    d.eps_sq = par[0] * par[0]; d.min_eig = par[1];
    d.frame = frames.data(); d.pt_ptr = pt_ptr.data(); d.lvl_ptr = lvl.data(); d.pt = pt.data(); d.pix = pix.data(); d.kept_cnt = kept_cnt.data();
    d.next_pt = next_pt.data(); d.err = err.data(); d.pt_status = status.data(); d.exit_code = code.data(); d.keep = keep.data();
    d.kept_ptr = kept_ptr.data(); d.kept_src = kept_src.data();
    std::vector<double> ms;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        lk_frames(d);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    // (what lk_time.py's checksum adds up from the device's arrays)
    long long sum = 1000003LL * kept_ptr[nf];
    for (size_t i = 0; i < np; ++i) {
        uint32_t bx, by;
        std::memcpy(&bx, &next_pt[2 * i], 4); std::memcpy(&by, &next_pt[2 * i + 1], 4);
        sum += (long long)(bx >> 8) + (long long)(by >> 8) + 7 * code[i] + 13 * keep[i];
    }
    std::printf("{\"host_loop\": {\"median_ms\": %.4f, \"min_ms\": %.4f, \"checksum\": %lld}}\n", ms[ms.size() / 2], ms[0], sum);
    return 0;
}
