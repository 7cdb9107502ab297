// The loop movba_mv_raster replaces, as a caller without it writes it, on one thread, from the rules of include/movba.h: per frame
// the 4-channel image cleared to -1, the walk over the records with its keep test and clamps, kps and mvs pushed, every source
// block painted with the four-way slot fill, the coverage summed, and then the gathers MOVExtractor makes - at the previous
// features and at the lattice centres.  The image is allocated once and only cleared per frame (the reference allocates it per
// frame too): a lower bound of the caller's cost.  Built and run by tests/dev/mv_raster_time.py; prints the median and minimum
// time of `reps` passes over all frames and a checksum of the results (the tool compares it with the device's).
//   mv_raster_loop <in> <reps>      in: the format of tests/mv_raster/mvr_main.cpp
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename T> static std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "mv_raster_loop: short input\n"); std::exit(2); }
    return a;
}

struct Rect { int x, y, w, h; };
struct Mv { float x, y; int dindx; };

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: mv_raster_loop <in> <reps>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int reps = std::atoi(argv[2]);
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

    size_t most = 0;
    for (size_t i = 0; i < nf; ++i) most = std::max(most, (size_t)rows[i] * (size_t)cols[i]);
    std::vector<int32_t> mvi(4 * most);
    std::vector<Rect> kps;
    std::vector<Mv> mvs;
    std::vector<int32_t> cand(4 * nq);
    std::vector<double> ms;
    long long checksum = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        checksum = 0;
        for (size_t fr = 0; fr < nf; ++fr) {
            const int width = cols[fr], height = rows[fr];
            std::fill(mvi.begin(), mvi.begin() + 4 * (std::ptrdiff_t)((size_t)width * height), -1);
            kps.clear(); mvs.clear();
            float coverage = 0;
            for (int32_t i = rec_ptr[fr]; i < rec_ptr[fr + 1]; ++i) {
                const float mb_h = bh[i], mb_w = bw[i], mb_h_half = mb_h / 2, mb_w_half = mb_w / 2;
                const float mv_x = (float)(dx[i] - sx[i]), mv_y = (float)(dy[i] - sy[i]);
                const float dst_x = dx[i], dst_y = dy[i];
                float d_x_top = dst_x - mb_w_half, d_y_top = dst_y - mb_h_half;
                if (d_x_top < 0) d_x_top = 0;
                if (d_y_top < 0) d_y_top = 0;
                if (dst_x + mb_w_half >= width) continue;
                if (dst_y + mb_h_half >= height) continue;
                kps.push_back(Rect{ (int)d_x_top, (int)d_y_top, (int)mb_w, (int)mb_h });
                const int dindx = (int)kps.size() - 1;
                const float src_x = dst_x + mv_x * -1, src_y = dst_y + mv_y * -1;
                float s_x_top = src_x - mb_w_half, s_y_top = src_y - mb_h_half, s_x_bottom = src_x + mb_w_half, s_y_bottom = src_y + mb_h_half;
                if (s_x_top < 0) s_x_top = 0;
                if (s_y_top < 0) s_y_top = 0;
                if (s_x_bottom >= width) s_x_bottom = (float)(width - 1);
                if (s_y_bottom >= height) s_y_bottom = (float)(height - 1);
                mvs.push_back(Mv{ mv_x, mv_y, dindx });
                const int size = (int)mvs.size() - 1;
                for (int h = (int)s_y_top; h <= (int)s_y_bottom; ++h) {
                    int32_t *p = mvi.data() + 4 * (size_t)h * width;
                    for (int w = (int)s_x_top; w <= (int)s_x_bottom; ++w) {
                        int32_t *v = p + 4 * w;
                        if (v[0] == -1) v[0] = size;
                        else if (v[1] == -1) v[1] = size;
                        else if (v[2] == -1) v[2] = size;
                        else v[3] = size;
                    }
                }
                coverage += (float)((int)mb_w * (int)mb_h);
            }
            const double area = coverage / (double)(width * height);
            long long sum = 0;
            for (int32_t q = q_ptr[fr]; q < q_ptr[fr + 1]; ++q) {
                const int x = (int)q_pt[2 * q], y = (int)q_pt[2 * q + 1];
                for (int c = 0; c < 4; ++c) {
                    cand[4 * (size_t)q + c] = x >= 0 && y >= 0 && x < width && y < height ? mvi[4 * ((size_t)y * width + x) + c] : -1;
                    sum += (long long)(c + 1) * (cand[4 * (size_t)q + c] + 1);
                }
            }
            int covered = 0;
            if (want[fr])
                for (int y = 8; y < height - 8; y += 16)
                    for (int x = 8; x < width - 8; x += 16) covered += mvi[4 * ((size_t)y * width + x)] >= 0;
            checksum += sum + 1000003LL * (long long)kps.size() + 1009LL * covered + (long long)coverage + (area < threshold[fr] ? 7 : 0);
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("{\"host_loop\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"checksum\": %lld}}\n", ms[ms.size() / 2], ms.front(), checksum);
    return 0;
}
