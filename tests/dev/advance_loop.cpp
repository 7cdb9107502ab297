// The inter-frame walk movba_advance replaces, as a caller without it writes it, on one thread, from the rules of include/movba.h:
// the sort, per feature the candidate loop with compute_descriptor and compute_distance, the cv::Rect truncation, the lbFound
// bookkeeping, the dist <= 40 gate, the new macroblocks, mov_cnt and the grid of extract_moves - over the frames where they lie,
// without the cv::Mat headers the reference builds per block: a lower bound of the caller's cost.  Built and run by
// tests/dev/advance_time.py; prints the median and minimum time of `reps` walks over all frames and a checksum of the results (the
// tool compares it with the device's).
//   advance_loop <in> <reps>      in: the format of tests/advance/adv_main.cpp
#include <algorithm>
#include <bitset>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

template <typename T> static std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "advance_loop: short input\n"); std::exit(2); }
    return a;
}

struct Blk {
    const uint8_t *p;
    int step, cols, rows;
    uint8_t at(int row, int col) const { return p[(size_t)row * step + col]; }
};

static uint8_t center_of(const Blk &m)
{
    const uint8_t center_row = (uint8_t)(m.rows / 2), center_col = (uint8_t)(m.cols / 2);
    return (uint8_t)((m.at(center_col, center_row) + m.at(center_col - 1, center_row - 1) + m.at(center_col, center_row - 1) + m.at(center_col - 1, center_row)) / 4);
}

static void descriptor_of(const Blk &m, int threshold, std::bitset<256> &desc)
{
    const uint8_t center = center_of(m), low = (uint8_t)(center - threshold), high = (uint8_t)(center + threshold);
    desc.reset();
    for (int y = 0; y < m.rows; ++y) {
        const uint8_t *p = m.p + (size_t)y * m.step;
        for (int x = 0; x < m.cols; ++x) {
            p++;
            if (low > *p || high < *p) desc.set((size_t)(y * m.rows + x), true);
        }
    }
}

static bool express_of(const Blk &m, int threshold)
{
    const uint8_t center = center_of(m), low = (uint8_t)(center - threshold), high = (uint8_t)(center + threshold);
    const uint8_t precheck = (uint8_t)(m.rows * m.cols * .125);
    uint8_t f = 0;
    for (int row = 0; row < m.rows; ++row) {
        const uint8_t *p = m.p + (size_t)row * m.step;
        for (int col = 0; col < m.cols; ++col) {
            p++;
            if (low > *p || high < *p) f++;
        }
        if (f >= precheck) break;
    }
    if (f < precheck) return false;
    const uint8_t slices = (uint8_t)(m.rows + m.cols - 1), rounds = (uint8_t)std::round(slices * .25), u_rounds = (uint8_t)(slices - rounds);
    for (int a = 0; a < 2; ++a) {
        uint8_t wins = 0, losses = 0;
        for (int i = 0; i < slices; ++i) {
            const int k0 = i - (m.rows - 1), y0 = k0 < 0 ? -k0 : 0, y1 = std::min(m.rows, m.cols - k0);
            const uint8_t *p = m.p + (size_t)y0 * m.step + (a == 0 ? y0 + k0 : m.cols - 1 - (y0 + k0));
            const std::ptrdiff_t step = m.step + (a == 0 ? 1 : -1);
            uint8_t win = 0, loss = 0;
            for (int y = y0; y < y1; ++y, p += step) {
                if (low > *p || high < *p) win++; else loss++;
            }
            if (wins < rounds) { if (win >= loss) wins++; else wins = 0; }
            if (losses < rounds) { if (loss > win) losses++; else losses = 0; }
            if (i > u_rounds && (wins == 0 || losses == 0)) break;
        }
        if (wins >= rounds && losses >= rounds) return true;
    }
    return false;
}

static bool inside(int x, int y, int w, int h, int rows, int cols) { return x >= 0 && y >= 0 && x + w < cols && y + h < rows; }
static bool known_shape(int w, int h) { return (w == 8 || w == 16) && (h == 8 || h == 16); }

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: advance_loop <in> <reps>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int reps = std::atoi(argv[2]);
    const std::vector<int32_t> hd = rd<int32_t>(f, 5);
    const size_t nf = (size_t)hd[0], np = (size_t)hd[1], nm = (size_t)hd[2], nk = (size_t)hd[3], ng = (size_t)hd[4];
    const auto rows = rd<int32_t>(f, nf), cols = rd<int32_t>(f, nf), threshold = rd<int32_t>(f, nf), force_grid = rd<int32_t>(f, nf), first_id = rd<int32_t>(f, nf);
    const auto prev_ptr = rd<int32_t>(f, nf + 1), mv_ptr = rd<int32_t>(f, nf + 1), kp_ptr = rd<int32_t>(f, nf + 1), g_ptr = rd<int32_t>(f, nf + 1);
    const auto prev_pt = rd<float>(f, 2 * np);
    const auto prev_mb = rd<int32_t>(f, 2 * np), prev_age = rd<int32_t>(f, np), prev_track = rd<int32_t>(f, np), prev_cand = rd<int32_t>(f, 4 * np);
    const auto prev_desc = rd<uint64_t>(f, 4 * np);
    const auto prev_coverage = rd<uint8_t>(f, np);
    const auto mv_pt = rd<float>(f, 2 * nm);
    const auto mv_dindx = rd<int32_t>(f, nm), kp_rect = rd<int32_t>(f, 4 * nk);
    const auto covered = rd<uint8_t>(f, ng);
    std::vector<std::vector<uint8_t>> images;
    for (size_t i = 0; i < nf; ++i) images.push_back(rd<uint8_t>(f, (size_t)rows[i] * (size_t)cols[i]));
    std::fclose(f);

    std::vector<std::bitset<256>> pdesc(np);
    for (size_t g = 0; g < np; ++g)
        for (int b = 0; b < 256; ++b) pdesc[g][(size_t)b] = (prev_desc[4 * g + (size_t)(b >> 6)] >> (b & 63)) & 1;

    std::vector<double> ms;
    long long checksum = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        checksum = 0;
        for (size_t fr = 0; fr < nf; ++fr) {
            const int R = rows[fr], C = cols[fr], thr = threshold[fr];
            const uint8_t *img = images[fr].data();
            const int p0 = prev_ptr[fr], n = prev_ptr[fr + 1] - p0, k0 = kp_ptr[fr], kn = kp_ptr[fr + 1] - k0, m0 = mv_ptr[fr];
            std::vector<int> order((size_t)n);
            std::iota(order.begin(), order.end(), 0);
            std::vector<int> count((size_t)n);
            for (int i = 0; i < n; ++i) count[(size_t)i] = (int)pdesc[(size_t)(p0 + i)].count();
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                return prev_age[(size_t)(p0 + a)] == prev_age[(size_t)(p0 + b)] ? count[(size_t)a] > count[(size_t)b] : prev_age[(size_t)(p0 + a)] > prev_age[(size_t)(p0 + b)];
            });
            std::vector<char> found((size_t)kn, 0);
            int current = first_id[fr];
            long long kept = 0, sum = 0;
            std::bitset<256> desc;
            for (int i = 0; i < n; ++i) {
                const size_t g = (size_t)(p0 + order[(size_t)i]);
                if (prev_coverage[g]) continue;
                const int32_t *cand = &prev_cand[4 * g];
                if (cand[0] == -1) continue;
                const int w = prev_mb[2 * g], h = prev_mb[2 * g + 1];
                int indx = cand[0];
                if (cand[1] >= 0) {
                    int best = 256;
                    for (int j = 0; j < 4; ++j) {
                        if (cand[j] == -1) break;
                        const float px = prev_pt[2 * g] + mv_pt[2 * (size_t)(m0 + cand[j])], py = prev_pt[2 * g + 1] + mv_pt[2 * (size_t)(m0 + cand[j]) + 1];
                        const int x = (int)(px - (float)(w / 2)), y = (int)(py - (float)(h / 2));
                        if (!inside(x, y, w, h, R, C)) continue;
                        descriptor_of(Blk{ img + (size_t)y * C + x, C, w, h }, thr, desc);
                        const int dist = (int)(pdesc[g] ^ desc).count();
                        if (dist < best) { best = dist; indx = cand[j]; }
                    }
                }
                const float px = prev_pt[2 * g] + mv_pt[2 * (size_t)(m0 + indx)], py = prev_pt[2 * g + 1] + mv_pt[2 * (size_t)(m0 + indx) + 1];
                const int x = (int)(px - (float)(w / 2)), y = (int)(py - (float)(h / 2)), d = mv_dindx[(size_t)(m0 + indx)];
                if ((d == -1 || !found[(size_t)d]) && inside(x, y, w, h, R, C)) {
                    if (d >= 0) found[(size_t)d] = 1;
                    descriptor_of(Blk{ img + (size_t)y * C + x, C, w, h }, thr, desc);
                    const int dist = (int)(pdesc[g] ^ desc).count();
                    if (dist <= 40) { ++kept; sum += (long long)prev_track[g] + i + x + y + (long long)desc.count(); }
                }
            }
            int mov_cnt = 0;
            for (int m = 0; m < kn; ++m) {
                if (found[(size_t)m]) continue;
                const int32_t *rc = &kp_rect[4 * (size_t)(k0 + m)];
                if (!inside(rc[0], rc[1], rc[2], rc[3], R, C) || !known_shape(rc[2], rc[3])) continue;
                const Blk blk{ img + (size_t)rc[1] * C + rc[0], C, rc[2], rc[3] };
                if (!express_of(blk, thr)) continue;
                descriptor_of(blk, thr, desc);
                ++current; ++mov_cnt;
                sum += (long long)current + m + (long long)desc.count();
            }
            int grid = 0;
            if (force_grid[fr] || mov_cnt < 60) {
                int gi = 0;
                for (int y = 8; y < R - 8; y += 16)
                    for (int x = 8; x < C - 8; x += 16, ++gi) {
                        const Blk blk{ img + (size_t)(y - 8) * C + (x - 8), C, 16, 16 };
                        if (!express_of(blk, thr)) continue;
                        descriptor_of(blk, thr, desc);
                        if (covered[(size_t)(g_ptr[fr] + gi)]) continue;
                        ++current; ++grid;
                        sum += (long long)current + gi + (long long)desc.count();
                    }
            }
            checksum += sum + 1000003LL * kept + 1009LL * mov_cnt + 7LL * grid + current;
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("{\"host_loop\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"checksum\": %lld}}\n", ms[ms.size() / 2], ms.front(), checksum);
    return 0;
}
