// The block loop movba_express replaces, as a caller without it writes it, on one thread: compute_express and compute_descriptor
// of EXPRESS.h:79-192 item by item over the images where they lie - the precheck with its row-wise `break`, the two diagonal
// passes with theirs, the descriptor only where the detector passed, the distance where a reference is given - without the
// cv::Mat headers the reference builds per block and per diagonal: a lower bound of the caller's cost.  Built and run by
// tests/dev/express_time.py; prints the median and minimum time of `reps` passes over all items and a checksum of the results (the
// tool compares it with the device's).
//   express_loop <in> <reps>      in: the format of tests/express/ex_main.cpp
#include <algorithm>
#include <bitset>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename T> static std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "express_loop: short input\n"); std::exit(2); }
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

// -1: the precheck failed, 0: no pass succeeded, 1: one did
static int express_of(const Blk &m, int threshold)
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
    if (f < precheck) return -1;
    const uint8_t slices = (uint8_t)(m.rows + m.cols - 1), rounds = (uint8_t)std::round(slices * .25), u_rounds = (uint8_t)(slices - rounds);
    for (int a = 0; a < 2; ++a) {
        uint8_t wins = 0, losses = 0;
        for (int i = 0; i < slices; ++i) {
            // diagonal i: from its first row down, one column right (pass 0) or left (pass 1) per row
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
        if (wins >= rounds && losses >= rounds) return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: express_loop <in> <reps>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int reps = std::atoi(argv[2]);
    const std::vector<int32_t> hd = rd<int32_t>(f, 3);
    const size_t ni = (size_t)hd[0], n = (size_t)hd[1];
    const auto rows = rd<int32_t>(f, ni), cols = rd<int32_t>(f, ni), threshold = rd<int32_t>(f, ni), item_ptr = rd<int32_t>(f, ni + 1);
    const auto rect = rd<int32_t>(f, 4 * n), mode = rd<int32_t>(f, n);
    const auto ref = rd<uint64_t>(f, hd[2] ? 4 * n : 0);
    std::vector<std::vector<uint8_t>> images;
    for (size_t i = 0; i < ni; ++i) images.push_back(rd<uint8_t>(f, (size_t)rows[i] * (size_t)cols[i]));
    std::fclose(f);

    std::vector<uint8_t> code(n);
    std::vector<std::bitset<256>> desc(n);
    std::vector<int32_t> count(n), distance(n);
    std::vector<double> ms;
    uint64_t checksum = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t i = 0; i < ni; ++i)
            for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
                const int32_t x = rect[4 * (size_t)k], y = rect[4 * (size_t)k + 1], w = rect[4 * (size_t)k + 2], h = rect[4 * (size_t)k + 3];
                count[k] = distance[k] = -1;
                desc[k].reset();
                if (!(x >= 0 && y >= 0 && (long long)x + w < cols[i] && (long long)y + h < rows[i])) { code[k] = 16; continue; }
                if (!((w == 8 || w == 16) && (h == 8 || h == 16))) { code[k] = 17; continue; }
                const Blk m{ images[i].data() + (size_t)y * cols[i] + x, cols[i], w, h };
                if (mode[k] == 0) {
                    const int e = express_of(m, threshold[i]);
                    if (e <= 0) { code[k] = e < 0 ? 18 : 19; continue; }
                    code[k] = 1;
                } else code[k] = 2;
                descriptor_of(m, threshold[i], desc[k]);
                count[k] = (int32_t)desc[k].count();
                if (hd[2]) {
                    std::bitset<256> r;
                    for (int b = 0; b < 256; ++b) r[b] = (ref[4 * (size_t)k + (b >> 6)] >> (b & 63)) & 1;
                    distance[k] = (int32_t)(r ^ desc[k]).count();
                }
            }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        // (what the device's code, count and distance add up to)
        uint64_t sum = 0;
        for (size_t k = 0; k < n; ++k) sum += (uint64_t)code[k] + 7 * (uint64_t)(count[k] + 1) + 13 * (uint64_t)(distance[k] + 1);
        checksum = sum;
    }
    std::sort(ms.begin(), ms.end());
    std::printf("{\"host_loop\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"checksum\": %llu}}\n", ms[ms.size() / 2], ms[0], (unsigned long long)checksum);
    return 0;
}
