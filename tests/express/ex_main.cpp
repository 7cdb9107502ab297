// movba_express's steps on the CPU: ex_item and ex_counts of mov-slam_amd/csrc/express.h - the two tests that keep a rectangle
// from being read, the centre, the wrapped bounds, the diagonals' masks, the descriptor's bit order, the vote state machine, the
// functions k_express calls from its lanes - item by item.  Every image lies in a buffer of exactly rows x cols bytes, so a read
// outside it is seen.  Built stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (no library source is linked);
// tests/test_express_cpu.py writes the call to a file, runs this and compares with the restatement.
//   ex_main <in> <out>
//   in:  int32 n_images n_items has_ref; int32 rows[ni] cols[ni] threshold[ni] item_ptr[ni + 1] item_rect[4 n] item_mode[n];
//        if has_ref: uint64 item_ref[4 n]; uint8 the images' pixels, rows tight, image after image
//   out: int32 count[n] distance[n] n_features[ni] pass[n] (0: none, 1: pass 0, 2: pass 1); uint64 desc[4 n]; uint8 code[n]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "express.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "ex_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "ex_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ex_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 3);
    const size_t ni = (size_t)hd[0], n = (size_t)hd[1];
    const auto rows = rd<int32_t>(f, ni), cols = rd<int32_t>(f, ni), threshold = rd<int32_t>(f, ni), item_ptr = rd<int32_t>(f, ni + 1);
    const auto item_rect = rd<int32_t>(f, 4 * n), item_mode = rd<int32_t>(f, n);
    const auto item_ref = rd<uint64_t>(f, hd[2] ? 4 * n : 0);
    // (one buffer per image, exactly as long as the image: the sanitizer sees a byte past its end)
    std::vector<std::vector<uint8_t>> images;
    for (size_t i = 0; i < ni; ++i) images.push_back(rd<uint8_t>(f, (size_t)rows[i] * (size_t)cols[i]));
    std::fclose(f);

    std::vector<int32_t> count(n), distance(n), n_features(ni), pass(n), item_image(n), zero(1, 0);
    std::vector<uint64_t> desc(4 * n);
    std::vector<uint8_t> code(n);
    for (size_t i = 0; i < ni; ++i) {
        // the library's device view of ONE image at a time: its items, its pixels at offset 0
        const int32_t first = item_ptr[i], m = item_ptr[i + 1] - first;
        if (m < 0 || (size_t)item_ptr[i + 1] > n) { std::fprintf(stderr, "ex_main: item_ptr is no prefix\n"); return 2; }
        int32_t features = 0;
        ExDev d{};
        d.n_images = 1; d.n_items = m;
        d.pixels = images[i].data(); d.img_off = zero.data(); d.rows = &rows[i]; d.cols = &cols[i]; d.threshold = &threshold[i];
        d.item_rect = item_rect.data() + 4 * (size_t)first; d.item_mode = item_mode.data() + first;
        d.item_image = item_image.data() + first;           // (all 0)
        d.item_ref = hd[2] ? item_ref.data() + 4 * (size_t)first : nullptr;
        d.features = &features;
        d.code = code.data() + first; d.desc = desc.data() + 4 * (size_t)first; d.count = count.data() + first; d.distance = distance.data() + first;
        d.n_features = &n_features[i];
        for (int32_t k = 0; k < m; ++k) pass[(size_t)first + k] = ex_item(d, k);
        ex_counts(d);
    }

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, count); wr(o, distance); wr(o, n_features); wr(o, pass); wr(o, desc); wr(o, code);
    std::fclose(o);
    std::printf("ex_main: ok\n");
    return 0;
}
