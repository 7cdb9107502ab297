// movba_point_normals' arithmetic on the CPU: pn_centre view by view and the per-point function of
// mov-slam_amd/csrc/point_normals.h - what k_pn_points inlines for both entry points - point by point, with and without a mask
// and a permutation in front of it.  Built stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (no library source is
// linked); tests/test_point_normals_cpu.py writes the call to a file, runs this and compares with the restatement.
//   pn_main <in> <out>
//   in:  int32 n_views n_points n_levels n_obs has_mask; double poses[7 nv] points[3 np]; int32 obs_ptr[np + 1] obs_view[n_obs]
//        ref_view[np] ref_level[np]; double scale[n_levels]; if has_mask: int32 perm[n_obs]; uint8 mask[n_obs]
//   out: double normals[3 np] max[np] min[np]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "point_normals.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "pn_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "pn_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: pn_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 5);
    const size_t nv = (size_t)hd[0], np = (size_t)hd[1], nl = (size_t)hd[2], n_obs = (size_t)hd[3];
    const bool has_mask = hd[4] != 0;
    const auto poses = rd<double>(f, 7 * nv), points = rd<double>(f, 3 * np);
    const auto obs_ptr = rd<int32_t>(f, np + 1), obs_view = rd<int32_t>(f, n_obs), ref_view = rd<int32_t>(f, np), ref_level = rd<int32_t>(f, np);
    const auto scale = rd<double>(f, nl);
    const auto perm = rd<int32_t>(f, has_mask ? n_obs : 0);
    const auto mask = rd<uint8_t>(f, has_mask ? n_obs : 0);
    std::fclose(f);

    // (exactly as long as they must be: the sanitizer sees an index one past the end)
    std::vector<double> centres(3 * nv), normals(3 * np), dmax(np), dmin(np);
    for (size_t v = 0; v < nv; ++v) pn_centre(&poses[7 * v], &centres[3 * v]);
    PnLists L{};
    L.ptr = obs_ptr.data(); L.view = obs_view.data();
    if (has_mask) { L.perm = perm.data(); L.mask = mask.data(); }
    for (size_t p = 0; p < np; ++p) {
        const PnPoint r = pn_point(&points[3 * p], L, p, centres.data(), ref_view[p], ref_level[p], scale.data(), (int32_t)nl);
        for (int k = 0; k < 3; ++k) normals[3 * p + k] = r.normal[k];
        dmax[p] = r.max_distance; dmin[p] = r.min_distance;
    }

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, normals); wr(o, dmax); wr(o, dmin);
    std::fclose(o);
    std::printf("pn_main: ok\n");
    return 0;
}
