// movba_view_points' arithmetic on the CPU: the per-item function of mov-slam_amd/csrc/view_points.h - what k_vp_items inlines -
// item by item, n_accepted counted from the codes, and the serial form of k_vp_views' radix select (vp_select_serial) on the
// order keys of every DEPTH view.  Built stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (no library source is
// linked); tests/test_view_points_cpu.py writes the call to a file, runs this and compares with the numpy restatement.
//   vp_main <in> <out>
//   in:  int32 n_points n_views n_items has_table; int32 mode[nv] n_levels[nv] q[nv] view_ptr[nv + 1] item_point[n];
//        double points[3 np] (normals[3 np] max[np] min[np] if has_table) poses[7 nv] cam[4 nv] bf[nv] bounds[4 nv]
//        log_scale[nv] cos_limit[nv]
//   out: uint8 code[n]; int32 level[n] n_accepted[nv]; double z[n] uv[2 n] dist[n] view_cos[n] ur[n] track_depth[n] median[nv]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "view_points.h"

using namespace movba;

namespace {

template <typename T> std::vector<T> rd(std::FILE *f, size_t count)
{
    std::vector<T> a(count);
    if (count && std::fread(a.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "vp_main: short input\n"); std::exit(2); }
    return a;
}

template <typename T> void wr(std::FILE *f, const std::vector<T> &a)
{
    if (!a.empty() && std::fwrite(a.data(), sizeof(T), a.size(), f) != a.size()) { std::fprintf(stderr, "vp_main: short output\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: vp_main <in> <out>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 4);
    const size_t np = (size_t)hd[0], nv = (size_t)hd[1], n = (size_t)hd[2];
    const bool table = hd[3] != 0;
    const auto mode = rd<int32_t>(f, nv), n_levels = rd<int32_t>(f, nv), q = rd<int32_t>(f, nv), view_ptr = rd<int32_t>(f, nv + 1),
               item_point = rd<int32_t>(f, n);
    const auto points = rd<double>(f, 3 * np);
    const auto normals = rd<double>(f, table ? 3 * np : 0), dmax = rd<double>(f, table ? np : 0), dmin = rd<double>(f, table ? np : 0);
    const auto poses = rd<double>(f, 7 * nv), cam = rd<double>(f, 4 * nv), bf = rd<double>(f, nv), bounds = rd<double>(f, 4 * nv),
               log_scale = rd<double>(f, nv), cos_limit = rd<double>(f, nv);
    std::fclose(f);

    std::vector<uint8_t> code(n);
    std::vector<int32_t> level(n), n_accepted(nv);
    std::vector<double> z(n), uv(2 * n), dist(n), view_cos(n), ur(n), track_depth(n), median(nv);
    for (size_t v = 0; v < nv; ++v) {
        VpView w{};
        w.mode = mode[v]; w.n_levels = n_levels[v]; w.q = q[v]; w.n = view_ptr[v + 1] - view_ptr[v]; w.item0 = view_ptr[v];
        for (int e = 0; e < 7; ++e) w.pose[e] = poses[7 * v + e];
        for (int e = 0; e < 4; ++e) { w.cam[e] = cam[4 * v + e]; w.bounds[e] = bounds[4 * v + e]; }
        w.bf = bf[v]; w.log_scale = log_scale[v]; w.cos_limit = cos_limit[v];
        double view[kVpViewDoubles];
        vp_view(w, view);
        std::vector<uint64_t> keys;
        int32_t acc = 0;
        for (size_t i = (size_t)view_ptr[v]; i < (size_t)view_ptr[v + 1]; ++i) {
            const size_t p = (size_t)item_point[i];
            const double zero[3] = { 0.0, 0.0, 0.0 };
            const bool full = w.mode != MOVBA_VIEW_DEPTH;
            const VpItem r = vp_item(w.mode, w.n_levels, view, &points[3 * p], full ? &normals[3 * p] : zero, full ? dmax[p] : 0.0, full ? dmin[p] : 0.0);
            code[i] = r.code; level[i] = r.level; z[i] = r.z; uv[2 * i] = r.u; uv[2 * i + 1] = r.v; dist[i] = r.dist;
            view_cos[i] = r.view_cos; ur[i] = r.ur; track_depth[i] = r.track_depth;
            acc += r.code < MOVBA_VP_REJ_BEHIND;
            if (!full) keys.push_back(im_order_key(r.z));
        }
        n_accepted[v] = acc;
        median[v] = w.mode != MOVBA_VIEW_DEPTH ? __builtin_nan("") :
                    keys.empty() ? -1.0 : vp_key_value(vp_select_serial(keys.data(), (int64_t)keys.size(), (int64_t)(keys.size() - 1) / w.q));
    }

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    wr(o, code); wr(o, level); wr(o, n_accepted); wr(o, z); wr(o, uv); wr(o, dist); wr(o, view_cos); wr(o, ur); wr(o, track_depth); wr(o, median);
    std::fclose(o);
    std::printf("vp_main: ok\n");
    return 0;
}
