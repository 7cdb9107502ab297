// The refit of movba_two_view_lo (stage 2b, include/movba.h) on the CPU: the library's own arithmetic (two_view_math.h: tv_lo_*,
// the code k_tv_lo inlines) with the matches summed serially by one thread.  tests/test_two_view_lo_cpu.py builds this file
// with the host compiler against the stand-in runtime header of tests/hipstub - plainly, and under AddressSanitizer +
// UndefinedBehaviorSanitizer - and compares what it prints with the numpy restatement.
//   lo_main <file>     file: int32 n, lo_iters | double fx fy cx cy threshold | E0[9] | obs1[2 n] | obs2[2 n]
//   prints             E <9 values>, L <the trace L_0 ...>, kept <k>, steps <s>, inliers0 <matches within the threshold of E0>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "two_view_math.h"

using namespace movba;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[2];
    double par[5], E0[9];
    if (std::fread(hd, 4, 2, f) != 2 || std::fread(par, 8, 5, f) != 5 || std::fread(E0, 8, 9, f) != 9) return 2;
    const int n = hd[0], lo_iters = hd[1];
    if (n < 0 || lo_iters < 0 || lo_iters > MOVBA_MAX_TWO_VIEW_LO_ITERS) return 2;
    std::vector<double> o1(2 * (size_t)n), o2(2 * (size_t)n);
    if (std::fread(o1.data(), 8, o1.size(), f) != o1.size() || std::fread(o2.data(), 8, o2.size(), f) != o2.size()) return 2;
    std::fclose(f);
    const double fm = 0.5 * (par[0] + par[1]), cx = par[2], cy = par[3], thr2 = par[4] * par[4], inv_f = 1.0 / fm;
    const Magsac ms(thr2);
    TvLoState st;
    TvLoTrack tr;
    tv_lo_begin(E0, st, tr);
    int inliers0 = 0;
    for (int i = 0; i < n; ++i)
        inliers0 += fm * fm * tv_sampson2(E0, (o1[2 * i] - cx) * inv_f, (o1[2 * i + 1] - cy) * inv_f, (o2[2 * i] - cx) * inv_f,
                                          (o2[2 * i + 1] - cy) * inv_f) <= thr2;
    std::vector<double> trace;
    for (int k = 0; k <= lo_iters; ++k) {
        double acc[kTvLoAcc] = { 0.0 };
        for (int i = 0; i < n; ++i)
            tv_lo_accumulate(ms, thr2, st.E, st.dE, k < lo_iters, fm, (o1[2 * i] - cx) * inv_f, (o1[2 * i + 1] - cy) * inv_f,
                             (o2[2 * i] - cx) * inv_f, (o2[2 * i + 1] - cy) * inv_f, acc);
        trace.push_back(acc[20]);
        if (!tv_lo_advance(st, tr, acc, k, lo_iters)) break;
    }
    double E[9];
    tv_lo_result(tr, E);
    std::printf("E");
    for (int e = 0; e < 9; ++e) std::printf(" %.17g", E[e]);
    std::printf("\nL");
    for (double l : trace) std::printf(" %.17g", l);
    std::printf("\nkept %d\nsteps %d\ninliers0 %d\n", tr.kept, tr.steps, inliers0);
    return 0;
}
