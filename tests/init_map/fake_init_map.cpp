// The fake device's side of movba_init_map (mov-slam_amd/csrc/init_map.cpp): the launch wrapper of init_map.h as a closure on the
// fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It does not optimise: for every pair it compacts the used matches
// as k_init_map does, evaluates the robust cost of the START estimate with the library's own per-point arithmetic (init_map.h),
// finds the median depth by counting ranks and applies the outcome test and the rescaling - what the kernel returns for
// max_iters == 0 - reading every input through the pointers the host laid out, touching both ends of every scratch array it
// was given and writing results where the host said, so that the sanitizers see the host's layout and hand-offs and the driver
// can check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>

#include "init_map.h"
#include "movba.h"

namespace {
std::atomic<int> g_im_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_init_map: %s\n", what);
    g_im_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_init_map_errors() { return g_im_errors.load(); }

namespace movba {

static void fake_pair(const ImDev &d, int pi)
{
    const ImPair p = d.pairs[pi];
    if (p.n == 0) return;
    const size_t m0 = (size_t)p.m0, cap = (size_t)p.cap;
    const uint8_t *use = d.use + m0;
    int32_t *idx = d.idx + p.s0;
    double *X = d.X + 3 * p.s0, *Xbk = d.Xbk + 3 * p.s0, *lin = d.lin + (size_t)kImLin * p.s0;
    int nu = 0;
    for (int i = 0; i < p.n; ++i)
        if (use[i]) {
            if (nu >= p.cap) { bad("more used matches than the host counted"); return; }
            idx[nu++] = i;
        }
    if (nu != p.cap || nu == 0) { bad("used matches and the host's count disagree"); return; }
    // (both ends of the scratch arrays the kernel would use)
    Xbk[0] = 0.0; Xbk[3 * cap - 1] = 0.0; lin[0] = 0.0; lin[(size_t)kImLin * cap - 1] = 0.0;
    // the start pose, normalised as the kernel does
    double q[7];
    for (int e = 0; e < 7; ++e) q[e] = p.pose2[e];
    const double s = q[3] < 0.0 ? -1.0 : 1.0, nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int e = 0; e < 4; ++e) q[e] = s * q[e] / nq;
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double R[9] = { 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                          2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) };
    const double cam[4] = { p.fx, p.fy, p.cx, p.cy };
    double cost = 0.0;
    for (int k = 0; k < nu; ++k) {
        const size_t m = m0 + (size_t)idx[k];
        const double v[3] = { d.pts[3 * m], d.pts[3 * m + 1], d.pts[3 * m + 2] };
        X[k] = v[0]; X[cap + k] = v[1]; X[2 * cap + k] = v[2];
        double c2[2];
        cost += im_cost(R, q + 4, cam, p.huber, v, d.obs1 + 2 * m, d.obs2 + 2 * m, d.sig1[m], d.sig2[m], c2);
        if (p.chi2) { p.chi2[2 * (size_t)idx[k]] = c2[0]; p.chi2[2 * (size_t)idx[k] + 1] = c2[1]; }
    }
    const int kmed = (nu - 1) / 2;
    double med = 0.0;
    for (int k = 0; k < nu; ++k) {
        const uint64_t mine = im_order_key(X[2 * cap + k]);
        int rank = 0;
        for (int j = 0; j < nu; ++j) {
            const uint64_t o = im_order_key(X[2 * cap + j]);
            rank += o < mine || (o == mine && j < k);
        }
        if (rank == kmed) med = X[2 * cap + k];
    }
    const int outcome = med < 0.0 ? MOVBA_IM_NEG_DEPTH : (nu < p.min_tracked ? MOVBA_IM_FEW_TRACKED : MOVBA_IM_OK);
    const double inv = outcome == MOVBA_IM_OK ? 1.0 / med : 1.0, nan = __builtin_nan("");
    for (int k = 0; k < nu; ++k)
        for (int c = 0; c < 3; ++c) p.points[3 * (size_t)idx[k] + c] = X[c * cap + k] * inv;
    for (int i = 0; i < p.n; ++i)
        if (!use[i]) {
            for (int c = 0; c < 3; ++c) p.points[3 * (size_t)i + c] = nan;
            if (p.chi2) { p.chi2[2 * (size_t)i] = nan; p.chi2[2 * (size_t)i + 1] = nan; }
        }
    double *o = p.out;
    for (int e = 0; e < kImOutDoubles; ++e) o[e] = 0.0;
    for (int e = 0; e < 4; ++e) o[e] = q[e];
    for (int e = 4; e < 7; ++e) o[e] = q[e] * inv;
    o[7] = med; o[8] = outcome; o[9] = nu; o[15] = cost; o[16] = cost;
    if (p.trace) { p.trace[0] = 0.0; p.trace[kImTraceDoubles - 1] = 0.0; }
}

hipError_t launch_init_map(const ImDev &dev, hipStream_t s)
{
    const ImDev d = dev;
    fake_enqueue(s, [=] {
        int64_t at = 0;
        for (int p = 0; p < d.n_pairs; ++p) {
            if (d.pairs[p].s0 != at) { bad("scratch offsets do not follow the pairs"); return; }
            at += d.pairs[p].cap;
            fake_pair(d, p);
        }
    });
    return hipSuccess;
}

}  // namespace movba
