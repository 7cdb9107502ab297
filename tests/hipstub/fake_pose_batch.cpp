// The fake device's side of movba_pose_opt_batch (mov-slam_amd/csrc/pose_opt.cpp): the two batched launch wrappers of
// pose_kernels.h as closures on the fake stream (fake_hip.cpp).  They read EVERY byte each frame's PoseDev points to and write
// its whole result record, so that the sanitizers see the host's layout and hand-offs; what they write is a function of the
// frame's own inputs (pose0 echoed, chi2 from the observations, flags from the index), so a driver can tell whether each
// frame's results came back to the right place.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>

#include "pose_kernels.h"

namespace {
std::atomic<long> g_pose_sink{0};
std::atomic<int> g_pose_errors{0};

long sum_all(const void *p, size_t n)
{
    const unsigned char *c = static_cast<const unsigned char *>(p);
    long s = 0;
    for (size_t k = 0; k < n; ++k) s += c[k];
    return s;
}

void bad(const char *what)
{
    std::fprintf(stderr, "fake_pose_batch: %s\n", what);
    g_pose_errors.fetch_add(1);
}
}  // namespace

// layout or hand-off errors the fake device saw (the driver fails on any)
extern "C" int fake_pose_batch_errors() { return g_pose_errors.load(); }

namespace movba {

hipError_t launch_pose_hyp_batch(const PoseDev *frames, const int32_t *hyp_first, int n_frames, int n_blocks, hipStream_t s)
{
    fake_enqueue(s, [=] {
        if (hyp_first[0] != 0 || hyp_first[n_frames] != n_blocks) bad("hypothesis grid: prefix does not span the grid");
        for (int f = 0; f < n_frames; ++f) {
            const PoseDev &p = frames[f];
            if (hyp_first[f + 1] - hyp_first[f] != p.n_hyp) bad("hypothesis grid: a frame's range is not its n_hyp");
            if (p.n_hyp == 0) continue;
            if (!p.hyp_done || !p.cand) bad("hypothesis grid: frame without its tables");
            long cs = sum_all(p.Xw, 24 * (size_t)p.n) + sum_all(p.obs, 16 * (size_t)p.n) + sum_all(p.isig, 8 * (size_t)p.n);
            for (int k = 0; k < 3 * p.n_hyp; ++k)
                if (p.samples[k] < 0 || p.samples[k] >= p.n) bad("hypothesis grid: sample index out of range");
            cs += sum_all(p.samples, 12 * (size_t)p.n_hyp);
            unsigned char *c = reinterpret_cast<unsigned char *>(p.cand);
            const size_t nb = pose_ransac_bytes(p.n_hyp);
            for (size_t k = 0; k < nb; ++k) c[k] = (unsigned char)(f + k);
            g_pose_sink += cs;
        }
    });
    return hipSuccess;
}

hipError_t launch_pose_opt_batch(const PoseDev *frames, int n_frames, bool staged, size_t lds_bytes, hipStream_t s)
{
    fake_enqueue(s, [=] {
        for (int f = 0; f < n_frames; ++f) {
            const PoseDev &p = frames[f];
            if (staged != (pose_opt_staged_lds_bytes(p.n, 0) <= 144 * 1024)) bad("frame in the wrong LM launch");
            if (staged && pose_opt_staged_lds_bytes(p.n, 0) > lds_bytes) bad("staged launch: LDS below a frame's need");
            long cs = sum_all(p.Xw, 24 * (size_t)p.n) + sum_all(p.obs, 16 * (size_t)p.n) + sum_all(p.isig, 8 * (size_t)p.n);
            if (p.n_hyp > 0) cs += sum_all(p.cand, pose_ransac_bytes(p.n_hyp));
            g_pose_sink += cs;
            for (int k = 0; k < 7; ++k) { p.pose_out[k] = p.pose0[k]; p.pose_out[9 + k] = p.pose0[k]; }
            p.pose_out[7] = p.n; p.pose_out[8] = p.n_hyp > 0 ? p.n : 0; p.pose_out[16] = p.rounds * p.its;
            p.pose_out[17] = p.n_hyp; p.pose_out[18] = p.lo_its > 0 ? 1 : 0; p.pose_out[19] = p.n;
            for (int k = 20; k < 24; ++k) p.pose_out[k] = 0.0;
            for (int i = 0; i < p.n; ++i) { p.chi2[i] = p.obs[2 * i] + p.isig[i]; p.level1[i] = (uint8_t)(i % 3 == 0); }
        }
    });
    return hipSuccess;
}

}  // namespace movba
