// movba_pose_opt_batch (include/movba.h): movba_pose_opt on many frames in one set of launches — several Tracking sessions
// on one GPU.  Every frame gets its own inputs, result record, outlier flags and hypothesis tables, laid out back to back in
// the handle's staging buffer and pose arena; the kernels are those of movba_pose_opt with the frame taken from blockIdx
// (pose_kernels.hip: k_pose_hyp_b, k_pose_opt_b), so each frame's result is the bits of its solo call.
//
// Kept out of api.cpp: the host-only test builds (tests/hipstub) link api.cpp against a fake device that defines exactly
// the launch wrappers api.cpp calls.
#include <algorithm>
#include <cstring>
#include <vector>

#include "handle.h"
#include "pose_kernels.h"

using namespace movba;

namespace {

bool desc_ok(const movba_pose_desc &d)
{
    return d.n >= 0 && (d.n == 0 || (d.Xw && d.obs)) && d.rounds >= 1 && d.its_per_round >= 1;
}

int frame_hyp(const movba_pose_desc &d) { return d.ransac_iters > 0 ? std::min(d.ransac_iters, (int32_t)MOVBA_MAX_RANSAC_ITERS) : 0; }

// offsets of one frame (n >= 4) in the staging buffer / pose arena
struct FrameLayout {
    int desc;               // index into the caller's arrays
    int n, n_hyp;
    bool staged;            // its matches fit LDS: k_pose_opt_b<true>, results straight into the pinned buffer
    size_t o_X, o_obs, o_is, o_samp, o_chi, o_pose, o_lvl, o_cand;
};

}  // namespace

extern "C" int movba_pose_opt_batch(movba_handle *h, const movba_pose_desc *descs, movba_pose_result *results, int32_t n)
{
    if (!h || n < 0 || n > MOVBA_MAX_POSE_BATCH || (n > 0 && (!descs || !results))) return MOVBA_ERR_ARG;
    // all descriptors are checked before anything is solved; on a non-zero return only `status` is written
    bool ok = true;
    for (int f = 0; f < n; ++f) ok &= desc_ok(descs[f]);
    if (!ok) {
        for (int f = 0; f < n; ++f) results[f].status = MOVBA_ERR_ARG;
        return MOVBA_ERR_ARG;
    }
    if (n == 0) return MOVBA_OK;

    // Layout.  Inputs of every frame, then the device array of PoseDev and the hypothesis grid's prefix (one H2D copy of
    // [0, h2d)); then the results: those of the staged frames (written into the pinned buffer by the kernel), then those of
    // the rest (written into the arena, one D2H copy of [o_unstaged, d2h)); then the candidate tables (arena only).
    // Staged frames come first in the PoseDev array, so each LM launch takes a contiguous range of it.
    std::vector<FrameLayout> fr;
    fr.reserve((size_t)n);
    for (int pass = 0; pass < 2; ++pass)
        for (int f = 0; f < n; ++f) {
            const movba_pose_desc &d = descs[f];
            if (d.n < 4) continue;          // (the reference returns 0 without touching the frame, Optimizer.cc:415-418)
            const bool staged = pose_opt_staged_lds_bytes(d.n, 0) <= 144 * 1024;
            if (staged != (pass == 0)) continue;
            FrameLayout L{};
            L.desc = f; L.n = d.n; L.n_hyp = frame_hyp(d); L.staged = staged;
            fr.push_back(L);
        }
    const int nv = (int)fr.size();
    int ns = 0;
    while (ns < nv && fr[ns].staged) ++ns;

    for (int f = 0; f < n; ++f) results[f].status = MOVBA_ERR_HIP;        // (until the device work is through)
    // fewer than 4 matches: what movba_pose_opt gives such a frame (MOVBA_EMPTY, pose0); the other frames are solved
    auto fill_empty = [&]() {
        for (int f = 0; f < n; ++f) {
            const movba_pose_desc &d = descs[f];
            if (d.n >= 4) continue;
            movba_pose_result &r = results[f];
            for (int k = 0; k < 7; ++k) { r.pose[k] = d.pose0[k]; r.ransac_pose[k] = d.pose0[k]; }
            r.n_inliers = 0; r.ransac_inliers = 0; r.lm_iters = 0; r.ransac_samples_used = 0; r.lo_accepted = 0; r.lo_inliers = 0;
            r.pad_q = 0;
            r.status = MOVBA_EMPTY;
        }
    };
    if (nv == 0) { fill_empty(); return MOVBA_OK; }

    Carver c;
    for (FrameLayout &L : fr) {
        L.o_X = c.take<double>(3 * (size_t)L.n); L.o_obs = c.take<double>(2 * (size_t)L.n); L.o_is = c.take<double>(L.n);
        L.o_samp = c.take<int32_t>(3 * (size_t)L.n_hyp + 1);
    }
    const size_t o_frames = c.take<PoseDev>(nv), o_hypf = c.take<int32_t>((size_t)nv + 1);
    const size_t h2d = c.off;
    size_t o_unstaged = 0;
    for (int k = 0; k < nv; ++k) {
        FrameLayout &L = fr[k];
        if (k == ns) o_unstaged = c.off;
        L.o_chi = c.take<double>(L.n); L.o_pose = c.take<double>(24); L.o_lvl = c.take<uint8_t>(L.n);
    }
    const size_t d2h = c.off;
    for (FrameLayout &L : fr) L.o_cand = L.n_hyp > 0 ? c.take<uint8_t>(pose_ransac_bytes(L.n_hyp) + 16) : 0;
    const size_t total = c.off;

    HIP_TRY(hipSetDevice(h->device));
    if (total > h->pose_cap) {
        if (h->pose_arena) { HIP_TRY(hipStreamSynchronize(h->stream)); HIP_TRY(hipFree(h->pose_arena)); h->pose_arena = nullptr; h->pose_cap = 0; }
        const size_t cap = align_up(2 * total, 1 << 16);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->pose_arena), cap));
        h->pose_cap = cap;
    }
    int rc = ensure_stage(h, d2h); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    // (a window uploaded on this handle and not run yet: its arrays may still be crossing the bus out of the staging buffer)
    HIP_TRY(hipEventSynchronize(h->copy_event));
    h->export_in_run = false;        // (results a run may have left in the staging buffer are overwritten here: download exports again)

    char *sg = h->stage, *ar = h->pose_arena;
    PoseDev *pd = reinterpret_cast<PoseDev *>(sg + o_frames);
    int32_t *hypf = reinterpret_cast<int32_t *>(sg + o_hypf);
    int n_blocks = 0;
    for (int k = 0; k < nv; ++k) {
        const FrameLayout &L = fr[k];
        const movba_pose_desc &d = descs[L.desc];
        std::memcpy(sg + L.o_X, d.Xw, sizeof(double) * 3 * (size_t)L.n);
        std::memcpy(sg + L.o_obs, d.obs, sizeof(double) * 2 * (size_t)L.n);
        double *isg = reinterpret_cast<double *>(sg + L.o_is);
        for (int i = 0; i < L.n; ++i) isg[i] = d.inv_sigma2 ? d.inv_sigma2[i] : 1.0;
        if (L.n_hyp > 0) (void)movba_pose_ransac_samples(L.n, L.n_hyp, d.ransac_seed, reinterpret_cast<int32_t *>(sg + L.o_samp));
        PoseDev p{};
        p.n = L.n; p.rounds = d.rounds; p.its = d.its_per_round; p.n_hyp = L.n_hyp; p.hyp_done = L.n_hyp > 0 ? 1 : 0;
        p.confidence = d.confidence; p.lo_its = L.n_hyp > 0 && d.lo_iters > 0 ? d.lo_iters : 0;
        p.fx = d.fx; p.fy = d.fy; p.cx = d.cx; p.cy = d.cy; p.huber_delta = d.huber_delta; p.chi2_gate = d.chi2_gate;
        for (int q = 0; q < 7; ++q) p.pose0[q] = d.pose0[q];
        char *out = L.staged ? h->stage_dev : ar;
        p.Xw = reinterpret_cast<double *>(ar + L.o_X); p.obs = reinterpret_cast<double *>(ar + L.o_obs); p.isig = reinterpret_cast<double *>(ar + L.o_is);
        p.samples = reinterpret_cast<const int32_t *>(ar + L.o_samp);
        p.chi2 = reinterpret_cast<double *>(out + L.o_chi); p.pose_out = reinterpret_cast<double *>(out + L.o_pose); p.level1 = reinterpret_cast<uint8_t *>(out + L.o_lvl);
        p.cand = L.n_hyp > 0 ? reinterpret_cast<double *>(ar + L.o_cand) : nullptr;
        std::memcpy(static_cast<void *>(pd + k), &p, sizeof(PoseDev));
        hypf[k] = n_blocks;
        n_blocks += L.n_hyp;
    }
    hypf[nv] = n_blocks;
    size_t lds = 0;
    for (int k = 0; k < ns; ++k) lds = std::max(lds, pose_opt_staged_lds_bytes(fr[k].n, 0));

    const PoseDev *frames = reinterpret_cast<const PoseDev *>(ar + o_frames);
    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    if (n_blocks > 0) HIP_TRY(launch_pose_hyp_batch(frames, reinterpret_cast<const int32_t *>(ar + o_hypf), nv, n_blocks, h->stream));
    if (ns > 0) HIP_TRY(launch_pose_opt_batch(frames, ns, true, lds, h->stream));
    if (ns < nv) {
        HIP_TRY(launch_pose_opt_batch(frames + ns, nv - ns, false, 0, h->stream));
        HIP_TRY(hipMemcpyAsync(sg + o_unstaged, ar + o_unstaged, d2h - o_unstaged, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));

    for (const FrameLayout &L : fr) {
        const movba_pose_desc &d = descs[L.desc];
        movba_pose_result &r = results[L.desc];
        const double *po = reinterpret_cast<const double *>(sg + L.o_pose);
        const bool hyp = L.n_hyp > 0;
        for (int k = 0; k < 7; ++k) r.pose[k] = po[k];
        r.n_inliers = (int32_t)po[7];
        r.ransac_inliers = hyp ? (int32_t)po[8] : 0;
        r.lm_iters = (int32_t)po[16];
        r.ransac_samples_used = hyp ? (int32_t)po[17] : 0; r.lo_accepted = hyp ? (int32_t)po[18] : 0; r.lo_inliers = hyp ? (int32_t)po[19] : 0;
        r.pad_q = 0;
        for (int k = 0; k < 7; ++k) r.ransac_pose[k] = hyp ? po[9 + k] : d.pose0[k];
        if (r.outlier) std::memcpy(r.outlier, sg + L.o_lvl, (size_t)L.n);
        if (r.chi2) std::memcpy(r.chi2, sg + L.o_chi, sizeof(double) * (size_t)L.n);
        r.status = MOVBA_OK;
    }
    fill_empty();
    return MOVBA_OK;
}
