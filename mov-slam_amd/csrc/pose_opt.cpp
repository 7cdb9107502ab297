// Optimizer::PoseOptimization (the reference's src/Optimizer.cc:397-459) behind the C-ABI (include/movba.h):
// movba_pose_opt, one frame per call, and movba_pose_opt_batch, many frames in one set of launches — several Tracking
// sessions on one GPU.  Both check, pack and read a frame with the same helpers below and lay it out in the handle's staging
// buffer and pose scratch; the batch gives every frame its own inputs, result record, outlier flags and hypothesis tables,
// back to back, and runs the solo call's kernels with the frame taken from blockIdx (pose_kernels.hip: k_pose_hyp_b,
// k_pose_opt_b), so each frame's result is the bits of its solo call.
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

// offsets of one frame (n >= 4) in the staging buffer / pose scratch
struct FrameLayout {
    int desc;               // index into the caller's arrays
    int n, n_hyp;
    bool staged;            // its matches fit LDS: k_pose_opt<true>, results straight into the pinned buffer
    size_t o_X, o_obs, o_is, o_samp, o_chi, o_pose, o_lvl, o_cand;
};

FrameLayout frame_layout(const movba_pose_desc &d, int index)
{
    FrameLayout L{};
    L.desc = index; L.n = d.n; L.n_hyp = frame_hyp(d); L.staged = pose_opt_staged_lds_bytes(d.n, 0) <= 144 * 1024;
    return L;
}

// what crosses to the device, and what comes back
void carve_inputs(Carver &c, FrameLayout &L)
{
    L.o_X = c.take<double>(3 * (size_t)L.n); L.o_obs = c.take<double>(2 * (size_t)L.n); L.o_is = c.take<double>(L.n);
    L.o_samp = c.take<int32_t>(3 * (size_t)L.n_hyp + 1);
}
void carve_results(Carver &c, FrameLayout &L)
{
    L.o_chi = c.take<double>(L.n); L.o_pose = c.take<double>(20); L.o_lvl = c.take<uint8_t>(L.n);
}

void pack_inputs(char *sg, const FrameLayout &L, const movba_pose_desc &d)
{
    std::memcpy(sg + L.o_X, d.Xw, sizeof(double) * 3 * (size_t)L.n);
    std::memcpy(sg + L.o_obs, d.obs, sizeof(double) * 2 * (size_t)L.n);
    double *isg = reinterpret_cast<double *>(sg + L.o_is);
    for (int i = 0; i < L.n; ++i) isg[i] = d.inv_sigma2 ? d.inv_sigma2[i] : 1.0;
    if (L.n_hyp > 0) (void)movba_pose_ransac_samples(L.n, L.n_hyp, d.ransac_seed, reinterpret_cast<int32_t *>(sg + L.o_samp));
}

// the device's view of a frame: `in` is where the kernels read the matches, `out` where the LM kernel leaves its results,
// `cand` the hypothesis tables in device memory (or nullptr)
PoseDev pose_dev(const movba_pose_desc &d, const FrameLayout &L, char *in, char *out, char *cand)
{
    PoseDev p{};
    p.n = L.n; p.rounds = d.rounds; p.its = d.its_per_round; p.n_hyp = L.n_hyp; p.hyp_done = 0;
    p.confidence = d.confidence; p.lo_its = L.n_hyp > 0 && d.lo_iters > 0 ? d.lo_iters : 0;
    p.fx = d.fx; p.fy = d.fy; p.cx = d.cx; p.cy = d.cy; p.huber_delta = d.huber_delta; p.chi2_gate = d.chi2_gate;
    for (int k = 0; k < 7; ++k) p.pose0[k] = d.pose0[k];
    p.Xw = reinterpret_cast<double *>(in + L.o_X); p.obs = reinterpret_cast<double *>(in + L.o_obs); p.isig = reinterpret_cast<double *>(in + L.o_is);
    p.samples = reinterpret_cast<const int32_t *>(in + L.o_samp);
    p.chi2 = reinterpret_cast<double *>(out + L.o_chi); p.pose_out = reinterpret_cast<double *>(out + L.o_pose); p.level1 = reinterpret_cast<uint8_t *>(out + L.o_lvl);
    p.cand = reinterpret_cast<double *>(cand);
    return p;
}

void clear_counts(movba_pose_result &r)
{
    r.n_inliers = 0; r.ransac_inliers = 0; r.lm_iters = 0; r.ransac_samples_used = 0; r.lo_accepted = 0; r.lo_inliers = 0; r.pad_q = 0;
}

// a solved frame's result out of the staging buffer: the 20-double record the LM kernel leaves, the flags and the errors
void read_result(const char *sg, const FrameLayout &L, const movba_pose_desc &d, movba_pose_result &r)
{
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

}  // namespace

extern "C" {

// minimal samples of the hypothesis stage: n_hyp triples of distinct match indices from a xorshift32 stream (the same
// function feeds the oracle in the tests, so both sides score the same hypotheses)
int movba_pose_ransac_samples(int32_t n, int32_t n_hyp, uint32_t seed, int32_t *out)
{
    if (n < 3 || n_hyp < 0 || !out) return MOVBA_ERR_ARG;
    uint32_t x = seed ? seed : 0x9E3779B9u;
    auto next = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (int h = 0; h < n_hyp; ++h) {
        int32_t a = (int32_t)(next() % (uint32_t)n), b, c;
        do { b = (int32_t)(next() % (uint32_t)n); } while (b == a);
        do { c = (int32_t)(next() % (uint32_t)n); } while (c == a || c == b);
        out[3 * h] = a; out[3 * h + 1] = b; out[3 * h + 2] = c;
    }
    return MOVBA_OK;
}

int movba_pose_opt(movba_handle *h, const movba_pose_desc *d, movba_pose_result *res)
{
    if (!h || !d || !res) return MOVBA_ERR_ARG;
    res->status = MOVBA_ERR_ARG;
    clear_counts(*res);
    if (!desc_ok(*d)) return MOVBA_ERR_ARG;
    for (int k = 0; k < 7; ++k) res->pose[k] = d->pose0[k];
    // fewer than 4 matches: the reference returns 0 without touching the frame (Optimizer.cc:415-418)
    if (d->n < 4) { res->status = MOVBA_EMPTY; return MOVBA_EMPTY; }
    FrameLayout L = frame_layout(*d, 0);
    Carver c;
    carve_inputs(c, L);
    const size_t h2d = c.off;
    carve_results(c, L);
    const size_t d2h_end = c.off;
    L.o_cand = c.take<uint8_t>(pose_ransac_bytes(L.n_hyp) + 16);
    const size_t total = c.off;
    // The hypothesis stage runs as a grid of its own over the whole chip (k_pose_hyp, one workgroup per sample) on a device
    // copy of the matches; the LM kernel then only picks the best candidate.  The LM keeps the matches in LDS when they fit
    // (staged), reading them once from the device copy (hypothesis stage on) or straight from the pinned buffer (off), and
    // writes its results back into the pinned buffer itself.
    const bool grid_hyp = L.n_hyp > 0, staged = L.staged;
    const bool need_arena = !staged || grid_hyp;
    int rc = begin_side_call(h, need_arena ? total : 0, total); if (rc) return rc;
    char *sg = h->stage, *ar = h->pose_scratch.p;
    pack_inputs(sg, L, *d);
    if (need_arena) HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    PoseDev p = pose_dev(*d, L, need_arena ? ar : h->stage_dev, staged ? h->stage_dev : ar, need_arena ? ar + L.o_cand : nullptr);
    STAMP_HOST(rc = stamp_pose(h, p); if (rc) return rc);
    if (grid_hyp) {
        HIP_TRY(launch_pose_hyp(p, h->stream));
        p.hyp_done = 1;
    }
    HIP_TRY(launch_pose_opt(p, staged, h->stream));
    if (!staged) HIP_TRY(hipMemcpyAsync(sg + L.o_chi, ar + L.o_chi, d2h_end - L.o_chi, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    read_result(sg, L, *d, *res);
    STAMP_HOST(stamp_report_pose(h, res->lm_iters));
    return MOVBA_OK;
}

int movba_pose_opt_batch(movba_handle *h, const movba_pose_desc *descs, movba_pose_result *results, int32_t n)
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
    // the rest (written into the pose scratch, one D2H copy of [o_unstaged, d2h)); then the candidate tables (device only).
    // Staged frames come first in the PoseDev array, so each LM launch takes a contiguous range of it.
    std::vector<FrameLayout> fr;
    fr.reserve((size_t)n);
    for (int pass = 0; pass < 2; ++pass)
        for (int f = 0; f < n; ++f) {
            if (descs[f].n < 4) continue;          // (the reference returns 0 without touching the frame, Optimizer.cc:415-418)
            const FrameLayout L = frame_layout(descs[f], f);
            if (L.staged == (pass == 0)) fr.push_back(L);
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
            clear_counts(r);
            r.status = MOVBA_EMPTY;
        }
    };
    if (nv == 0) { fill_empty(); return MOVBA_OK; }

    Carver c;
    for (FrameLayout &L : fr) carve_inputs(c, L);
    const size_t o_frames = c.take<PoseDev>(nv), o_hypf = c.take<int32_t>((size_t)nv + 1);
    const size_t h2d = c.off;
    size_t o_unstaged = 0;
    for (int k = 0; k < nv; ++k) {
        if (k == ns) o_unstaged = c.off;
        carve_results(c, fr[k]);
    }
    const size_t d2h = c.off;
    for (FrameLayout &L : fr) L.o_cand = L.n_hyp > 0 ? c.take<uint8_t>(pose_ransac_bytes(L.n_hyp) + 16) : 0;
    const size_t total = c.off;

    int rc = begin_side_call(h, total, d2h); if (rc) return rc;
    char *sg = h->stage, *ar = h->pose_scratch.p;
    PoseDev *pd = reinterpret_cast<PoseDev *>(sg + o_frames);
    int32_t *hypf = reinterpret_cast<int32_t *>(sg + o_hypf);
    int n_blocks = 0;
    for (int k = 0; k < nv; ++k) {
        const FrameLayout &L = fr[k];
        const movba_pose_desc &d = descs[L.desc];
        pack_inputs(sg, L, d);
        PoseDev p = pose_dev(d, L, ar, L.staged ? h->stage_dev : ar, L.n_hyp > 0 ? ar + L.o_cand : nullptr);
        p.hyp_done = L.n_hyp > 0 ? 1 : 0;
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

    for (const FrameLayout &L : fr) read_result(sg, L, descs[L.desc], results[L.desc]);
    fill_empty();
    return MOVBA_OK;
}

}  // extern "C"
