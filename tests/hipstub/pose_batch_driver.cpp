// Drives movba_pose_opt_batch's HOST side (mov-slam_amd/csrc/pose_opt.cpp) against the fake device of this directory
// (fake_device.cpp, fake_pose_batch.cpp), under AddressSanitizer + UndefinedBehaviorSanitizer or ThreadSanitizer: batches of
// mixed frame sizes (frames beyond the LDS limit, frames with fewer than 4 matches, batches that make the staging buffer and
// the pose arena grow between calls), invalid calls, a batch between an LBA upload and its run, and two threads on two
// handles.  Exit code 0 and the last line "POSE-BATCH OK" = every check held.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "movba.h"

extern "C" int fake_pose_batch_errors();

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #c); __atomic_add_fetch(&fails, 1, __ATOMIC_RELAXED); } } while (0)

struct Frame {
    std::vector<double> X, o, isig, chi2;
    std::vector<uint8_t> outl;
    movba_pose_desc d{};
    movba_pose_result r{};
};

void make_frame(Frame &f, int n, unsigned seed, int n_hyp, bool with_isig)
{
    std::mt19937 rng(seed);
    f.X.resize(3 * (size_t)n); f.o.resize(2 * (size_t)n); f.isig.assign(n, 1.0);
    for (int i = 0; i < n; ++i) {
        f.X[3 * i] = (double)(rng() % 100) * 0.01; f.X[3 * i + 1] = (double)(rng() % 100) * 0.01; f.X[3 * i + 2] = 5.0 + i;
        f.o[2 * i] = (double)(rng() % 640); f.o[2 * i + 1] = (double)(rng() % 480);
        f.isig[i] = 1.0 + (double)(rng() % 4);
    }
    f.chi2.assign(n, -7.0); f.outl.assign(n, 9);
    f.d = movba_pose_desc{};
    f.d.n = n; f.d.Xw = n ? f.X.data() : nullptr; f.d.obs = n ? f.o.data() : nullptr; f.d.inv_sigma2 = with_isig ? f.isig.data() : nullptr;
    f.d.fx = f.d.fy = 320; f.d.cx = 320; f.d.cy = 240;
    for (int k = 0; k < 7; ++k) f.d.pose0[k] = 0.01 * (seed % 97) + k;
    f.d.huber_delta = 2.2; f.d.chi2_gate = 5.0; f.d.rounds = 4; f.d.its_per_round = 10;
    f.d.ransac_iters = n_hyp; f.d.ransac_seed = seed; f.d.confidence = n_hyp ? 0.95 : 0.0; f.d.lo_iters = n_hyp ? 10 : 0;
    f.r = movba_pose_result{};
    f.r.outlier = n ? f.outl.data() : nullptr; f.r.chi2 = n ? f.chi2.data() : nullptr;
}

// one batch of frames; every result checked against what the fake device writes for the frame's own inputs
void run_batch(movba_handle *h, std::vector<Frame> &fs)
{
    const int n = (int)fs.size();
    std::vector<movba_pose_desc> d(n);
    std::vector<movba_pose_result> r(n);
    for (int k = 0; k < n; ++k) { d[k] = fs[k].d; r[k] = fs[k].r; r[k].status = 99; }
    EXPECT(movba_pose_opt_batch(h, d.data(), r.data(), n) == MOVBA_OK);
    for (int k = 0; k < n; ++k) {
        const Frame &f = fs[k];
        const int m = f.d.n;
        bool pose_ok = true;
        for (int q = 0; q < 7; ++q) pose_ok &= r[k].pose[q] == f.d.pose0[q] && r[k].ransac_pose[q] == f.d.pose0[q];
        EXPECT(pose_ok);
        if (m < 4) {
            EXPECT(r[k].status == MOVBA_EMPTY && r[k].n_inliers == 0 && r[k].lm_iters == 0);
            bool untouched = true;
            for (int i = 0; i < m; ++i) untouched &= f.chi2[i] == -7.0 && f.outl[i] == 9;
            EXPECT(untouched);
            continue;
        }
        const int n_hyp = f.d.ransac_iters;
        EXPECT(r[k].status == MOVBA_OK && r[k].n_inliers == m && r[k].lm_iters == f.d.rounds * f.d.its_per_round);
        EXPECT(r[k].ransac_inliers == (n_hyp ? m : 0) && r[k].ransac_samples_used == n_hyp && r[k].lo_inliers == (n_hyp ? m : 0));
        bool arr_ok = true;
        for (int i = 0; i < m; ++i) {
            const double is = f.d.inv_sigma2 ? f.isig[i] : 1.0;
            arr_ok &= f.chi2[i] == f.o[2 * i] + is && f.outl[i] == (uint8_t)(i % 3 == 0);
        }
        EXPECT(arr_ok);
    }
}

void mixed_batches(movba_handle *h, unsigned seed)
{
    // small first, then the staging buffer and the arena grow twice, then small again
    const int sizes[3][8] = { { 4, 50, 3, 120, 0, 60, 8, 30 }, { 500, 1200, 4000, 2, 50, 3500, 700, 4 }, { 5000, 6000, 20, 1, 3100, 40, 900, 2000 } };
    for (int round = 0; round < 4; ++round) {
        const int *sz = sizes[round % 3];
        std::vector<Frame> fs(8);
        for (int k = 0; k < 8; ++k) make_frame(fs[k], sz[k], seed + 31 * round + k, (k % 3 == 0) ? 0 : 10 + 20 * (k % 2), k % 2 == 0);
        run_batch(h, fs);
    }
}

// an LBA window uploaded, then a batch of poses on the same handle, then the window's run: the window's arrays leave the staging
// buffer before the batch overwrites it, and the window's results are still downloaded after the batch
void lba_with_batches(movba_handle *h, int reps, unsigned seed)
{
    const int NP = 12, P = 800;
    std::vector<double> poses(7 * NP, 0.0), points(3 * P, 1.0), obs, isig;
    std::vector<uint8_t> fixed(NP, 0);
    std::vector<int32_t> ep, el;
    for (int i = 0; i < NP; ++i) { poses[7 * i + 3] = 1.0; poses[7 * i + 4] = 0.3 * i; fixed[i] = i < 2; }
    std::mt19937 rng(9);
    for (int l = 0; l < P; ++l) {
        const int run = 2 + (int)(rng() % 4), first = (int)(rng() % (unsigned)(NP - run + 1));
        for (int k = first; k < first + run; ++k) { ep.push_back(k); el.push_back(l); }
    }
    const size_t E = ep.size();
    obs.assign(2 * E, 100.0); isig.assign(E, 1.0);
    movba_lba_desc w{};
    w.n_poses = NP; w.n_points = P; w.n_edges = (int32_t)E;
    w.poses = poses.data(); w.pose_fixed = fixed.data(); w.points = points.data();
    w.edge_pose = ep.data(); w.edge_point = el.data(); w.obs = obs.data(); w.inv_sigma2 = isig.data();
    w.fx = w.fy = 320; w.cx = 320; w.cy = 240; w.huber_delta = 2.236; w.chi2_gate = 5.0; w.max_iters = 10; w.flags = MOVBA_FLAG_STALE_ERROR_QUIRK;
    std::vector<double> op(7 * NP, 0.0), opt(3 * P, 0.0), oc(E, 0.0);
    std::vector<uint8_t> oo(E, 9);
    movba_lba_result res{};
    res.poses = op.data(); res.points = opt.data(); res.chi2 = oc.data(); res.outlier = oo.data();
    for (int rep = 0; rep < reps; ++rep) {
        EXPECT(movba_lba_upload(h, &w) == MOVBA_OK);
        std::vector<Frame> fs(6);
        for (int k = 0; k < 6; ++k) make_frame(fs[k], 300 + 900 * k, seed + 6 * rep + k, k % 2 ? 50 : 0, true);
        run_batch(h, fs);
        EXPECT(movba_lba_run(h) == MOVBA_OK);
        EXPECT(movba_lba_download(h, &res) == MOVBA_OK);
        EXPECT(res.n_solves == 10 && op[3] == 1.0 && opt[0] == 1.0 && oo[0] == 0 && oc[0] == 1.0);
    }
}

}  // namespace

int main()
{
    // ---- 1. mixed frame sizes on one handle; invalid calls write nothing but status ----
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        mixed_batches(h, 11u);
        std::vector<Frame> fs(3);
        for (int k = 0; k < 3; ++k) make_frame(fs[k], 40 + k, 5u + k, 0, true);
        movba_pose_desc d[3] = { fs[0].d, fs[1].d, fs[2].d };
        movba_pose_result r[3] = { fs[0].r, fs[1].r, fs[2].r };
        d[1].rounds = 0;
        EXPECT(movba_pose_opt_batch(h, d, r, 3) == MOVBA_ERR_ARG);
        EXPECT(r[0].status == MOVBA_ERR_ARG && r[2].status == MOVBA_ERR_ARG && fs[0].chi2[0] == -7.0 && fs[2].outl[0] == 9);
        d[1].rounds = 4; d[2].Xw = nullptr;
        EXPECT(movba_pose_opt_batch(h, d, r, 3) == MOVBA_ERR_ARG);
        d[2].Xw = fs[2].X.data();
        EXPECT(movba_pose_opt_batch(h, d, r, -1) == MOVBA_ERR_ARG);
        EXPECT(movba_pose_opt_batch(h, d, r, MOVBA_MAX_POSE_BATCH + 1) == MOVBA_ERR_ARG);
        EXPECT(movba_pose_opt_batch(h, nullptr, r, 3) == MOVBA_ERR_ARG);
        EXPECT(movba_pose_opt_batch(h, d, nullptr, 3) == MOVBA_ERR_ARG);
        EXPECT(movba_pose_opt_batch(nullptr, d, r, 3) == MOVBA_ERR_ARG);
        EXPECT(movba_pose_opt_batch(h, nullptr, nullptr, 0) == MOVBA_OK);
        EXPECT(fs[1].chi2[0] == -7.0);
        run_batch(h, fs);
        movba_destroy(h);
    }
    // ---- 2. a batch between an LBA upload and its run ----
    {
        movba_handle *h = nullptr;
        EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
        lba_with_batches(h, 3, 70u);
        movba_destroy(h);
    }
    // ---- 3. two threads, a handle each: pose batches on one, LBA solves with batches between upload and run on the other ----
    {
        auto poses_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            for (int it = 0; it < 3; ++it) mixed_batches(h, seed + 100 * it);
            movba_destroy(h);
        };
        auto lba_thread = [](unsigned seed) {
            movba_handle *h = nullptr;
            EXPECT(movba_create(&h, 0, nullptr, nullptr) == MOVBA_OK);
            lba_with_batches(h, 4, seed);
            movba_destroy(h);
        };
        std::thread a(poses_thread, 300u), b(lba_thread, 700u);
        a.join(); b.join();
    }
    EXPECT(fake_pose_batch_errors() == 0);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("POSE-BATCH OK\n");
    return 0;
}
