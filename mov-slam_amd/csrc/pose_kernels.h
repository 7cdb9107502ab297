// Device view + launch wrapper of the pose-only optimisation kernel (pose_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clock_stamp.h"

namespace movba {

struct PoseDev {
    int32_t n, rounds, its, n_hyp;     // n_hyp > 0: RANSAC / P3P hypothesis stage in front of the LM (samples: n_hyp x 3 match indices)
    int32_t hyp_done, pad;             // the candidates were solved and scored by k_pose_hyp already (tables in `cand`)
    double fx, fy, cx, cy, huber_delta, chi2_gate;
    double pose0[7];
    double confidence;      // stopping rule of the hypothesis stage (<= 0 or >= 1: every sample is eligible)
    int32_t lo_its, pad3;   // local-optimisation step on the winning hypothesis: LM iterations of the refit on its inliers (0: off)
    const double *Xw;       // n x 3
    const double *obs;      // n x 2
    const double *isig;     // n
    double *chi2;           // n out
    uint8_t *level1;        // n out: outlier flags
    double *pose_out;       // 20: pose (7) + inlier count | inliers of the best hypothesis, its pose (7) | LM iterations run | samples the
                            // stopping rule admitted | LO refit kept (0 / 1) | inliers of the LM's start pose
    const int32_t *samples; // n_hyp x 3
    double *cand;           // device scratch for the candidate poses and scores (pose_ransac_bytes); unused when the stage runs staged in k_pose_opt
#ifdef MOVBA_CLOCK_STAMP
    StampBuf stamp;         // diagnostic build only, behind everything the product build has (clock_stamp.h)
#endif
};

// staged: inputs and outputs are device views of pinned host memory, the kernel keeps the matches in LDS
// (pose_opt_staged_lds_bytes(n) must fit the 150 KB granted by configure_pose_kernels())
size_t pose_opt_staged_lds_bytes(int n, int n_hyp);
size_t pose_ransac_bytes(int n_hyp);
hipError_t configure_pose_kernels();
hipError_t launch_pose_hyp(const PoseDev &p, hipStream_t s);      // the hypothesis stage as a grid of its own (inputs in device memory)
hipError_t launch_pose_opt(const PoseDev &p, bool staged, hipStream_t s);
// movba_pose_opt_batch (pose_opt.cpp): the same kernel bodies over n_frames frames of a device array, one workgroup per
// frame (LM: k_pose_opt_b) or per (frame, sample) (hypothesis stage: k_pose_hyp_b, n_blocks = hyp_first[n_frames], the prefix
// sum of the frames' n_hyp).  staged: every frame's staged LDS need is at most lds_bytes <= 144 KB
hipError_t launch_pose_hyp_batch(const PoseDev *frames, const int32_t *hyp_first, int n_frames, int n_blocks, hipStream_t s);
hipError_t launch_pose_opt_batch(const PoseDev *frames, int n_frames, bool staged, size_t lds_bytes, hipStream_t s);

}  // namespace movba
