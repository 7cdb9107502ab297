// Marginal covariances of a solved window (movba_lba_marginals: marginals.cpp, kernels in marginals.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace movba {

// Device view of one marginals call.  `w` is the window's own view with its controller replaced by `ctrl`, a scratch copy of the
// run's controller (lambda = damping, done = 0): the linearisation, schur and factorisation kernels of the LM run through it
// unchanged and leave the run's own controller, state and results alone.
struct MargDev {
    DevWindow w;
    const Ctrl *run_ctrl;       // the run's controller (copied into ctrl by k_marg_ctrl)
    Ctrl *ctrl;
    double damping;
    double *linv;               // ntile x NB x NB: inverses of the diagonal factor tiles L(I, I)^-1
    double *W;                  // L^-1, lower block triangle in the factor's tile layout (tile_off(I, J), I >= J, I < ntile)
    double *sig;                // S^-1 = W^T W, the same layout
    int32_t *flags;             // [0] the factorisation met a non-positive pivot, [1] a point block Hll + damping I is not positive definite
    double *pose_out;           // NP x 36, caller order (NaN for keyframes outside the system; the host zeroes the fixed ones)
    double *point_out;          // P x 9
    int32_t want_points, pose_blocks;   // point blocks wanted; workgroups of k_marg_out that gather the pose blocks
};

// the device pass: scratch controller, linearisation at the final state, S and its factor, W, sigma, pose and point blocks
hipError_t launch_marginals(const MargDev &m, hipStream_t s);

}  // namespace movba
