// Device view + launch wrapper of movba_two_view and movba_two_view_lo (two_view.hip; host side: two_view.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace movba {

// One frame pair as the kernels read it.  Every pointer is device memory or a device view of pinned host memory.
struct TvPair {
    int32_t n, n_hyp;               // matches; samples (0 for a pair with fewer than 5 matches)
    int32_t m0, h0;                 // first match / first sample of the pair in the call's concatenated arrays
    int32_t min_tri, pad;
    double f, fx, fy, cx, cy;       // f = 0.5 (fx + fy): what stages 1 - 3 normalise with
    double thr2, conf, th2, min_par, max_depth;
    uint8_t *inlier, *good, *code;  // n each, out
    double *points;                 // n x 3 out
    double *out;                    // kTvOutDoubles out
};

struct TvDev {
    int32_t n_pairs, n_hyp_total;
    const TvPair *pairs;
    const int32_t *hyp_first;       // n_pairs + 1: prefix of n_hyp
    const double *obs1, *obs2;      // all pairs' matches x 2
    const int32_t *samples;         // n_hyp_total x 5, every index checked by its generator
    // scratch
    double *cand;                   // n_hyp_total x 10 x 9
    double *loss;                   // n_hyp_total x 10 (infinity: no candidate)
    int32_t *cnt;                   // n_hyp_total x 10
    int32_t *nsol;                  // n_hyp_total
    uint8_t *inl0;                  // all matches
    double *cosv;                   // all matches
    double *rec;                    // n_pairs x kTvRecDoubles
    // movba_two_view_lo: n_pairs x kTvLoDoubles (two_view_math.h), zero-filled by the host and part of its upload; nullptr when
    // neither a refit nor `info` is asked for.  A slot whose mark is set holds the refit's kept E: k_tv_recover goes on with it
    double *lo;
    int32_t lo_iters;               // steps of the refit at most; 0: k_tv_lo is not launched
};

constexpr int kTvThreads = 256;
constexpr int kTvRecDoubles = 32;   // winner E 9, R 9, t 3, n_inliers, n_pass, samples_used, winner index, has_model

// k_tv_hyp, k_tv_lo (lo_iters > 0 only), k_tv_recover, k_tv_check on the stream, in that order
hipError_t launch_two_view(const TvDev &d, hipStream_t s);

}  // namespace movba
