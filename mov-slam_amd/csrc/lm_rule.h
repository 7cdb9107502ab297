// g2o's Levenberg step rule as the three LM loops of the library apply it: decide_body (kernels.hip), lm_round
// (pose_kernels.hip) and k_init_map (init_map.hip).  Plain C++ without builtins: a host build compiles it as it stands, over the
// stand-in runtime header of tests/hipstub (tests/lm_rule/lm_rule_main.cpp; tests/init_map/im_main.cpp runs its whole loop by it).
//
// Where the rule comes from: OptimizationAlgorithmLevenberg::solve and the loop conditions of
// SparseOptimizer::optimize.  lambda starts at tau max |H_jj|; a trial's gain is rho = (F0 - F1) / (sum x (lambda x + b) + 1e-3);
// it is accepted on rho > 0 with a finite F1, and lambda then shrinks by 1 - (2 rho - 1)^3 held to [1/3, 2/3]; a rejected one
// multiplies lambda by nu and doubles nu; trials repeat while rho < 0, up to max_trials; the optimisation ends (Terminate) on
// the last allowed trial, on rho == 0 or on a lambda that is no longer finite.
// The booking of a FAILED solve - F1 = DBL_MAX (finite), scale = 0 + 1e-3, the estimate not moved - follows this repository's
// oracle (the trial loop of its C restatement under oracle/: `if (ok2) ws_update`), not a pinned g2o: g2o applies the stale increment its linear
// solver left behind and computes the scale from it, which gives the same decision only while F0 is finite (reject and pop).
// With F0 = inf (a point on a keyframe's z = 0 plane) rho = (inf - DBL_MAX) / 1e-3 = +inf and the trial counts as ACCEPTED, of
// a state that has not moved.  Later g2o revisions book the failed solve differently again (they gate the acceptance on the
// solve and take scale = 1: VERDICT.md, weak point 4); the reference builds against an unpinned g2o.  A change of that
// booking is a change of lm_gain below and of the oracle, nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace movba {

constexpr double kLmTau = 1e-5;          // computeLambdaInit's tau
constexpr double kLmScaleEps = 1e-3;     // what computeScale's sum is offset by

// lambda of the first trial from the largest |H_jj| over the free pose and point blocks
__host__ __device__ __forceinline__ double lm_lambda_init(double max_abs_diag) { return kLmTau * max_abs_diag; }

// Gain ratio of a trial and the cost it is booked with.  F1, scale: the trial's summed cost and sum x (lambda x + b), which
// a failed solve (solved = false) replaces by DBL_MAX and 0.
struct LmGain { double rho, F1; };
__host__ __device__ __forceinline__ LmGain lm_gain(double F0, double F1, double scale, bool solved)
{
    if (!solved) { F1 = DBL_MAX; scale = 0.0; }
    scale += kLmScaleEps;
    return LmGain{ (F0 - F1) / scale, F1 };
}

__host__ __device__ __forceinline__ bool lm_accept(double rho, double F1) { return rho > 0.0 && std::isfinite(F1); }

// lambda and nu behind a trial; returns lambda_ok = isfinite(lambda)
__host__ __device__ __forceinline__ bool lm_update(bool accepted, double rho, double &lambda, double &nu)
{
    if (accepted) {
        const double t = 2.0 * rho - 1.0;
        double alpha = 1.0 - t * t * t;                // (pow(tmp, 3) in g2o: a library call of ~100 instructions on the device)
        alpha = fmin(alpha, 2.0 / 3.0);
        lambda *= fmax(1.0 / 3.0, alpha);
        nu = 2.0;
    } else {
        lambda *= nu;
        nu *= 2.0;
    }
    return std::isfinite(lambda);
}

// another trial of the same linearisation?  (qmax: trials taken, this one included)
__host__ __device__ __forceinline__ bool lm_more_trials(double rho, int qmax, int max_trials, bool lambda_ok)
{
    return rho < 0.0 && qmax < max_trials && lambda_ok;
}

// Terminate: no further iteration
__host__ __device__ __forceinline__ bool lm_terminate(double rho, int qmax, int max_trials, bool lambda_ok)
{
    return qmax == max_trials || rho == 0.0 || !lambda_ok;
}

}  // namespace movba
