// The Levenberg step rule of mov-slam_amd/csrc/lm_rule.h on the CPU, over the stand-in runtime header of tests/hipstub.
// tests/test_lm_rule_cpu.py builds this file with the host compiler under the sanitizers and runs it.
//   lm_rule_main hand          the hand cases: prints `hand ok`, or the first case that fails and exits 1
//   lm_rule_main <file>        replays a recorded run.  file: one trial per line, `lambda rho F1` (F1 `nan`: not recorded).
//                              The carried nu starts at 2.  Prints per trial: `trial <accept> <lambda behind it> <nu behind it>`
//                              with 17 significant digits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "lm_rule.h"

using namespace movba;

#define EXPECT(c) do { if (!(c)) { std::printf("hand case failed, line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int hand()
{
    const double inf = std::numeric_limits<double>::infinity();
    EXPECT(kLmTau == 1e-5 && kLmScaleEps == 1e-3 && lm_lambda_init(4.0) == 4e-5);
    // a solve that succeeded: rho = (F0 - F1) / (scale + 1e-3)
    LmGain g = lm_gain(10.0, 4.0, 2.999, true);
    EXPECT(g.F1 == 4.0 && g.rho == 6.0 / (2.999 + 1e-3));
    // a failed solve with a finite F0: F1 is booked as DBL_MAX, the scale as 0 + 1e-3, rho < 0, rejected
    g = lm_gain(10.0, 4.0, 123.0, false);
    EXPECT(g.F1 == DBL_MAX && g.rho == (10.0 - DBL_MAX) / 1e-3 && g.rho < 0.0 && !lm_accept(g.rho, g.F1));
    // a failed solve with F0 = inf: rho = +inf, accepted
    g = lm_gain(inf, 4.0, 123.0, false);
    EXPECT(g.F1 == DBL_MAX && g.rho == inf && lm_accept(g.rho, g.F1));
    // a cost that is not finite is never accepted, nor is rho = nan
    EXPECT(!lm_accept(1.0, inf) && !lm_accept(1.0, std::nan("")) && !lm_accept(std::nan(""), 1.0) && lm_accept(1e-300, 0.0));
    // rho == 0: rejected, and the optimisation terminates; rho < 0 asks for another trial instead
    EXPECT(!lm_accept(0.0, 1.0) && lm_terminate(0.0, 1, 10, true) && !lm_more_trials(0.0, 1, 10, true));
    EXPECT(!lm_terminate(-1.0, 1, 10, true) && lm_more_trials(-1.0, 1, 10, true) && !lm_terminate(0.5, 1, 10, true));
    // lambda = 1e308 with nu = 4: the product is not finite, lambda_ok false, no further trial, terminates
    double lambda = 1e308, nu = 4.0;
    const bool ok = lm_update(false, -1.0, lambda, nu);
    EXPECT(!ok && lambda == inf && nu == 8.0 && !lm_more_trials(-1.0, 1, 10, ok) && lm_terminate(-1.0, 1, 10, ok));
    // qmax == max_trials: no further trial, terminates
    EXPECT(!lm_more_trials(-1.0, 10, 10, true) && lm_terminate(-1.0, 10, 10, true) && lm_more_trials(-1.0, 9, 10, true));
    // nu runs 2, 4, 8 over rejections and returns to 2 on an acceptance; lambda is multiplied by each in turn
    lambda = 1.0; nu = 2.0;
    EXPECT(lm_update(false, -1.0, lambda, nu) && lambda == 2.0 && nu == 4.0);
    EXPECT(lm_update(false, -1.0, lambda, nu) && lambda == 8.0 && nu == 8.0);
    EXPECT(lm_update(false, -1.0, lambda, nu) && lambda == 64.0 && nu == 16.0);
    EXPECT(lm_update(true, 0.5, lambda, nu) && lambda == 64.0 * (2.0 / 3.0) && nu == 2.0);     // 1 - 0^3 = 1, held to 2/3
    EXPECT(lm_update(true, 1.5, lambda, nu) && lambda == 64.0 * (2.0 / 3.0) * (1.0 / 3.0) && nu == 2.0);   // 1 - 2^3 < 1/3
    lambda = 1.0;
    const double t = 2.0 * 0.9 - 1.0;
    EXPECT(lm_update(true, 0.9, lambda, nu) && lambda == 1.0 - t * t * t && lambda > 0.48 && lambda < 0.49);   // inside: the cube itself
    std::printf("hand ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    if (!std::strcmp(argv[1], "hand")) return hand();
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    double lambda, rho, F1, nu = 2.0;
    while (std::fscanf(f, "%lf %lf %lf", &lambda, &rho, &F1) == 3) {
        const bool accept = lm_accept(rho, F1 != F1 ? 0.0 : F1);
        lm_update(accept, rho, lambda, nu);
        std::printf("trial %d %.17g %.17g\n", accept ? 1 : 0, lambda, nu);
    }
    std::fclose(f);
    return 0;
}
