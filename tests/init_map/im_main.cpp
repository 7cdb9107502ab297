// The bundle adjustment of movba_init_map (stage 2, include/movba.h) on the CPU: the library's own per-point arithmetic
// (init_map.h: im_linearize, im_schur, im_back, im_cost - the code k_init_map inlines - and the step rule of lm_rule.h) with the
// points summed serially by one thread.  What surrounds that arithmetic is this file's own, written for the host: a plain 6 x 6 Cholesky, the quaternion to matrix
// conversion and SE3Quat's exponential as SURVEY A.8 writes it - NOT device_math.h's solve6 and se3_oplus, which the kernel uses
// and which only the GPU tests exercise.  tests/test_init_map_cpu.py builds this file with the host compiler against the
// stand-in runtime header of tests/hipstub and compares what it prints with the oracle.
//   im_main <file>     file: int32 n, max_iters, max_trials, pad | double fx fy cx cy huber | pose2[7] | obs1[2 n] | obs2[2 n] |
//                            points[3 n] | inv_sigma2_1[n] | inv_sigma2_2[n]
//   prints             pose <7>, cost0, cost, lambda, iters <n>, solves <n>, cholfail <n>, then per trial: trial <lambda> <F0> <F1> <rho> <accept>,
//                      then points <3 n>
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "init_map.h"
#include "lm_rule.h"
#include "movba.h"

using namespace movba;

namespace {

void q2R(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

void qnorm(double q[4])
{
    const double s = q[3] < 0.0 ? -1.0 : 1.0, n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int e = 0; e < 4; ++e) q[e] = s * q[e] / n;
}

// T <- exp(u) T, u = (omega, upsilon)
void oplus(const double u[6], const double T[7], double out[7])
{
    const double w[3] = { u[0], u[1], u[2] }, th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
    double b, d;
    if (th < 1e-5) { b = 0.5; d = 1.0 / 6.0; }
    else { b = (1.0 - std::cos(th)) / th2; d = (th - std::sin(th)) / (th2 * th); }
    const double Om[9] = { 0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0 };
    double Om2[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = w[i] * w[j] - (i == j ? th2 : 0.0);
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) + b * Om[i] + d * Om2[i];
    // exp's rotation as a quaternion: axis-angle
    double e[4] = { 0, 0, 0, 1 };
    if (th > 0.0) { const double s = std::sin(0.5 * th) / th; e[0] = s * w[0]; e[1] = s * w[1]; e[2] = s * w[2]; e[3] = std::cos(0.5 * th); }
    const double et[3] = { V[0] * u[3] + V[1] * u[4] + V[2] * u[5], V[3] * u[3] + V[4] * u[4] + V[5] * u[5], V[6] * u[3] + V[7] * u[4] + V[8] * u[5] };
    double r[4];
    r[3] = e[3] * T[3] - e[0] * T[0] - e[1] * T[1] - e[2] * T[2];
    r[0] = e[3] * T[0] + e[0] * T[3] + e[1] * T[2] - e[2] * T[1];
    r[1] = e[3] * T[1] + e[1] * T[3] + e[2] * T[0] - e[0] * T[2];
    r[2] = e[3] * T[2] + e[2] * T[3] + e[0] * T[1] - e[1] * T[0];
    qnorm(r);
    double Re[9], Xc[3];
    q2R(e, Re);
    const double zero[3] = { 0, 0, 0 };
    im_map(Re, zero, T + 4, Xc);
    for (int k = 0; k < 4; ++k) out[k] = r[k];
    for (int k = 0; k < 3; ++k) out[4 + k] = et[k] + Xc[k];
}

bool chol6(const double Su[21], double lambda, const double b[6], double x[6])
{
    double L[36];
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
            const int i = a <= c ? a : c, j = a <= c ? c : a;
            L[a * 6 + c] = Su[i * 6 - i * (i - 1) / 2 + (j - i)] + (a == c ? lambda : 0.0);
        }
    for (int j = 0; j < 6; ++j) {
        double d = L[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        L[j * 6 + j] = std::sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double s = L[i * 6 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = s / L[j * 6 + j];
        }
    }
    for (int i = 0; i < 6; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * x[k]; x[i] = s / L[i * 6 + i]; }
    for (int i = 5; i >= 0; --i) { double s = x[i]; for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k]; x[i] = s / L[i * 6 + i]; }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[4];
    double par[5], pose[7];
    if (std::fread(hd, 4, 4, f) != 4 || std::fread(par, 8, 5, f) != 5 || std::fread(pose, 8, 7, f) != 7) return 2;
    const int n = hd[0], max_iters = hd[1], max_trials = hd[2] > 0 ? hd[2] : 10;
    if (n < 1 || n > 100000 || max_iters < 0 || max_iters > MOVBA_MAX_INIT_MAP_ITERS) return 2;
    std::vector<double> o1(2 * (size_t)n), o2(2 * (size_t)n), X(3 * (size_t)n), s1(n), s2(n), lin((size_t)kImLin * n), Xbk;
    if (std::fread(o1.data(), 8, o1.size(), f) != o1.size() || std::fread(o2.data(), 8, o2.size(), f) != o2.size() ||
        std::fread(X.data(), 8, X.size(), f) != X.size() || std::fread(s1.data(), 8, s1.size(), f) != s1.size() ||
        std::fread(s2.data(), 8, s2.size(), f) != s2.size()) return 2;
    std::fclose(f);
    const double cam[4] = { par[0], par[1], par[2], par[3] }, huber = par[4];
    qnorm(pose);
    double lambda = 0.0, ni = 2.0, cost0 = 0.0, R[9];
    int iters = 0, solves = 0, chol_fail = 0;
    bool ok = true;
    std::vector<double> trace;
    for (int it = 0; it < max_iters && ok; ++it) {
        q2R(pose, R);
        double acc[28] = { 0.0 }, md = 0.0;
        for (int k = 0; k < n; ++k) {
            double *l = &lin[(size_t)kImLin * k];
            im_linearize(R, pose + 4, cam, huber, &X[3 * k], &o1[2 * k], &o2[2 * k], s1[k], s2[k], l, acc);
            md = std::fmax(std::fmax(std::fabs(l[0]), std::fabs(l[3])), std::fmax(std::fabs(l[5]), md));
        }
        double F0 = acc[27];
        if (it == 0) {
            for (int a = 0; a < 6; ++a) md = std::fmax(std::fabs(acc[a * 6 - a * (a - 1) / 2]), md);
            lambda = lm_lambda_init(md); ni = 2.0; cost0 = F0;
        }
        double rho = 0.0;
        int qmax = 0;
        bool lambda_ok = true;
        do {
            double sc[27] = { 0.0 }, Su[21], bS[6], xp[6], trial[7], Rt[9];
            for (int k = 0; k < n; ++k) im_schur(&lin[(size_t)kImLin * k], lambda, sc);
            for (int e = 0; e < 21; ++e) Su[e] = acc[e] - sc[e];
            for (int a = 0; a < 6; ++a) bS[a] = acc[21 + a] - sc[21 + a];
            const bool ok2 = chol6(Su, lambda, bS, xp);
            for (int e = 0; e < 7; ++e) trial[e] = pose[e];
            if (ok2) oplus(xp, pose, trial);
            q2R(trial, Rt);
            double F1 = 0.0, scale = 0.0;
            Xbk = X;
            if (ok2) for (int a = 0; a < 6; ++a) scale += xp[a] * (lambda * xp[a] + acc[21 + a]);
            for (int k = 0; k < n; ++k) {
                double xl[3], c2[2];
                if (ok2) {
                    scale += im_back(&lin[(size_t)kImLin * k], lambda, xp, xl);
                    for (int c = 0; c < 3; ++c) X[3 * k + c] += xl[c];
                }
                F1 += im_cost(Rt, trial + 4, cam, huber, &X[3 * k], &o1[2 * k], &o2[2 * k], s1[k], s2[k], c2);
            }
            if (!ok2) ++chol_fail;
            const LmGain gain = lm_gain(F0, F1, scale, ok2);
            F1 = gain.F1; rho = gain.rho;
            const bool accept = lm_accept(rho, F1);
            trace.insert(trace.end(), { lambda, F0, F1, rho, accept ? 1.0 : 0.0 });
            lambda_ok = lm_update(accept, rho, lambda, ni);
            if (accept) {
                F0 = F1;
                for (int e = 0; e < 7; ++e) pose[e] = trial[e];
            } else {
                X = Xbk;
            }
            ++solves; ++qmax;
        } while (lm_more_trials(rho, qmax, max_trials, lambda_ok));
        iters = it + 1;
        if (lm_terminate(rho, qmax, max_trials, lambda_ok)) ok = false;
    }
    q2R(pose, R);
    double cost = 0.0;
    std::vector<double> chi2(2 * (size_t)n);
    for (int k = 0; k < n; ++k) cost += im_cost(R, pose + 4, cam, huber, &X[3 * k], &o1[2 * k], &o2[2 * k], s1[k], s2[k], &chi2[2 * k]);
    if (max_iters == 0) cost0 = cost;
    std::printf("pose");
    for (int e = 0; e < 7; ++e) std::printf(" %.17g", pose[e]);
    std::printf("\ncost0 %.17g\ncost %.17g\nlambda %.17g\niters %d\nsolves %d\ncholfail %d\n", cost0, cost, lambda, iters, solves, chol_fail);
    for (size_t t = 0; t < trace.size(); t += 5) std::printf("trial %.17g %.17g %.17g %.17g %d\n", trace[t], trace[t + 1], trace[t + 2], trace[t + 3], (int)trace[t + 4]);
    std::printf("points");
    for (double v : X) std::printf(" %.17g", v);
    std::printf("\nchi2");
    for (double v : chi2) std::printf(" %.17g", v);
    std::printf("\n");
    return 0;
}
