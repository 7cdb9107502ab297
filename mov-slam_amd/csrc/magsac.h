// sigma-consensus++ scoring shared by the hypothesis stages of movba_pose_opt (pose_kernels.hip) and movba_two_view
// (two_view_math.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace movba {

// sigma-consensus++ (MAGSAC++: Barath, Noskova, Ivashechkin, Matas, CVPR 2020), what flag 38 = cv::USAC_MAGSAC of the reference's
// call scores models with (src/Optimizer.cc:437, Examples/Monocular/TartanAir.yaml:51): a residual is not classified at ONE
// threshold, its noise scale is marginalised over (0, sigma_max], sigma_max = tau / k, tau^2 = chi2_gate (the caller's
// reprojectionError), k^2 = 9.21034 (0.99 quantile of chi^2 with the residual's 2 degrees of freedom).  With x = r^2 / (2
// sigma_max^2), x_k = k^2 / 2 the paper's incomplete gamma functions are elementary for n = 2:
//     weight  w(r)   = sqrt(pi) (erfc(sqrt x) - erfc(sqrt x_k))                                             r <= tau, else 0
//     loss    rho(r) = sigma_max^2 / 2 (sqrt(pi) / 2 erf(sqrt x) - sqrt x exp(-x)) + r^2 / 4 w(r)           r <= tau, rho(tau) beyond
// (common factors dropped).  loss: rho / rho(tau) in [0, 1], 1 = outlier or behind the camera; weight: w / w(0).
struct Magsac {
    double s2, g_k, inv_rho_max, inv_w0;
    __host__ __device__ explicit Magsac(double gate)
    {
        const double sq_pi = 1.7724538509055160273, k2 = 9.210340371976184, xk = 0.5 * k2;
        s2 = gate / k2;
        g_k = sq_pi * erfc(sqrt(xk));
        inv_rho_max = 1.0 / (0.5 * s2 * (0.5 * sq_pi * erf(sqrt(xk)) - sqrt(xk) * exp(-xk)));
        inv_w0 = 1.0 / (sq_pi * (1.0 - erfc(sqrt(xk))));
    }
    __host__ __device__ void terms(double chi2, bool in_front, double gate, double &loss, double &weight) const
    {
        const double sq_pi = 1.7724538509055160273;
        if (!in_front || !(chi2 <= gate)) { loss = 1.0; weight = 0.0; return; }
        const double x = chi2 / (2.0 * s2), sx = sqrt(x);
        const double w = sq_pi * erfc(sx) - g_k;
        loss = (0.5 * s2 * (0.5 * sq_pi * erf(sx) - sx * exp(-x)) + 0.25 * chi2 * w) * inv_rho_max;
        weight = w > 0.0 ? w * inv_w0 : 0.0;
    }
};

}  // namespace movba
