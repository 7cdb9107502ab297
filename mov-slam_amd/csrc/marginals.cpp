// movba_lba_marginals (include/movba.h): marginal covariances of the window's last solve, read out of the normal matrix the LM
// kernels build at its final state.  The device pass is marginals.hip; this file checks the call, lays out the scratch, queues
// the pass and hands the blocks over after ONE synchronisation, or nothing at all when the matrix is not positive definite.
#include <cmath>
#include <cstring>

#include "handle.h"
#include "kernels.h"
#include "marginals.h"

using namespace movba;

extern "C" {

int movba_lba_marginals(movba_handle *h, double damping, double *pose_cov, double *point_cov)
{
    if (!h || (!pose_cov && !point_cov) || !(damping >= 0.0) || !std::isfinite(damping)) return MOVBA_ERR_ARG;
    // a run of this upload that solved the window (not one that ended before the solve, was stopped, or failed)
    if (!h->uploaded || !h->ran || h->early_status != MOVBA_OK || h->run_status != MOVBA_OK || h->ctrl_host->n_sync_timeouts > 0)
        return MOVBA_ERR_STATE;
    HIP_TRY(hipSetDevice(h->device));
    const DevWindow &w = h->win;
    const int nt = w.dense.ntile, NP = w.NP, P = w.P;
    const size_t tile = (size_t)kDenseNB * kDenseNB, ntri = (size_t)nt * (nt + 1) / 2;
    Carver c;
    const size_t o_ctrl = c.take<Ctrl>(1), o_linv = c.take<double>((size_t)nt * tile);
    const size_t o_w = c.take<double>(ntri * tile), o_sig = c.take<double>(ntri * tile);
    // the outputs in one block behind them: the two flag words, the pose blocks, the point blocks (one copy to the host)
    const size_t o_out = c.off;
    Carver oc;
    const size_t o_flags = oc.take<int32_t>(4), o_pose = oc.take<double>((size_t)NP * 36), o_pt = oc.take<double>((size_t)P * 9);
    const size_t out_bytes = point_cov ? oc.off : o_pt;
    // the device scratch and the pinned image of the outputs
    int rc = h->marg.grow(h, o_out + oc.off); if (rc == MOVBA_OK) rc = h->marg_host.grow(h, oc.off); if (rc) return rc;

    char *a = h->marg.p, *out = a + o_out;
    MargDev m{};
    m.w = w;
    m.w.ctrl = reinterpret_cast<Ctrl *>(a + o_ctrl);
    m.run_ctrl = w.ctrl;
    m.ctrl = m.w.ctrl;
    m.damping = damping;
    m.linv = reinterpret_cast<double *>(a + o_linv);
    m.W = reinterpret_cast<double *>(a + o_w);
    m.sig = reinterpret_cast<double *>(a + o_sig);
    m.flags = reinterpret_cast<int32_t *>(out + o_flags);
    m.pose_out = reinterpret_cast<double *>(out + o_pose);
    m.point_out = reinterpret_cast<double *>(out + o_pt);
    m.want_points = point_cov ? 1 : 0;
    m.pose_blocks = (NP + 255) / 256;
    HIP_TRY(launch_marginals(m, h->stream));
    HIP_TRY(hipMemcpyAsync(h->marg_host.p, out, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    const char *hb = h->marg_host.p;
    const int32_t *flags = reinterpret_cast<const int32_t *>(hb + o_flags);
    if (flags[0] || flags[1]) return MOVBA_SINGULAR;
    if (pose_cov) {
        const double *src = reinterpret_cast<const double *>(hb + o_pose);
        std::memcpy(pose_cov, src, sizeof(double) * 36 * (size_t)NP);
        for (int i = 0; i < NP && i < (int)h->pose_fixed.size(); ++i)
            if (h->pose_fixed[i]) std::memset(pose_cov + 36 * (size_t)i, 0, sizeof(double) * 36);
    }
    if (point_cov) std::memcpy(point_cov, hb + o_pt, sizeof(double) * 9 * (size_t)P);
    return MOVBA_OK;
}

}  // extern "C"
