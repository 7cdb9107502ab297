// The fake device's side of movba_two_view (mov-slam_amd/csrc/two_view.cpp): the launch wrapper of two_view.h as a closure on
// the fake stream (fake_hip.cpp).  It runs the library's own arithmetic (two_view_math.h: plain C++, the code the kernels
// inline) pair by pair on the CPU - the five-point solve as a group of ONE lane - reading every input through the pointers the
// host laid out and writing results where the host said, so the sanitizers see the host's layout and hand-offs and a driver
// can check the values that come back.  Test infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <vector>

#include "two_view.h"
#include "two_view_math.h"

namespace {
std::atomic<int> g_tv_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_two_view: %s\n", what);
    g_tv_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_two_view_errors() { return g_tv_errors.load(); }

namespace movba {

static void fake_pair(const TvDev &d, int pi)
{
    const TvPair p = d.pairs[pi];
    const double *o1 = d.obs1 + 2 * (size_t)p.m0, *o2 = d.obs2 + 2 * (size_t)p.m0;
    const double inv_f = 1.0 / p.f, f2 = p.f * p.f, nan = __builtin_nan("");
    auto nx = [&](const double *o, int i, int k) { return (o[2 * i + k] - (k ? p.cy : p.cx)) * inv_f; };
    // k_tv_hyp
    const Magsac ms(p.thr2);
    std::vector<double> sl(p.n_hyp);
    std::vector<int> sc(p.n_hyp), sb(p.n_hyp);
    TvWork w;
    for (int h = 0; h < p.n_hyp; ++h) {
        const size_t hg = (size_t)p.h0 + h;
        double q[20], E[90] = { 0.0 };
        for (int k = 0; k < 5; ++k) {
            const int i = d.samples[5 * hg + k];
            if (i < 0 || i >= p.n) { bad("sample index out of range"); return; }
            q[4 * k] = nx(o1, i, 0); q[4 * k + 1] = nx(o1, i, 1); q[4 * k + 2] = nx(o2, i, 0); q[4 * k + 3] = nx(o2, i, 1);
        }
        int ns = 0;
        tv_five_point(w, q, E, &ns, 0, 1, TvSyncNone{});
        d.nsol[hg] = ns;
        for (int e = 0; e < 90; ++e) d.cand[90 * hg + e] = e < 9 * ns ? E[e] : 0.0;
        double bl = 0.0;
        int bi = -1, bc = 0;
        for (int c = 0; c < 10; ++c) {
            if (c >= ns) { d.loss[10 * hg + c] = INFINITY; d.cnt[10 * hg + c] = -1; continue; }
            double ls = 0.0;
            int cn = 0;
            for (int i = 0; i < p.n; ++i) {
                const double s2 = f2 * tv_sampson2(E + 9 * c, nx(o1, i, 0), nx(o1, i, 1), nx(o2, i, 0), nx(o2, i, 1));
                double l1, wt;
                ms.terms(s2, true, p.thr2, l1, wt);
                ls += l1; cn += s2 <= p.thr2;
            }
            d.loss[10 * hg + c] = ls; d.cnt[10 * hg + c] = cn;
            if (bi < 0 || ls < bl) { bi = 10 * h + c; bl = ls; bc = cn; }
        }
        sl[h] = bl; sc[h] = bc; sb[h] = bi;
    }
    // k_tv_recover
    int best = -1, used = 0;
    tv_walk(sl.data(), sc.data(), sb.data(), p.n_hyp, p.n, p.conf, &best, &used);
    double *o = p.out;
    for (int e = 0; e < kTvOutDoubles; ++e) o[e] = 0.0;
    o[3] = 1.0; o[17] = MOVBA_TV_NO_MODEL; o[21] = used; o[22] = -1.0;
    int n_in = 0;
    std::vector<uint8_t> inl(p.n, 0);
    const double *Ew = best >= 0 ? d.cand + 90 * (size_t)p.h0 + 9 * (size_t)best : nullptr;
    if (Ew)
        for (int i = 0; i < p.n; ++i) {
            inl[i] = f2 * tv_sampson2(Ew, nx(o1, i, 0), nx(o1, i, 1), nx(o2, i, 0), nx(o2, i, 1)) <= p.thr2;
            n_in += inl[i];
        }
    if (!Ew || n_in == 0) {
        for (int i = 0; i < p.n; ++i) {
            p.inlier[i] = 0; p.good[i] = 0; p.code[i] = MOVBA_TV_CHK_NONE;
            p.points[3 * (size_t)i] = nan; p.points[3 * (size_t)i + 1] = nan; p.points[3 * (size_t)i + 2] = nan;
        }
        return;
    }
    double Rt[2][9], tt[3], R[9], t[3];
    tv_decompose(Ew, Rt[0], Rt[1], tt);
    int cheir[4], pick = 0;
    for (int c = 0; c < 4; ++c) {
        for (int e = 0; e < 3; ++e) t[e] = (c & 2) ? -tt[e] : tt[e];
        cheir[c] = 0;
        for (int i = 0; i < p.n; ++i)
            if (inl[i]) cheir[c] += tv_cheirality(Rt[c & 1], t, nx(o1, i, 0), nx(o1, i, 1), nx(o2, i, 0), nx(o2, i, 1), p.max_depth);
        if (cheir[c] > cheir[pick]) pick = c;
    }
    for (int e = 0; e < 9; ++e) R[e] = Rt[pick & 1][e];
    for (int e = 0; e < 3; ++e) t[e] = (pick & 2) ? -tt[e] : tt[e];
    // k_tv_check
    std::vector<double> cs;
    int n_good = 0;
    for (int i = 0; i < p.n; ++i) {
        const bool ok = inl[i] && tv_cheirality(R, t, nx(o1, i, 0), nx(o1, i, 1), nx(o2, i, 0), nx(o2, i, 1), p.max_depth);
        p.inlier[i] = ok;
        double X[3] = { nan, nan, nan }, cp = 0.0;
        uint8_t code = MOVBA_TV_CHK_REJ_NOT_INLIER;
        if (ok) code = tv_check(R, t, p.fx, p.fy, p.cx, p.cy, o1[2 * i], o1[2 * i + 1], o2[2 * i], o2[2 * i + 1], p.th2, X, &cp);
        const bool acc = code == MOVBA_TV_CHK_GOOD || code == MOVBA_TV_CHK_LOW_PARALLAX;
        if (acc) { cs.push_back(cp); ++n_good; }
        p.points[3 * (size_t)i] = X[0]; p.points[3 * (size_t)i + 1] = X[1]; p.points[3 * (size_t)i + 2] = X[2];
        p.good[i] = code == MOVBA_TV_CHK_GOOD; p.code[i] = code;
    }
    double parallax = 0.0;
    if (n_good > 0) {
        const int idx = n_good - 1 < 50 ? n_good - 1 : 50;
        int at = 0;             // rank by counting, as the kernel
        for (int i = 0; i < n_good; ++i) {
            int rank = 0;
            for (int j = 0; j < n_good; ++j) rank += cs[j] < cs[i] || (cs[j] == cs[i] && j < i);
            if (rank == idx) at = i;
        }
        parallax = std::acos(cs[at]) * 180.0 / 3.14159265358979323846;
    }
    const int min_good = std::max((int)(0.75 * (double)n_in), p.min_tri);
    const int outcome = cheir[pick] < min_good ? MOVBA_TV_FEW_GOOD : (parallax > p.min_par ? MOVBA_TV_OK : MOVBA_TV_LOW_PARALLAX);
    double qv[4];
    tv_R2q(R, qv);
    o[0] = qv[0]; o[1] = qv[1]; o[2] = qv[2]; o[3] = qv[3]; o[4] = t[0]; o[5] = t[1]; o[6] = t[2];
    for (int e = 0; e < 9; ++e) o[7 + e] = Ew[e];
    o[16] = parallax; o[17] = outcome; o[18] = n_in; o[19] = cheir[pick]; o[20] = n_good; o[21] = used; o[22] = best;
}

hipError_t launch_two_view(const TvDev &dev, hipStream_t s)
{
    const TvDev d = dev;
    fake_enqueue(s, [=] {
        if (d.hyp_first[0] != 0 || d.hyp_first[d.n_pairs] != d.n_hyp_total) { bad("hyp_first does not span the samples"); return; }
        for (int p = 0; p < d.n_pairs; ++p) {
            if (d.pairs[p].h0 != d.hyp_first[p] || d.hyp_first[p + 1] - d.hyp_first[p] != d.pairs[p].n_hyp) { bad("hyp_first and the pairs disagree"); return; }
            fake_pair(d, p);
        }
    });
    return hipSuccess;
}

}  // namespace movba
