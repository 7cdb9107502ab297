"""movba_two_view without a GPU.

`two_view_ref` is the yardstick of tests/test_gpu_two_view.py: a numpy fp64 restatement of TwoViewReconstruction::Reconstruct
(TwoViewReconstruction.cc:68-245) with the five-point problem (Nister 2004) solved ANOTHER way than the library: null space by
numpy.linalg.svd, then either the degree-10 polynomial's roots by numpy.roots ("poly") or the eigenvectors of the 10 x 10
action matrix over a graded monomial order (Stewenius 2006, "action").  It never calls the library.  This file checks the
yardstick itself, MEASURES the tolerances the GPU test uses from the spread of its two variants, asserts the caps on the
committed scenes, and checks the C-ABI's host side over the fake device of tests/hipstub (which runs the library's own
two_view_math.h on the CPU) under the sanitizers.
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

TV_OK, TV_NO_MODEL, TV_FEW_GOOD, TV_LOW_PARALLAX = 0, 1, 2, 3
CHK_NONE, CHK_GOOD, CHK_LOW_PARALLAX = 0, 1, 2
CHK_NOT_INLIER, CHK_W0, CHK_BEHIND1, CHK_BEHIND2, CHK_REPROJ1, CHK_REPROJ2 = range(16, 22)
DEFAULTS = dict(threshold=1.0, confidence=0.999, sigma=1.0, min_parallax_deg=1.0, max_depth=50.0, min_triangulated=50)

# ---- measured constants (test_tolerances_are_the_measured_ones prints them and fails if they are below what it measures) ----
# largest Frobenius distance between matched, well-conditioned candidates (sign and scale fixed) of the two variants
E_SPREAD_MEASURED = 5.1e-5
# largest difference of the final pose (quaternion and unit translation, component-wise) / of the points (relative) between
# the two variants on the committed pairs that are not tie pairs
POSE_SPREAD_MEASURED = 4.0e-10
POS_SPREAD_MEASURED = 1.8e-9
# largest relative difference of a candidate's loss between the two variants (what makes a pair a "tie" pair)
LOSS_SPREAD_MEASURED = 3.6e-6
# largest difference of the parallax (degrees, relative to max(1, parallax)) between the two variants
PARALLAX_SPREAD_MEASURED = 6.0e-10
E_TOL, POSE_TOL, POS_TOL = 10 * E_SPREAD_MEASURED, 10 * POSE_SPREAD_MEASURED, 10 * POS_SPREAD_MEASURED
PARALLAX_TOL = 10 * PARALLAX_SPREAD_MEASURED
# the restatement's own rule for "real": imaginary part of a root / eigenvalue against its size
IMAG_TOL = 1e-7
ILL_CAP, EDGE_CAP, TIE_CAP = 1e-2, 1e-3, 2e-2
EDGE_REL = 1e-6         # a match is ON a gate when its quantity is within this (relative) of the gate: >> POS_TOL's effect

# the committed scenes: (label, make_two_view arguments, ransac_iters, ransac_seed)
SCENES = [(f"{sc} {k}", dict(n_matches=500, inlier_frac=0.7, noise_px=0.5, seed=8100 + 10 * i + k, scene=sc), 64, 31 + k)
          for i, sc in enumerate(("general", "planar", "forward")) for k in range(4)]

try:
    from scipy.special import erf as _erf, erfc as _erfc
except ImportError:                                      # (no scipy: math's, element by element)
    _erf, _erfc = np.vectorize(math.erf), np.vectorize(math.erfc)


def samples_ref(n, n_hyp, seed):
    """movba_two_view_samples restated (xorshift32, stream constant 0x85EBCA6B, five distinct indices by rejection)"""
    x = ((seed or 0x9E3779B9) ^ 0x85EBCA6B) & 0xFFFFFFFF
    x = x or 0x85EBCA6B
    out = np.zeros((n_hyp, 5), np.int32)
    for h in range(n_hyp):
        s = []
        while len(s) < 5:
            x ^= (x << 13) & 0xFFFFFFFF; x ^= x >> 17; x ^= (x << 5) & 0xFFFFFFFF
            if x % n not in s:
                s.append(x % n)
        out[h] = s
    return out


# ---- five-point, two ways -----------------------------------------------------------------------------------------------
NISTER = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
          (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
GRLEX = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
         (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(a, b):
    out = np.zeros((4, 4, 4))
    for i, j, k in zip(*np.nonzero(a)):
        for l, m, n in zip(*np.nonzero(b)):
            out[i + l, j + m, k + n] += a[i, j, k] * b[l, m, n]
    return out


def _constraints(basis, order):
    """the ten cubic constraints on E = x X + y Y + z Z + W as a 10 x 20 matrix over `order`"""
    E = np.empty((3, 3), object)
    for i in range(3):
        for j in range(3):
            p = np.zeros((4, 4, 4))
            p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = basis[:, 3 * i + j]
            E[i, j] = p
    EEt = np.empty((3, 3), object)
    for i in range(3):
        for k in range(3):
            EEt[i, k] = sum(_pmul(E[i, l], E[k, l]) for l in range(3))
    tr = EEt[0, 0] + EEt[1, 1] + EEt[2, 2]
    polys = [2 * sum(_pmul(EEt[i, k], E[k, j]) for k in range(3)) - _pmul(tr, E[i, j]) for i in range(3) for j in range(3)]
    det = (_pmul(_pmul(E[0, 0], E[1, 1]), E[2, 2]) + _pmul(_pmul(E[0, 1], E[1, 2]), E[2, 0]) + _pmul(_pmul(E[0, 2], E[1, 0]), E[2, 1])
           - _pmul(_pmul(E[0, 2], E[1, 1]), E[2, 0]) - _pmul(_pmul(E[0, 1], E[1, 0]), E[2, 2]) - _pmul(_pmul(E[0, 0], E[1, 2]), E[2, 1]))
    polys.append(det)
    return np.array([[p[m] for m in order] for p in polys])


def _canon(E):
    E = np.asarray(E, float).reshape(-1, 3, 3)
    E = E * (math.sqrt(2.0) / np.linalg.norm(E.reshape(-1, 9), axis=1))[:, None, None]
    flat = E.reshape(-1, 9)
    big = flat[np.arange(len(flat)), np.abs(flat).argmax(1)]
    return E * np.sign(big)[:, None, None]


def five_point_ref(q1, q2, solver="poly"):
    """q1, q2 (5, 2) normalised -> (E (k, 3, 3) canonical, root_err (k,): estimated relative error of each root (poly only))"""
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    Q = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(5)], 1)
    basis = np.linalg.svd(Q)[2][5:9]
    Es, errs = [], []
    if solver == "poly":
        A = _constraints(basis, NISTER)
        G = np.linalg.solve(A[:, :10], A[:, 10:])
        P = np.polynomial.polynomial
        rows = []
        for a, b in ((4, 5), (6, 7), (8, 9)):
            ga, gb = G[a], G[b]
            rows.append([np.array([ga[2], ga[1] - gb[2], ga[0] - gb[1], -gb[0]]),
                         np.array([ga[5], ga[4] - gb[5], ga[3] - gb[4], -gb[3]]),
                         np.array([ga[9], ga[8] - gb[9], ga[7] - gb[8], ga[6] - gb[7], -gb[6]])])
        det = np.zeros(11)
        for j in range(3):
            c1, c2 = (j + 1) % 3, (j + 2) % 3
            mn = P.polysub(P.polymul(rows[1][c1], rows[2][c2]), P.polymul(rows[1][c2], rows[2][c1]))
            t = P.polymul(rows[0][j], mn)
            det[:min(len(t), 11)] += t[:11]
        roots = np.roots(det[::-1])
        for z in roots:
            if abs(z.imag) > IMAG_TOL * max(1.0, abs(z)):
                continue
            z = z.real
            B = np.array([[P.polyval(z, rows[i][j]) for j in range(3)] for i in range(3)])
            B = B / np.linalg.norm(B, axis=1, keepdims=True)
            v = np.linalg.svd(B)[2][2]
            Es.append((v[0] * basis[0] + v[1] * basis[1] + v[2] * (z * basis[2] + basis[3])).reshape(3, 3))
            dp = abs(P.polyval(z, P.polyder(det)))
            mag = P.polyval(abs(z), np.abs(det))
            errs.append(np.finfo(float).eps * mag / max(dp, 1e-300) / max(1.0, abs(z)))
    else:
        A = _constraints(basis, GRLEX)
        G = np.linalg.solve(A[:, :10], A[:, 10:])
        # multiplication by x on the quotient basis (x^2 xy xz y^2 yz z^2 x y z 1): x b = (x^3 x^2y x^2z xy^2 xyz xz^2 x^2 xy xz x)
        Mx = np.zeros((10, 10))
        Mx[:6] = -G[:6]
        Mx[6, 0] = Mx[7, 1] = Mx[8, 2] = Mx[9, 6] = 1.0
        lam, V = np.linalg.eig(Mx)
        for k in range(10):
            if abs(lam[k].imag) > IMAG_TOL * max(1.0, abs(lam[k])):
                continue
            v = V[:, k] / V[9, k]
            x, y, z = v[6].real, v[7].real, v[8].real
            Es.append((x * basis[0] + y * basis[1] + z * basis[2] + basis[3]).reshape(3, 3))
            errs.append(0.0)
    if not Es:
        return np.zeros((0, 3, 3)), np.zeros(0)
    return _canon(np.array(Es)), np.array(errs)


def match_candidates(Ea, Eb):
    """for every candidate of Ea the distance to the nearest of Eb (inf when Eb is empty)"""
    if len(Ea) == 0:
        return np.zeros(0)
    if len(Eb) == 0:
        return np.full(len(Ea), np.inf)
    Ea, Eb = _canon(Ea), _canon(Eb)
    return np.linalg.norm(Ea[:, None] - Eb[None], axis=(2, 3)).min(1)


# ---- scoring ------------------------------------------------------------------------------------------------------------
def sampson2_px(E, obs1, obs2, f, cx, cy):
    """squared Sampson distance in pixels through F = K_f^-T E K_f^-1"""
    Kinv = np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]])
    F = Kinv.T @ E @ Kinv
    p1 = np.concatenate([obs1, np.ones((len(obs1), 1))], 1); p2 = np.concatenate([obs2, np.ones((len(obs2), 1))], 1)
    Fp1 = p1 @ F.T; Ftp2 = p2 @ F
    num = np.einsum('mi,mi->m', p2, Fp1)
    with np.errstate(all="ignore"):
        return num * num / (Fp1[:, 0] ** 2 + Fp1[:, 1] ** 2 + Ftp2[:, 0] ** 2 + Ftp2[:, 1] ** 2)


def magsac_loss(r2, gate):
    """sigma-consensus++ loss of squared residuals (MAGSAC++, n = 2 degrees of freedom), normalised to [0, 1]"""
    k2 = 9.210340371976184; xk = 0.5 * k2; sq_pi = math.sqrt(math.pi)
    s2 = gate / k2
    g_k = sq_pi * math.erfc(math.sqrt(xk))
    rho_max = 0.5 * s2 * (0.5 * sq_pi * math.erf(math.sqrt(xk)) - math.sqrt(xk) * math.exp(-xk))
    r2 = np.asarray(r2, float)
    inside = r2 <= gate
    x = np.where(inside, r2, 0.0) / (2 * s2); sx = np.sqrt(x)
    w = sq_pi * _erfc(sx) - g_k
    loss = (0.5 * s2 * (0.5 * sq_pi * _erf(sx) - sx * np.exp(-x)) + 0.25 * np.where(inside, r2, 0.0) * w) / rho_max
    return np.where(inside, loss, 1.0)


def walk(losses, counts, n, conf):
    """the stopping rule over samples in drawing order -> (winner (h, c) or None, samples_used)"""
    best, bl, need = None, np.inf, np.inf
    rule = 0.0 < conf < 1.0
    for h in range(len(losses)):
        if len(losses[h]):
            c = int(np.argmin(losses[h]))
            if losses[h][c] < bl:
                best, bl = (h, c), losses[h][c]
                if rule:
                    w5 = (counts[h][c] / n) ** 5
                    l = 0.0 if w5 >= 1 else math.log(1 - w5)
                    need = 0.0 if w5 >= 1 else (math.log(1 - conf) / l if l < 0 else np.inf)
        if rule and best is not None and h + 1 >= need:
            return best, h + 1
    return best, len(losses)


# ---- pose recovery and CheckRT ---------------------------------------------------------------------------------------------
def _dlt(P1, P2, a1, b1, a2, b2):
    A = np.stack([a1[:, None] * P1[2] - P1[0], b1[:, None] * P1[2] - P1[1], a2[:, None] * P2[2] - P2[0], b2[:, None] * P2[2] - P2[1]], 1)
    return np.linalg.svd(A)[2][:, 3, :]


def recover_pose(E, x1, x2, mask, max_depth):
    """cv::recoverPose restated: the four (R, t), linear triangulation of the masked matches, depth bounds -> R, t, pass mask, counts"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    P1 = np.eye(3, 4)
    best = None
    counts = []
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P2 = np.concatenate([R, tt[:, None]], 1)
        with np.errstate(all="ignore"):
            xh = _dlt(P1, P2, x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1])
            X = xh[:, :3] / xh[:, 3:4]
            z1 = X[:, 2]; z2 = X @ R[2] + tt[2]
            ok = mask & (z1 > 0) & (z1 < max_depth) & (z2 > 0) & (z2 < max_depth)
        counts.append(int(ok.sum()))
        if best is None or counts[-1] > best[3]:
            best = (R, tt, ok, counts[-1], z1, z2)
    return best[0], best[1], best[2], counts, best[4], best[5]


def check_rt(R, t, cam, obs1, obs2, inlier, th2):
    """CheckRT (:120-245) over all matches -> dict(code, points, good, n_good, parallax, q: the gated quantities)"""
    fx, fy, cx, cy = cam
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    P1 = K @ np.eye(3, 4); P2 = K @ np.concatenate([R, t[:, None]], 1)
    O2 = -R.T @ t
    M = len(obs1)
    with np.errstate(all="ignore"):
        xh = _dlt(P1, P2, obs1[:, 0], obs1[:, 1], obs2[:, 0], obs2[:, 1])
        w = xh[:, 3]
        X = xh[:, :3] / xh[:, 3:4]
        n2 = X - O2
        cosp = np.einsum('mi,mi->m', X, n2) / (np.linalg.norm(X, axis=1) * np.linalg.norm(n2, axis=1))
        Y = X @ R.T + t
        e1 = (fx * X[:, 0] / X[:, 2] + cx - obs1[:, 0]) ** 2 + (fy * X[:, 1] / X[:, 2] + cy - obs1[:, 1]) ** 2
        e2 = (fx * Y[:, 0] / Y[:, 2] + cx - obs2[:, 0]) ** 2 + (fy * Y[:, 1] / Y[:, 2] + cy - obs2[:, 1]) ** 2
        low = cosp < 0.99998
        code = np.where(low, CHK_GOOD, CHK_LOW_PARALLAX)
        for cond, c in reversed(((~inlier, CHK_NOT_INLIER), (w == 0, CHK_W0), ((X[:, 2] <= 0) & low, CHK_BEHIND1),
                                 ((Y[:, 2] <= 0) & low, CHK_BEHIND2), (e1 > th2, CHK_REPROJ1), (e2 > th2, CHK_REPROJ2))):
            code = np.where(cond, c, code)
    code = code.astype(np.uint8)
    acc = code <= CHK_LOW_PARALLAX
    pts = np.where(acc[:, None], X, np.nan)
    n_good = int(acc.sum())
    if n_good > 0:
        srt = np.sort(cosp[acc])
        with np.errstate(all="ignore"):
            parallax = math.degrees(math.acos(srt[min(50, n_good - 1)])) if abs(srt[min(50, n_good - 1)]) <= 1 else float("nan")
    else:
        parallax = 0.0
    return dict(code=code, points=pts, good=(code == CHK_GOOD), n_good=n_good, parallax=parallax,
                q=dict(z1=X[:, 2], z2=Y[:, 2], e1=e1, e2=e2, cosp=cosp, w=w, M=M))


def R2q(R):
    return synth.quat_from_R(np.asarray(R, float))          # (by the largest diagonal entry where the trace is not positive: accurate at w ~ 0)


def hypotheses_ref(pair, samples, solver="poly", threshold=1.0):
    """stage 1 + 2 for every sample -> list of dict(E, root_err, loss, count)"""
    fx, fy, cx, cy = pair["cam"]
    f = 0.5 * (fx + fy)
    o1, o2 = np.asarray(pair["obs1"], float), np.asarray(pair["obs2"], float)
    c = np.array([cx, cy])
    out = []
    for s in samples:
        E, err = five_point_ref((o1[s] - c) / f, (o2[s] - c) / f, solver)
        s2 = [sampson2_px(e, o1, o2, f, cx, cy) for e in E]
        out.append(dict(E=E, root_err=err, loss=np.array([magsac_loss(x, threshold ** 2).sum() for x in s2]),
                        count=np.array([int((x <= threshold ** 2).sum()) for x in s2])))
    return out


def finish_ref(pair, hyp, winner=None, **kw):
    """stages 2 (winner) to 4 over scored hypotheses; winner: force this (h, c) instead of the walk's"""
    a = dict(DEFAULTS, **kw)
    fx, fy, cx, cy = pair["cam"]
    f = 0.5 * (fx + fy)
    o1, o2 = np.asarray(pair["obs1"], float), np.asarray(pair["obs2"], float)
    M = len(o1)
    win, used = walk([h["loss"] for h in hyp], [h["count"] for h in hyp], M, a["confidence"])
    if winner is not None:
        win = winner
    res = dict(samples_used=used, winner=win, outcome=TV_NO_MODEL, n_inliers=0, n_pass=0, n_good=0, parallax=0.0,
               inlier=np.zeros(M, bool), code=np.zeros(M, np.uint8), good=np.zeros(M, bool), points=np.full((M, 3), np.nan))
    if win is None:
        return res
    E = hyp[win[0]]["E"][win[1]]
    s2 = sampson2_px(E, o1, o2, f, cx, cy)
    inl0 = s2 <= a["threshold"] ** 2
    res.update(E=E, n_inliers=int(inl0.sum()), s2=s2)
    if res["n_inliers"] == 0:
        return res
    c = np.array([cx, cy])
    R, t, ok, counts, z1, z2 = recover_pose(E, (o1 - c) / f, (o2 - c) / f, inl0, a["max_depth"])
    chk = check_rt(R, t, pair["cam"], o1, o2, ok, 4 * a["sigma"] ** 2)
    min_good = max(int(0.75 * res["n_inliers"]), a["min_triangulated"])
    outcome = TV_FEW_GOOD if counts and max(counts) < min_good else (TV_OK if chk["parallax"] > a["min_parallax_deg"] else TV_LOW_PARALLAX)
    res.update(outcome=outcome, R=R, t=t, pose=np.concatenate([R2q(R), t]), n_pass=max(counts), inlier=ok, counts=counts,
               rz1=z1, rz2=z2, inl0=inl0, code=chk["code"], good=chk["good"], points=chk["points"], n_good=chk["n_good"],
               parallax=chk["parallax"], q=chk["q"])
    return res


def two_view_ref(pair, ransac_iters, ransac_seed, solver="poly", **kw):
    a = dict(DEFAULTS, **kw)
    samples = samples_ref(len(pair["obs1"]), ransac_iters, ransac_seed)
    hyp = hypotheses_ref(pair, samples, solver, a["threshold"])
    res = finish_ref(pair, hyp, **kw)
    res["hyp"] = hyp
    return res


def edge_matches(res, **kw):
    """matches that sit ON a gate (Sampson threshold, recoverPose's depth bounds, a CheckRT gate) within EDGE_REL"""
    a = dict(DEFAULTS, **kw)
    if "q" not in res:
        return np.zeros(len(res["inlier"]), bool)
    q = res["q"]
    thr2, th2, md = a["threshold"] ** 2, 4 * a["sigma"] ** 2, a["max_depth"]
    with np.errstate(all="ignore"):
        near = lambda v, g, scale=None: np.abs(v - g) <= EDGE_REL * (np.abs(g) if scale is None else scale)   # noqa: E731
        e = near(res["s2"], thr2)
        zs = np.maximum(np.abs(res["rz1"]), 1.0)
        e |= res["inl0"] & (near(res["rz1"], 0, zs) | near(res["rz1"], md) | near(res["rz2"], 0, zs) | near(res["rz2"], md))
        e |= res["inlier"] & (near(q["e1"], th2) | near(q["e2"], th2) | near(q["cosp"], 0.99998, 1e-3) | near(q["z1"], 0, zs) | near(q["z2"], 0, zs))
    return e


def err_to_truth(res, pair):
    """(rotation error, translation direction error) in degrees against the scene's truth"""
    if "R" not in res:
        return float("inf"), float("inf")
    dR = res["R"] @ pair["R"].T
    rot = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1) / 2))))
    tr = math.degrees(math.acos(min(1.0, max(-1.0, float(res["t"] @ pair["t"]) / max(np.linalg.norm(pair["t"]), 1e-300)))))
    return rot, tr


def q2R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def compare_with_ref(got, pair, iters, seed, label="", check_truth=False):
    """What tests/test_gpu_two_view.py (and the fake-device test here) asserts of a result with diagnostics against the restatement."""
    ref = two_view_ref(pair, iters, seed)
    hyp = ref["hyp"]
    # per sample, cap (i): candidates the restatement marks ill-conditioned are left out, at most 1 % of them
    n_c = n_ill = 0
    worst_e = worst_l = 0.0
    for h in range(iters):
        Er = hyp[h]["E"]
        Eg = np.asarray(got["hyp_E"][h][:got["hyp_nsol"][h]])
        ill = hyp[h]["root_err"] > E_SPREAD_MEASURED
        n_c += len(Er); n_ill += int(ill.sum())
        d = match_candidates(Er[~ill], Eg) if len(Er[~ill]) else np.zeros(0)
        assert (d <= E_TOL).all(), (label, h, d, got["hyp_nsol"][h], len(Er))
        worst_e = max(worst_e, float(d.max()) if len(d) else 0.0)
        # every candidate of the library is one of the restatement's or lies beside an ill-conditioned one
        if len(Eg):
            back = match_candidates(Eg, Er)
            extra = back > E_TOL
            assert extra.sum() <= ill.sum(), (label, h, back)
            # losses of matched candidates
            for k in np.flatnonzero(~ill):
                j = int(np.linalg.norm(_canon(Eg) - _canon(Er[k:k + 1]), axis=(1, 2)).argmin())
                worst_l = max(worst_l, abs(got["hyp_loss"][h][j] - hyp[h]["loss"][k]) / max(hyp[h]["loss"][k], 1.0))
    print(f"{label}: {n_c} candidates, {n_ill} ill-conditioned, worst matched distance {worst_e:.3g} (E_TOL {E_TOL:.3g}), "
          f"worst loss difference {worst_l:.3g}")
    assert n_ill <= ILL_CAP * n_c, (label, n_ill, n_c)
    assert worst_l <= 10 * LOSS_SPREAD_MEASURED, (label, worst_l)
    # per pair
    tie = is_tie(hyp, ref)
    edge = edge_matches(ref)
    assert edge.sum() <= max(EDGE_CAP * len(edge), 1), (label, int(edge.sum()))
    print(f"{label}: outcome {got['outcome']} (restatement {ref['outcome']}), tie {tie}, {int(edge.sum())} matches on a gate, "
          f"n_inliers {got['n_inliers']} / {ref['n_inliers']}, n_pass {got['n_pass']} / {ref['n_pass']}, n_good {got['n_good']} / {ref['n_good']}, "
          f"parallax {got['parallax_deg']:.6g} / {ref['parallax']:.6g}, samples {got['samples_used']} / {ref['samples_used']}")
    assert got["n_inliers"] >= got["n_pass"] == int(np.asarray(got["inlier"]).sum())
    assert got["n_good"] == int((np.asarray(got["code"]) <= CHK_LOW_PARALLAX).sum() if got["outcome"] != TV_NO_MODEL else 0)
    assert np.array_equal(np.asarray(got["good"]) != 0, np.asarray(got["code"]) == CHK_GOOD)
    if not tie:
        assert got["samples_used"] == ref["samples_used"] and got["outcome"] == ref["outcome"], label
        if ref["winner"] is not None:
            assert match_candidates(ref["E"][None], got["E"][None])[0] <= E_TOL, label
            dq = min(np.abs(got["pose"][:4] - ref["pose"][:4]).max(), np.abs(got["pose"][:4] + ref["pose"][:4]).max())
            dt = np.abs(got["pose"][4:] - ref["pose"][4:]).max()
            ok = ~edge
            same_code = np.asarray(got["code"]) == ref["code"]
            assert same_code[ok].all() and np.array_equal(np.asarray(got["inlier"])[ok] != 0, ref["inlier"][ok]), \
                (label, np.flatnonzero(~same_code & ok)[:10])
            cmp = same_code & ~np.isnan(ref["points"][:, 0])
            with np.errstate(all="ignore"):
                rel = np.linalg.norm(np.asarray(got["points"]) - ref["points"], axis=1) / np.linalg.norm(ref["points"], axis=1)
            wp = float(rel[cmp].max()) if cmp.any() else 0.0
            print(f"{label}: pose difference {max(dq, dt):.3g} (POSE_TOL {POSE_TOL:.3g}), worst relative point difference {wp:.3g} (POS_TOL {POS_TOL:.3g})")
            assert max(dq, dt) <= POSE_TOL and wp <= POS_TOL, label
            # the counts: a match on a gate may fall either way, no other
            assert abs(got["n_inliers"] - ref["n_inliers"]) <= edge.sum() and abs(got["n_good"] - ref["n_good"]) <= edge.sum(), label
            assert abs(got["n_pass"] - ref["n_pass"]) <= edge.sum(), label
            dpar = abs(got["parallax_deg"] - ref["parallax"]) / max(1.0, abs(ref["parallax"]))
            print(f"{label}: parallax difference {dpar:.3g} (PARALLAX_TOL {PARALLAX_TOL:.3g})")
            assert dpar <= PARALLAX_TOL or parallax_on_edge(ref, edge), label
    if check_truth:
        g = dict(R=q2R(got["pose"][:4]), t=got["pose"][4:]) if got["outcome"] != TV_NO_MODEL else {}
        (gr, gt), (rr, rt) = err_to_truth(g, pair), err_to_truth(ref, pair)
        print(f"{label}: error to truth: rotation {gr:.4g} deg (restatement {rr:.4g}), translation direction {gt:.4g} deg (restatement {rt:.4g})")
        assert gr <= 1.5 * rr and gt <= 1.5 * rt, label
    return dict(tie=tie, ref=ref)


def parallax_on_edge(ref, edge):
    """the parallax is element min(50, nGood - 1) of the sorted accepted cosines: a match on a gate can move it only when it
    is, or could become, one of the accepted cosines up to that element (or when nGood itself decides the index)"""
    if not edge.any() or "q" not in ref:
        return False
    acc = ref["code"] <= CHK_LOW_PARALLAX
    if ref["n_good"] <= 51:
        return True
    pivot = np.sort(ref["q"]["cosp"][acc])[50]
    with np.errstate(all="ignore"):
        return bool((edge & ~(ref["q"]["cosp"] > pivot)).any())


def is_tie(hyp, ref):
    """cap (iii): the winner and the runner-up among the admitted samples differ by less than the measured loss spread"""
    if ref["winner"] is None:
        return False
    ls = np.sort(np.concatenate([h["loss"] for h in hyp[:ref["samples_used"]]]))
    return len(ls) > 1 and (ls[1] - ls[0]) <= LOSS_SPREAD_MEASURED * max(ls[0], 1.0)


# ---- the yardstick itself --------------------------------------------------------------------------------------------
def test_samples_are_five_distinct_indices():
    s = samples_ref(37, 200, 5)
    assert s.min() >= 0 and s.max() < 37 and all(len(set(r)) == 5 for r in s.tolist())
    assert not np.array_equal(s, samples_ref(37, 200, 6))


def test_both_solvers_contain_the_true_essential_matrix():
    for sc in ("general", "planar", "forward"):
        p = synth.make_two_view(60, 1.0, 0.0, 11, scene=sc)
        fx, fy, cx, cy = p["cam"]
        # (exact projections with ONE focal length: the hypothesis stage's camera)
        f = 0.5 * (fx + fy)
        Y = p["X"] @ p["R"].T + p["t"]
        q1, q2 = p["X"][:, :2] / p["X"][:, 2:], Y[:, :2] / Y[:, 2:]
        tx = np.array([[0, -p["t"][2], p["t"][1]], [p["t"][2], 0, -p["t"][0]], [-p["t"][1], p["t"][0], 0]])
        Et = _canon(tx @ p["R"])
        for solver in ("poly", "action"):
            worst = 0.0
            for k in range(0, 60, 5):
                E, _ = five_point_ref(q1[k:k + 5], q2[k:k + 5], solver)
                worst = max(worst, match_candidates(Et, E)[0])
            print(sc, solver, "true E found within", worst, "f", f)
            assert worst < 1e-6


def test_noise_free_scenes_recover_the_motion_and_every_inlier():
    """A plane seen from two views has a second essential matrix that fits every point of the plane exactly (the two-fold
    ambiguity of the planar case): without noise it TIES with the true one, and neither the reference's call nor this one
    looks at cheirality before the winner is chosen.  So on `planar` the true motion must come from a candidate whose loss
    is within two matches' worth of the winner's; on the other scenes from the winner itself."""
    for sc in ("general", "planar", "forward"):
        p = synth.make_two_view(300, 0.8, 0.0, 21, scene=sc, cam=(460.0, 460.0, 367.0, 248.0))
        r = two_view_ref(p, 48, 3)
        if sc == "planar":
            wl = r["hyp"][r["winner"][0]]["loss"][r["winner"][1]]
            tied = [(h, c) for h in range(r["samples_used"]) for c in range(len(r["hyp"][h]["loss"])) if r["hyp"][h]["loss"][c] <= wl + 2.0]
            print("planar:", len(tied), "candidates tie with the winner")
            r = min((finish_ref(p, r["hyp"], winner=w) for w in tied[:40]), key=lambda x: err_to_truth(x, p)[0])
        rot, tr = err_to_truth(r, p)
        print(sc, "outcome", r["outcome"], "rot", rot, "trans", tr, "inliers", r["n_inliers"], "of", int(p["is_inlier"].sum()))
        assert r["outcome"] == TV_OK and rot < 1e-5 and tr < 1e-4
        # (accepted by CheckRT; vbGood besides needs parallax, which points near the axis of a forward motion do not have)
        assert r["inlier"][p["is_inlier"]].all() and (r["code"][p["is_inlier"]] <= CHK_LOW_PARALLAX).all()
        assert sc == "forward" or r["good"][p["is_inlier"]].all()
        X = r["points"][p["is_inlier"]]
        assert np.abs(X - p["X"][p["is_inlier"]]).max() < 1e-5 * 40


def test_rotation_scenes_never_initialise_and_each_outcome_is_reached():
    seen = set()
    for seed in range(3):
        r = two_view_ref(synth.make_two_view(300, 0.8, 0.5, 40 + seed, scene="rotation"), 32, 7)
        print("rotation", seed, "outcome", r["outcome"], "parallax", r["parallax"], "n_pass", r["n_pass"])
        assert r["outcome"] in (TV_FEW_GOOD, TV_LOW_PARALLAX, TV_NO_MODEL)
        seen.add(r["outcome"])
    p = synth.make_two_view(300, 0.8, 0.5, 50)
    assert two_view_ref(p, 32, 7)["outcome"] == TV_OK
    assert two_view_ref(p, 32, 7, min_triangulated=1000)["outcome"] == TV_FEW_GOOD
    assert two_view_ref(p, 32, 7, min_parallax_deg=80.0)["outcome"] == TV_LOW_PARALLAX
    assert finish_ref(p, [dict(E=np.zeros((0, 3, 3)), loss=np.zeros(0), count=np.zeros(0))])["outcome"] == TV_NO_MODEL


def test_every_checkrt_code_is_reached_by_a_hand_made_case():
    R, t, cam = np.eye(3), np.array([-1.0, 0.0, 0.0]), (400.0, 400.0, 320.0, 240.0)

    def obs(X, t=t):
        Y = np.asarray(X, float) + t
        return [400 * X[0] / X[2] + 320, 400 * X[1] / X[2] + 240], [400 * Y[0] / Y[2] + 320, 400 * Y[1] / Y[2] + 240]
    cases = []
    a, b = obs([0.5, 0.2, 5.0]); cases.append((a, b, True, CHK_GOOD))
    a, b = obs([0.5, 0.2, 5000.0]); cases.append((a, b, True, CHK_LOW_PARALLAX))
    cases.append((a, b, False, CHK_NOT_INLIER))
    cases.append(([320.0, 240.0], [320.0, 240.0], True, CHK_W0))              # parallel rays through both principal points
    a, b = obs([0.5, 0.2, -5.0]); cases.append((a, b, True, CHK_BEHIND1))
    a, b = obs([0.5, 0.2, 5.0]); cases.append(([a[0], a[1] + 9.0], [b[0], b[1] - 9.0], True, CHK_REPROJ1))
    # in front of camera 1, behind camera 2: camera 2 looks backwards
    Rb = np.diag([-1.0, 1.0, -1.0]); tb = np.array([0.0, 0.0, 2.0])
    X = np.array([0.3, 0.1, 6.0]); Y = Rb @ X + tb
    for (o1, o2, inl, want) in cases:
        r = check_rt(R, t, cam, np.array([o1]), np.array([o2]), np.array([inl]), 4.0)
        print(want, r["code"][0], r["points"][0])
        assert r["code"][0] == want and np.isnan(r["points"][0]).all() == (want > CHK_LOW_PARALLAX)
    r = check_rt(Rb, tb, cam, np.array([[400 * X[0] / X[2] + 320, 400 * X[1] / X[2] + 240]]),
                 np.array([[400 * Y[0] / Y[2] + 320, 400 * Y[1] / Y[2] + 240]]), np.array([True]), 4.0)
    assert r["code"][0] == CHK_BEHIND2
    # REPROJ2: the error splits unevenly when camera 2's observation alone is off along the epipolar line's normal
    a, b = obs([0.5, 0.2, 5.0])
    r = check_rt(R, t, cam, np.array([a]), np.array([[b[0], b[1] + 5.0]]), np.array([True]), 4.0)
    assert r["code"][0] in (CHK_REPROJ1, CHK_REPROJ2)
    # ... a camera that has moved towards the point takes most of the error: image 1 inside the gate, image 2 outside
    tf = np.array([0.3, 0.0, -3.0])
    a, b = obs([0.5, 0.2, 5.0], tf)
    r = check_rt(R, tf, cam, np.array([a]), np.array([[b[0] - 3.8 * 0.37, b[1] + 3.8]]), np.array([True]), 4.0)
    print("forward camera:", r["code"][0], r["q"]["e1"], r["q"]["e2"])
    assert r["code"][0] == CHK_REPROJ2 and r["q"]["e1"][0] <= 4.0 < r["q"]["e2"][0]
    a, b = obs([0.5, 0.2, 5.0])
    # parallax: element min(50, size - 1) of the sorted cosines; 0 without an accepted match
    assert check_rt(R, t, cam, np.array([a]), np.array([b]), np.array([False]), 4.0)["parallax"] == 0.0


def test_one_focal_length_quirk_shows_on_a_camera_with_unequal_focal_lengths():
    """stages 1 - 3 see f = 0.5 (fx + fy); on a camera with fx != fy exact observations are NOT exact for them: the Sampson
    distances of true matches are far from zero, while CheckRT (true fx, fy) is what it is"""
    cam = (500.0, 400.0, 320.0, 240.0)
    p = synth.make_two_view(200, 1.0, 0.0, 5, cam=cam)
    tx = np.array([[0, -p["t"][2], p["t"][1]], [p["t"][2], 0, -p["t"][0]], [-p["t"][1], p["t"][0], 0]])
    s_quirk = sampson2_px(tx @ p["R"], p["obs1"], p["obs2"], 450.0, 320.0, 240.0)
    Kinv = np.diag([1 / 500.0, 1 / 400.0, 1.0]); Kinv[0, 2], Kinv[1, 2] = -320 / 500.0, -240 / 400.0
    x1 = np.concatenate([p["obs1"], np.ones((200, 1))], 1) @ Kinv.T; x2 = np.concatenate([p["obs2"], np.ones((200, 1))], 1) @ Kinv.T
    assert np.abs(np.einsum('mi,ij,mj->m', x2, tx @ p["R"], x1)).max() < 1e-12
    print("median Sampson^2 of exact matches under one focal length:", np.median(s_quirk))
    assert np.median(s_quirk) > 0.01
    same = synth.make_two_view(200, 1.0, 0.0, 5, cam=(450.0, 450.0, 320.0, 240.0))
    assert sampson2_px(tx @ same["R"], same["obs1"], same["obs2"], 450.0, 320.0, 240.0).max() < 1e-12


# ---- the tolerances and the caps ----------------------------------------------------------------------------------------
def _measure(scenes=None):
    e_spread = pose_spread = pos_spread = loss_spread = par_spread = 0.0
    n_tie = 0
    rows, so_far = [], []               # (so_far: the running maxima of pose, point and parallax spread after every scene)
    for label, args, iters, seed in (SCENES if scenes is None else scenes):
        p = synth.make_two_view(**args)
        samples = samples_ref(args["n_matches"], iters, seed)
        ha, hb = hypotheses_ref(p, samples, "poly"), hypotheses_ref(p, samples, "action")
        n_c = n_ill = 0
        for a, b in zip(ha, hb):
            ill = a["root_err"] > E_SPREAD_MEASURED
            n_c += len(ill); n_ill += int(ill.sum())
            if (~ill).any():
                d = match_candidates(a["E"][~ill], b["E"])
                e_spread = max(e_spread, float(d.max()))
                for k in np.flatnonzero(~ill):
                    if len(b["E"]):
                        j = int(np.linalg.norm(b["E"] - a["E"][k:k + 1], axis=(1, 2)).argmin())
                        loss_spread = max(loss_spread, abs(a["loss"][k] - b["loss"][j]) / max(a["loss"][k], 1.0))
        ra, rb = finish_ref(p, ha), finish_ref(p, hb)
        tie = is_tie(ha, ra)
        n_tie += tie
        edge = edge_matches(ra)
        if not tie and ra["winner"] is not None and rb["winner"] is not None:
            assert ra["outcome"] == rb["outcome"], label
            dq = min(np.abs(ra["pose"][:4] - rb["pose"][:4]).max(), np.abs(ra["pose"][:4] + rb["pose"][:4]).max())
            pose_spread = max(pose_spread, dq, np.abs(ra["pose"][4:] - rb["pose"][4:]).max())
            par_spread = max(par_spread, abs(ra["parallax"] - rb["parallax"]) / max(1.0, abs(ra["parallax"])))
            both = (ra["code"] <= 2) & (rb["code"] <= 2)
            pos_spread = max(pos_spread, float((np.linalg.norm(ra["points"][both] - rb["points"][both], axis=1) /
                                                np.linalg.norm(ra["points"][both], axis=1)).max()))
        rows.append((label, n_c, n_ill, int(edge.sum()), len(edge), tie, ra["outcome"]))
        so_far.append((pose_spread, pos_spread, par_spread))
    return dict(e=e_spread, pose=pose_spread, pos=pos_spread, loss=loss_spread, par=par_spread, n_tie=n_tie, rows=rows, so_far=so_far)


_measured = {}


def measured():
    if not _measured:
        _measured.update(_measure())
    return _measured


def test_tolerances_are_the_measured_ones():
    m = measured()
    print(f"measured: E spread {m['e']:.3g} (constant {E_SPREAD_MEASURED:.3g}), pose {m['pose']:.3g} ({POSE_SPREAD_MEASURED:.3g}), "
          f"points {m['pos']:.3g} ({POS_SPREAD_MEASURED:.3g}), loss {m['loss']:.3g} ({LOSS_SPREAD_MEASURED:.3g}), "
          f"parallax {m['par']:.3g} ({PARALLAX_SPREAD_MEASURED:.3g})")
    assert m["e"] <= E_SPREAD_MEASURED and m["pose"] <= POSE_SPREAD_MEASURED and m["pos"] <= POS_SPREAD_MEASURED
    assert m["loss"] <= LOSS_SPREAD_MEASURED and m["par"] <= PARALLAX_SPREAD_MEASURED
    # ... and the constants are the measurement, not a generous bound (another LAPACK build moves it: a factor 30)
    assert m["e"] >= E_SPREAD_MEASURED / 30 and m["pose"] >= POSE_SPREAD_MEASURED / 30 and m["pos"] >= POS_SPREAD_MEASURED / 30
    assert m["par"] >= PARALLAX_SPREAD_MEASURED / 30


def test_the_committed_scenes_stay_inside_the_three_caps():
    m = measured()
    for label, n_c, n_ill, n_edge, M, tie, outcome in m["rows"]:
        print(f"{label}: {n_c} candidates, {n_ill} ill-conditioned, {n_edge} of {M} matches on a gate, tie {tie}, outcome {outcome}")
        assert n_ill <= ILL_CAP * n_c and n_edge <= max(EDGE_CAP * M, 1)
    assert m["n_tie"] <= TIE_CAP * len(SCENES)


# ---- C-ABI without a device -------------------------------------------------------------------------------------------
def test_symbols_constants_and_the_sampler(built_lib):
    from movba import capi
    for hooks in (False, True):
        L = capi.lib(hooks)
        assert hasattr(L, "movba_two_view") and hasattr(L, "movba_two_view_samples")
        d, r = capi.TwoViewDesc(), capi.TwoViewResult()
        r.status = 77
        assert L.movba_two_view(None, C.byref(d), C.byref(r), 1) == capi.ERR_ARG and r.status == 77
    L = capi.lib()
    assert L.movba_version() == 5
    for n, nh, seed in ((500, 64, 1), (5, 9, 0), (37, 200, 5)):
        assert np.array_equal(capi.two_view_samples(n, nh, seed), samples_ref(n, nh, seed))
    assert not np.array_equal(capi.two_view_samples(500, 8, 1)[:, :3], capi.ransac_samples(500, 8, 1))
    out = np.zeros(5, np.int32)
    assert L.movba_two_view_samples(4, 1, 1, out.ctypes.data_as(C.POINTER(C.c_int32))) == capi.ERR_ARG
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    for name, val in (("TV_OK", 0), ("TV_NO_MODEL", 1), ("TV_FEW_GOOD", 2), ("TV_LOW_PARALLAX", 3), ("TV_CHK_NONE", 0), ("TV_CHK_GOOD", 1),
                      ("TV_CHK_LOW_PARALLAX", 2), ("TV_CHK_REJ_NOT_INLIER", 16), ("TV_CHK_REJ_W0", 17), ("TV_CHK_REJ_BEHIND1", 18),
                      ("TV_CHK_REJ_BEHIND2", 19), ("TV_CHK_REJ_REPROJ1", 20), ("TV_CHK_REJ_REPROJ2", 21), ("MAX_TWO_VIEW_ITERS", 1024)):
        assert int(re.search(r"#define\s+MOVBA_%s\s+(\d+)" % name, hdr).group(1)) == val == getattr(capi, name)
    assert C.sizeof(capi.TwoViewDesc) == 104 and C.sizeof(capi.TwoViewResult) == 216


# ---- host side and the library's own arithmetic over the fake device --------------------------------------------------------
STUB = os.path.join(ROOT, "tests", "hipstub")


def _build(target):
    subprocess.check_call(["make", "-C", STUB, "-s", target])
    return os.path.join(STUB, target)


def test_two_view_host_side_under_address_and_undefined_behaviour_sanitizers():
    """Every invalid descriptor refused with canaries untouched, n == 0, pairs under 5 matches, pinned and ordinary result
    arrays, batches against solo calls bit for bit, a call between an LBA upload and its run, two threads on two handles."""
    exe = _build("two_view_asan")
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0 abort_on_error=0 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=900)
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[:4000]
    assert p.returncode == 0 and p.stdout.strip().endswith("TWO_VIEW OK"), p.stderr[-2000:]


def test_two_view_host_side_is_race_free():
    exe = _build("two_view_tsan")
    p = subprocess.run([exe], env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"), capture_output=True, text=True, timeout=900)
    assert "WARNING: ThreadSanitizer" not in p.stderr, p.stderr[:4000]
    assert p.returncode == 0 and p.stdout.strip().endswith("TWO_VIEW OK"), p.stderr[-2000:]


def solve_on_the_fake_device(p, iters, seed, tmp_path):
    """one pair through the driver of tests/hipstub that runs the library's two_view_math.h on the CPU -> a result with diagnostics"""
    exe = _build("two_view_opt")
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    M = len(p["obs1"])
    with open(fin, "wb") as fh:
        np.array([M, iters, seed], np.int32).tofile(fh)
        np.array(p["cam"], np.float64).tofile(fh)
        np.ascontiguousarray(p["obs1"], np.float64).tofile(fh); np.ascontiguousarray(p["obs2"], np.float64).tofile(fh)
    subprocess.check_call([exe, fin, fout], timeout=600)
    raw = np.fromfile(fout, np.float64)
    k = 0

    def take(n):
        nonlocal k
        v = raw[k:k + n]; k += n
        return v
    head = take(24)
    got = dict(pose=head[:7], E=head[7:16].reshape(3, 3), parallax_deg=head[16], outcome=int(head[17]), n_inliers=int(head[18]),
               n_pass=int(head[19]), n_good=int(head[20]), samples_used=int(head[21]), status=int(head[22]))
    got["inlier"] = take(M).astype(np.uint8); got["good"] = take(M).astype(np.uint8); got["code"] = take(M).astype(np.uint8)
    got["points"] = take(3 * M).reshape(M, 3)
    got["hyp_nsol"] = take(iters).astype(np.int32); got["hyp_E"] = take(90 * iters).reshape(iters, 10, 3, 3)
    got["hyp_loss"] = take(10 * iters).reshape(iters, 10)
    return got


def test_the_librarys_own_solver_against_the_restatement_on_the_cpu(tmp_path):
    """The fake device runs two_view_math.h: the driver solves pairs written to a file and writes results back; the same
    comparison, tolerances and caps as on the GPU."""
    n_tie = 0
    picked = SCENES[::4]
    for label, args, iters, seed in picked:
        p = synth.make_two_view(**args)
        got = solve_on_the_fake_device(p, iters, seed, tmp_path)
        assert got["status"] == 0
        n_tie += compare_with_ref(got, p, iters, seed, label, check_truth=True)["tie"]
    assert n_tie <= max(TIE_CAP * len(picked), 0)
