"""movba_triangulate without a GPU.

`triangulate_ref` is the yardstick of tests/test_gpu_triangulate.py: a numpy fp64 restatement of the loop body of
LocalMapping::CreateNewMapPoints (LocalMapping.cc:313-476), written from the reference text, null vector from numpy.linalg.svd.
It never calls the library.  This file checks the yardstick itself (noise-free recovery, every reachable code, one hand-made
case per quirk), MEASURES the position tolerance the GPU test uses, counts the matches that sit on a gate, and checks the
C-ABI's host side: symbols, argument checks, and triangulate.cpp under the sanitizers over the fake device of tests/hipstub.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

DLT, STEREO1, STEREO2 = 1, 2, 3
REJ_W0, REJ_PARALLAX, REJ_DEPTH, REJ_BEHIND1, REJ_BEHIND2, REJ_REPROJ1, REJ_REPROJ2, REJ_ZERO_DIST, REJ_FAR = range(16, 25)
ACCEPTED = (DLT, STEREO1, STEREO2)
CODE_NAMES = {1: "dlt", 2: "stereo1", 3: "stereo2", 16: "w0", 17: "parallax", 18: "depth", 19: "behind1", 20: "behind2",
              21: "reproj1", 22: "reproj2", 23: "zero_dist", 24: "far"}

# Position tolerance, relative to |X|: 10 x the largest spread of the restatement against ITSELF with the null vector taken
# two ways (SVD of A; eigh of A^T A) over the scenes of SCENES below.  Measured (test_position_tolerance_is_the_measured_one
# prints it): see POS_SPREAD_MEASURED.  The factor 10 covers a third algorithm - the device's one-sided Jacobi - with another
# rounding order.
POS_SPREAD_MEASURED = 1.22e-10      # (mono 1.14e-10, stereo 1.22e-10, mixed 5.3e-11; medians 1e-14, 99th percentiles 3e-13)
POS_TOL = 10 * POS_SPREAD_MEASURED
# the stereo parallax comparison (c1 < c2) does not depend on the point: its margin is the rounding of cos(2 atan2(b / 2, d))
# against the algebraic form (d^2 - a^2) / (d^2 + a^2) the device uses - a few ulp of 1
PARALLAX_MARGIN = 1e-13
EDGE_CAP = 1e-3         # at most 0.1 % of a scene's matches may sit on a gate

# the committed scenes: (label, make_triangulation arguments)
SCENES = [("mono 30 x 2000", dict(n_pairs=30, n_per_pair=2000, seed=7101)),
          ("stereo 30 x 2000", dict(n_pairs=30, n_per_pair=2000, seed=7102, stereo=True)),
          ("mixed 30 x 2000", dict(n_pairs=30, n_per_pair=2000, seed=7103, stereo=True, stereo_frac=0.5))]


def scene(args):
    return synth.make_triangulation(**args)


def _views(views):
    q = np.asarray(views["poses"], np.float64)[:, :4]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)
    t = np.asarray(views["poses"], np.float64)[:, 4:]
    O = -np.einsum('vji,vj->vi', R, t)
    nv = len(q)
    bf = np.asarray(views["bf"], np.float64) if views.get("bf") is not None else np.zeros(nv)
    b = np.asarray(views["b"], np.float64) if views.get("b") is not None else np.zeros(nv)
    return R, t, O, np.asarray(views["cam"], np.float64), bf, b


def _null_svd(A):
    return np.linalg.svd(A)[2][:, 3, :]


def _null_eigh(A):
    return np.linalg.eigh(np.einsum('mji,mjk->mik', A, A))[1][:, :, 0]


def tri_quantities(views, pairs, matches, null=_null_svd, c1_shift=0.0):
    """Every continuous quantity of the loop body, for all matches at once (NaN where the reference never computes it)."""
    R, t, O, cam, bf, b = _views(views)
    ptr = np.asarray(pairs["pair_ptr"], np.int64)
    M = int(ptr[-1]) if len(ptr) else 0
    pv = np.asarray(pairs["pair_view"], np.int64).reshape(-1, 2)
    pair = np.repeat(np.arange(len(pv)), np.diff(ptr))
    i1, i2 = pv[pair, 0], pv[pair, 1]
    o1, o2 = np.asarray(matches["obs1"], np.float64).reshape(-1, 2), np.asarray(matches["obs2"], np.float64).reshape(-1, 2)
    neg = np.full(M, -1.0)
    ur1 = np.asarray(matches["ur1"], np.float64) if matches.get("ur1") is not None else neg
    ur2 = np.asarray(matches["ur2"], np.float64) if matches.get("ur2") is not None else neg
    d1 = np.asarray(matches["depth1"], np.float64) if matches.get("depth1") is not None else neg
    d2 = np.asarray(matches["depth2"], np.float64) if matches.get("depth2") is not None else neg
    R1, R2, t1, t2, O1, O2, k1, k2 = R[i1], R[i2], t[i1], t[i2], O[i1], O[i2], cam[i1], cam[i2]
    with np.errstate(all="ignore"):
        # unprojectEig, rays, cosParallaxRays (:334-339)
        xn1 = np.stack([(o1[:, 0] - k1[:, 2]) / k1[:, 0], (o1[:, 1] - k1[:, 3]) / k1[:, 1], np.ones(M)], 1)
        xn2 = np.stack([(o2[:, 0] - k2[:, 2]) / k2[:, 0], (o2[:, 1] - k2[:, 3]) / k2[:, 1], np.ones(M)], 1)
        ray1 = np.einsum('mji,mj->mi', R1, xn1); ray2 = np.einsum('mji,mj->mi', R2, xn2)
        cos_rays = np.einsum('mi,mi->m', ray1, ray2) / (np.linalg.norm(ray1, axis=1) * np.linalg.norm(ray2, axis=1))
        st1, st2 = ur1 >= 0, ur2 >= 0
        # the if / else if at :345-348
        c1 = np.where(st1, np.cos(2 * np.arctan2(b[i1] / 2, d1)), cos_rays + 1) + c1_shift
        c2 = np.where(~st1 & st2, np.cos(2 * np.arctan2(b[i2] / 2, d2)), cos_rays + 1)
        use_dlt = ~st1 & ~st2
        use_s1 = ~use_dlt & st1 & (c1 < c2)
        use_s2 = ~use_dlt & ~use_s1 & st2 & (c2 < c1)
        # cv::triangulatePoints over normalised coordinates, P = [Rcw | tcw] (:365-376)
        P1 = np.concatenate([R1, t1[:, :, None]], 2); P2 = np.concatenate([R2, t2[:, :, None]], 2)
        A = np.stack([xn1[:, 0:1] * P1[:, 2] - P1[:, 0], xn1[:, 1:2] * P1[:, 2] - P1[:, 1],
                      xn2[:, 0:1] * P2[:, 2] - P2[:, 0], xn2[:, 1:2] * P2[:, 2] - P2[:, 1]], 1)
        xh = np.zeros((M, 4))
        if use_dlt.any():
            xh[use_dlt] = null(A[use_dlt])
        w = np.where(use_dlt, xh[:, 3], np.nan)
        X = np.full((M, 3), np.nan)
        ok = use_dlt & (w != 0)
        X[ok] = xh[ok, :3] / xh[ok, 3:4]

        # KeyFrame::UnprojectStereo (:382, :388)
        def unproject(o, k, d, Rv, Ov):
            xc = np.stack([(o[:, 0] - k[:, 2]) * d * (1.0 / k[:, 0]), (o[:, 1] - k[:, 3]) * d * (1.0 / k[:, 1]), d], 1)
            return np.einsum('mji,mj->mi', Rv, xc) + Ov
        s1ok, s2ok = use_s1 & (d1 > 0), use_s2 & (d2 > 0)
        X[s1ok] = unproject(o1, k1, d1, R1, O1)[s1ok]
        X[s2ok] = unproject(o2, k2, d2, R2, O2)[s2ok]
        Y1 = np.einsum('mij,mj->mi', R1, X) + t1; Y2 = np.einsum('mij,mj->mi', R2, X) + t2
        z1, z2 = Y1[:, 2], Y2[:, 2]

        def reproj(Y, k, o, st, ur, bf_used):
            z = Y[:, 2]; invz = 1.0 / z
            mono = (k[:, 0] * Y[:, 0] / z + k[:, 2] - o[:, 0]) ** 2 + (k[:, 1] * Y[:, 1] / z + k[:, 3] - o[:, 1]) ** 2
            u = k[:, 0] * Y[:, 0] * invz + k[:, 2]
            ster = (u - o[:, 0]) ** 2 + (k[:, 1] * Y[:, 1] * invz + k[:, 3] - o[:, 1]) ** 2 + (u - bf_used * invz - ur) ** 2
            return np.where(st, ster, mono)
        e1 = reproj(Y1, k1, o1, st1, ur1, bf[i1])
        e2 = reproj(Y2, k2, o2, st2, ur2, bf[i1])          # view 1's mbf, as the reference has it (:456)
        dist1 = np.linalg.norm(X - O1, axis=1); dist2 = np.linalg.norm(X - O2, axis=1)
    return dict(M=M, X=X, w=w, use_dlt=use_dlt, use_s1=use_s1, use_s2=use_s2, d1=d1, d2=d2, z1=z1, z2=z2, e1=e1, e2=e2,
                dist1=dist1, dist2=dist2, c1=c1, c2=c2, cos_rays=cos_rays, st1=st1, st2=st2, Y1=Y1, Y2=Y2, k1=k1, k2=k2, bf1=bf[i1])


GATES = (("w0", REJ_W0), ("behind1", REJ_BEHIND1), ("behind2", REJ_BEHIND2), ("reproj1", REJ_REPROJ1), ("reproj2", REJ_REPROJ2),
         ("zero", REJ_ZERO_DIST), ("far", REJ_FAR))


def tri_decide(q, reproj_gate, far_threshold, flip=None):
    """The reference's chain of `continue`s over the quantities; flip: name of ONE gate whose decision is inverted."""
    with np.errstate(all="ignore"):
        g = dict(w0=q["w"] == 0, behind1=q["z1"] <= 0, behind2=q["z2"] <= 0, reproj1=q["e1"] > reproj_gate,
                 reproj2=q["e2"] > reproj_gate, zero=(q["dist1"] == 0) | (q["dist2"] == 0),
                 far=(far_threshold > 0) & ((q["dist1"] >= far_threshold) | (q["dist2"] >= far_threshold)))
    if flip:
        g[flip] = ~g[flip]
    g["w0"] = g["w0"] & q["use_dlt"]
    code = np.where(q["use_dlt"], DLT, np.where(q["use_s1"], STEREO1, STEREO2)).astype(np.uint8)
    for name, c in reversed(GATES):                     # (reversed: an earlier gate overrides a later one)
        code = np.where(g[name], c, code).astype(np.uint8)
    # the rejects in front of the 3-D position
    depth_bad = (q["use_s1"] & ~(q["d1"] > 0)) | (q["use_s2"] & ~(q["d2"] > 0))
    code = np.where(depth_bad, REJ_DEPTH, code)
    code = np.where(~q["use_dlt"] & ~q["use_s1"] & ~q["use_s2"], REJ_PARALLAX, code)
    return code.astype(np.uint8)


def triangulate_ref(views, pairs, matches, reproj_gate=5.0, far_threshold=0.0, null=_null_svd):
    """-> dict(points (M, 3): NaN where no 3-D position was reached, code (M,), n_accepted, q: the quantities)"""
    q = tri_quantities(views, pairs, matches, null)
    code = tri_decide(q, reproj_gate, far_threshold)
    X = q["X"].copy()
    X[np.isin(code, (REJ_W0, REJ_PARALLAX, REJ_DEPTH))] = np.nan
    return dict(points=X, code=code, n_accepted=int(np.isin(code, ACCEPTED).sum()), q=q)


def edge_alternatives(views, pairs, matches, ref, reproj_gate, far_threshold, tol=None):
    """Which matches sit ON a gate, and which codes such a match may carry besides the restatement's.

    A point that is off by delta = tol * |X| moves the gated quantities by at most (first order, each bound written for the
    worst direction):
      depth      z = r3 . X + tz, |r3| = 1                                  |dz|    <= delta
      distance   |X - O|                                                    |ddist| <= delta
      residual   r = proj(Xc) - obs; |d proj / d Xc| <= G with
                 G = (sqrt(2) fmax (1 + rho) + bf / z) / z, rho = |(x, y)| / z   (pinhole Jacobian; the bf term is the stereo row)
                 e = |r|^2                                                  |de|    <= 2 sqrt(e) G delta + (G delta)^2
      w          the unit null vector's last component; X = xyz / w         on the edge when |w| <= tol
    A match is on the edge of a gate when its quantity is within that bound of the gate's threshold.  The stereo parallax
    comparison does not involve the point: its margin is PARALLAX_MARGIN.  -> (edge (M,) bool, list of (M,) code arrays)."""
    tol = POS_TOL if tol is None else tol
    q = ref["q"]
    with np.errstate(all="ignore"):
        delta = tol * np.linalg.norm(q["X"], axis=1)

        def G(Y, k, bfv):
            z = np.abs(Y[:, 2]); rho = np.hypot(Y[:, 0], Y[:, 1]) / z
            return (np.sqrt(2.0) * np.maximum(k[:, 0], k[:, 1]) * (1 + rho) + np.abs(bfv) / z) / z
        g1, g2 = G(q["Y1"], q["k1"], q["bf1"]) * delta, G(q["Y2"], q["k2"], q["bf1"]) * delta
        on = dict(w0=q["use_dlt"] & (np.abs(q["w"]) <= tol), behind1=np.abs(q["z1"]) <= delta, behind2=np.abs(q["z2"]) <= delta,
                  reproj1=np.abs(q["e1"] - reproj_gate) <= 2 * np.sqrt(q["e1"]) * g1 + g1 * g1,
                  reproj2=np.abs(q["e2"] - reproj_gate) <= 2 * np.sqrt(q["e2"]) * g2 + g2 * g2,
                  zero=(q["dist1"] <= delta) | (q["dist2"] <= delta),
                  far=(far_threshold > 0) & ((np.abs(q["dist1"] - far_threshold) <= delta) | (np.abs(q["dist2"] - far_threshold) <= delta)))
        par = ~q["use_dlt"] & (np.abs(q["c1"] - q["c2"]) <= PARALLAX_MARGIN)
    # only gates the match actually REACHES count (an accepted match reached all; a rejected one those up to its own)
    code = ref["code"]
    has_pos = ~np.isin(code, (REJ_PARALLAX, REJ_DEPTH))
    reached_upto = np.where(np.isin(code, ACCEPTED), 255, code)
    edge = par.copy()
    alts = []
    for name, c in GATES:
        e = on[name] & has_pos & (c <= reached_upto)
        edge |= e
        alts.append(np.where(e, tri_decide(q, reproj_gate, far_threshold, flip=name), code))
    if par.any():
        for shift in (2 * PARALLAX_MARGIN, -2 * PARALLAX_MARGIN):
            q2 = tri_quantities(views, pairs, matches, c1_shift=shift)
            alts.append(np.where(par, tri_decide(q2, reproj_gate, far_threshold), code))
    return edge, alts


def compare_with_ref(got, sc, label="", lost_w=False):
    """What tests/test_gpu_triangulate.py asserts of a result against the restatement (returns the figures it printed)."""
    ref = triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
    edge, alts = edge_alternatives(sc["views"], sc["pairs"], sc["matches"], ref, sc["reproj_gate"], sc["far_threshold"])
    M = ref["q"]["M"]
    # the cap is a condition on the SCENE, asserted on the restatement alone before the result is looked at (scenes below
    # 1 000 matches may hold one such match)
    assert edge.sum() <= max(EDGE_CAP * M, 1), (label, int(edge.sum()))
    # lost_w (off unless asked for; tests/test_gpu_general_position.py asks): a DLT match whose unit null vector has |w| <= POS_TOL has
    # no position - X = xyz / w moves by |dw / w| >= 1 under an error of POS_TOL in w, and with the sign of w goes behind the cameras
    # or beyond every distance.  The synthetic scenes hold one such match, the hand-placed w = 0 case: exactly 0 - REJ_W0 and NaN
    # on both sides - where view 1 has the identity rotation, 1e-17 and a position of 1e17 m in a rotated world frame.  There, at
    # most one per scene, neither its position nor which of the gates behind w0 rejects it is compared.
    w_lost = ref["q"]["use_dlt"] & (np.abs(ref["q"]["w"]) <= POS_TOL) if lost_w else np.zeros(M, bool)
    assert w_lost.sum() <= max(EDGE_CAP * M, 1), (label, int(w_lost.sum()))
    code = np.asarray(got["code"])
    same = code == ref["code"]
    allowed = same | (w_lost & ~np.isin(code, ACCEPTED))
    for a in alts:
        allowed |= edge & (code == a)
    n_diff = int((~same).sum())
    with np.errstate(all="ignore"):
        rel = np.linalg.norm(np.asarray(got["points"]) - ref["points"], axis=1) / np.linalg.norm(ref["points"], axis=1)
    cmp_pos = same & ~np.isnan(ref["points"][:, 0]) & ~w_lost
    worst = float(rel[cmp_pos].max()) if cmp_pos.any() else 0.0
    print(f"{label}: {M} matches, {int(edge.sum())} on an edge, {n_diff} codes differ, worst relative position error {worst:.3g} "
          f"(POS_TOL {POS_TOL:.3g}), accepted {got['n_accepted']} (restatement {ref['n_accepted']})")
    assert allowed.all(), (label, np.flatnonzero(~allowed)[:10], code[~allowed][:10], ref["code"][~allowed][:10])
    assert worst <= POS_TOL, (label, worst)
    nan_ref = np.isnan(ref["points"]).any(1)
    assert np.array_equal(np.isnan(np.asarray(got["points"])).any(1)[same], nan_ref[same]), label
    assert got["n_accepted"] == int(np.isin(code, ACCEPTED).sum()), label
    return dict(M=M, edge=int(edge.sum()), n_diff=n_diff, worst=worst)


# ---- the yardstick itself --------------------------------------------------------------------------------------------
def test_restatement_recovers_noise_free_points():
    sc = synth.make_triangulation(6, 500, 7001, mismatch_frac=0.0, special_frac=0.0, noise=False, far_threshold=0.0)
    # (the scene's observations are rounded to float32: take them back to exact projections of the truth)
    R, t, O, cam, bf, b = _views(sc["views"])
    v2 = np.repeat(sc["pairs"]["pair_view"][:, 1], np.diff(sc["pairs"]["pair_ptr"]))
    for key, idx in (("obs1", np.zeros_like(v2)), ("obs2", v2)):
        Y = np.einsum('mij,mj->mi', R[idx], sc["truth"]) + t[idx]
        sc["matches"][key] = np.stack([cam[idx, 0] * Y[:, 0] / Y[:, 2] + cam[idx, 2], cam[idx, 1] * Y[:, 1] / Y[:, 2] + cam[idx, 3]], 1)
    r = triangulate_ref(sc["views"], sc["pairs"], sc["matches"], 5.0, 0.0)
    rel = np.linalg.norm(r["points"] - sc["truth"], axis=1) / np.linalg.norm(sc["truth"], axis=1)
    print("noise-free recovery: max relative error", rel[1:].max())
    # (match 0 is the scene's w = 0 case; rounding x the conditioning of a 0.2 m baseline at 30 m)
    assert (r["code"][1:] == DLT).all() and rel[1:].max() < 1e-9


def test_every_reachable_code_occurs_on_the_synthetic_scenes():
    """ZERO_DIST cannot occur: a point in camera centre O has depth r3 . O + tz = 0 in that camera and is rejected as 'behind'
    first (in the reference too); every other code does."""
    seen = set()
    for label, args in SCENES:
        sc = scene(args)
        r = triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
        counts = {CODE_NAMES[c]: int(n) for c, n in zip(*np.unique(r["code"], return_counts=True))}
        print(label, counts)
        seen |= set(np.unique(r["code"]).tolist())
        assert r["n_accepted"] > 0.6 * r["q"]["M"]
    assert seen == set(CODE_NAMES) - {REJ_ZERO_DIST}, sorted(set(CODE_NAMES) - seen)


def _one(poses, cam, obs1, obs2, bf=None, b=None, ur1=None, ur2=None, d1=None, d2=None, gate=5.0, far=0.0):
    views = dict(poses=np.array(poses, float), cam=np.array(cam, float))
    if bf is not None:
        views.update(bf=np.array(bf, float), b=np.array(b, float))
    m = dict(obs1=np.array([obs1], float), obs2=np.array([obs2], float))
    for k, a in (("ur1", ur1), ("ur2", ur2), ("depth1", d1), ("depth2", d2)):
        if a is not None:
            m[k] = np.array([a], float)
    pairs = dict(pair_view=np.array([[0, 1]], np.int32), pair_ptr=np.array([0, 1], np.int32))
    return dict(views=views, pairs=pairs, matches=m, reproj_gate=gate, far_threshold=far), triangulate_ref(views, pairs, m, gate, far)


CAM2 = [[320, 320, 320, 240]] * 2
POSES2 = [[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, -0.5, 0, 0]]          # view 2's centre at x = +0.5


def _proj(X, pose, cam):
    Y = np.array(X, float) + np.array(pose[4:], float)
    return [cam[0] * Y[0] / Y[2] + cam[2], cam[1] * Y[1] / Y[2] + cam[3]], Y[2]


def quirk_cases():
    """(label, scene of one match, expected code): the hand-made cases, also run on the device by the GPU test"""
    X = [0.3, -0.2, 8.0]
    (o1, z1), (o2, z2) = _proj(X, POSES2[0], CAM2[0]), _proj(X, POSES2[1], CAM2[1])
    Xb = [0.3, -0.2, -8.0]
    (o1b, _), (o2b, _) = _proj(Xb, POSES2[0], CAM2[0]), _proj(Xb, POSES2[1], CAM2[1])
    wide1, wide2 = [-200.0, 240.0], [900.0, 240.0]
    st = dict(bf=[40, 40], b=[0.125, 0.125])
    out = []
    for bf1, want in ((40.0, STEREO2), (80.0, REJ_REPROJ2)):
        out.append((f"view 2 stereo residual with view 1's bf = {bf1}",
                    _one(POSES2, CAM2, o1, o2, bf=[bf1, 40.0], b=[bf1 / 320, 0.125], ur1=-1.0, d1=-1.0, ur2=o2[0] - 40.0 / z2, d2=z2), want))
    out.append(("both stereo, rays wide apart: un-projected from view 2",
                _one(POSES2, CAM2, wide1, wide2, ur1=wide1[0] + 204.0, d1=10.0, ur2=wide2[0] - 4e-4, d2=1e5, **st), None))
    out.append(("view 2 stereo only", _one(POSES2, CAM2, [330.0, 240.0], [310.0, 240.0], ur1=-1.0, d1=-1.0, ur2=305.0, d2=8.0, **st), None))
    out.append(("view 1 stereo only, rays wide apart", _one(POSES2, CAM2, wide1, wide2, ur1=wide1[0] + 204.0, d1=10.0, ur2=-1.0, d2=-1.0, **st), REJ_PARALLAX))
    out.append(("plain DLT", _one(POSES2, CAM2, o1, o2), DLT))
    out.append(("far", _one(POSES2, CAM2, o1, o2, far=5.0), REJ_FAR))
    out.append(("behind view 1", _one(POSES2, CAM2, o1b, o2b), REJ_BEHIND1))
    out.append(("parallel rays through both principal points", _one(POSES2, CAM2, [320.0, 240.0], [320.0, 240.0]), REJ_W0))
    out.append(("stereo depth zero", _one(POSES2, CAM2, o1, o2, ur1=o1[0] - 5.0, d1=0.0, ur2=-1.0, d2=-1.0, **st), REJ_DEPTH))
    return out


def test_hand_made_cases_one_per_quirk():
    cases = {label: (sc, r, want) for label, (sc, r), want in quirk_cases()}
    for label, (sc, r, want) in cases.items():
        print(label, CODE_NAMES[int(r["code"][0])], r["points"][0])
        if want is not None:
            assert r["code"][0] == want, label
    X = [0.3, -0.2, 8.0]
    # view 2's stereo residual subtracts VIEW 1's bf (:456): the observation is consistent with view 2's own bf = 40 and
    # passes when view 1 has the same, fails when view 1's is 80; the point itself is the same
    for key in ("view 2 stereo residual with view 1's bf = 40.0", "view 2 stereo residual with view 1's bf = 80.0"):
        assert np.allclose(cases[key][1]["points"][0], X, atol=1e-9)
    # both stereo: view 2's parallax is never evaluated (its cosine stays cosParallaxRays + 1); with rays more than 90 degrees
    # apart that number is below view 1's cosine and the point is un-projected from VIEW 2, whose own cosine (depth 1e5 m)
    # would never have been the smaller one
    q = cases["both stereo, rays wide apart: un-projected from view 2"][1]["q"]
    assert q["c2"][0] == q["cos_rays"][0] + 1 and q["c2"][0] < q["c1"][0] and q["use_s2"][0]
    assert np.cos(2 * np.arctan2(0.0625, 1e5)) > q["c1"][0]
    # view 1 mono, view 2 stereo: now view 2's parallax IS evaluated and decides
    q = cases["view 2 stereo only"][1]["q"]
    assert q["use_s2"][0] and abs(q["c2"][0] - np.cos(2 * np.arctan2(0.0625, 8.0))) < 1e-15
    for key in ("plain DLT", "far", "behind view 1"):
        assert np.isfinite(cases[key][1]["points"][0]).all()
    for key in ("view 1 stereo only, rays wide apart", "parallel rays through both principal points", "stereo depth zero"):
        assert np.isnan(cases[key][1]["points"][0]).all()


# ---- the tolerance and the edge count ---------------------------------------------------------------------------------
def test_position_tolerance_is_the_measured_one():
    worst = 0.0
    for label, args in SCENES:
        sc = scene(args)
        a = triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
        bq = tri_quantities(sc["views"], sc["pairs"], sc["matches"], null=_null_eigh)
        ok = a["q"]["use_dlt"] & ~np.isnan(a["points"][:, 0]) & ~np.isnan(bq["X"][:, 0])
        if not ok.any():
            continue
        rel = np.linalg.norm(a["q"]["X"][ok] - bq["X"][ok], axis=1) / np.linalg.norm(a["q"]["X"][ok], axis=1)
        print(f"{label}: SVD against eigh(A^T A) over {int(ok.sum())} DLT points: median {np.median(rel):.2g}, "
              f"99th percentile {np.percentile(rel, 99):.2g}, max {rel.max():.3g}")
        worst = max(worst, float(rel.max()))
    print(f"measured spread {worst:.3g}; POS_SPREAD_MEASURED {POS_SPREAD_MEASURED:.3g}; POS_TOL {POS_TOL:.3g}")
    # the constant is the measurement (another LAPACK build moves it: within a factor 3 either way)
    assert POS_SPREAD_MEASURED / 3 <= worst <= POS_SPREAD_MEASURED * 3


def test_at_most_a_thousandth_of_a_scene_sits_on_a_gate():
    for label, args in SCENES:
        sc = scene(args)
        ref = triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
        edge, _ = edge_alternatives(sc["views"], sc["pairs"], sc["matches"], ref, sc["reproj_gate"], sc["far_threshold"])
        print(f"{label}: {int(edge.sum())} of {ref['q']['M']} matches on an edge at POS_TOL {POS_TOL:.3g}")
        assert edge.sum() <= EDGE_CAP * ref["q"]["M"]


# ---- C-ABI without a device -------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_refuses_null(built_lib):
    for hooks in (False, True):
        L = built_lib.lib(hooks)
        assert hasattr(L, "movba_triangulate")
        d, r = built_lib.TriDesc(), built_lib.TriResult()
        r.status = 77
        assert L.movba_triangulate(None, C.byref(d), C.byref(r)) == built_lib.ERR_ARG and r.status == 77
    L = built_lib.lib()
    assert L.movba_triangulate(None, None, None) == built_lib.ERR_ARG
    assert [L.movba_status_string(s).decode() for s in (0, -1, -2)] == [built_lib.status_string(s) for s in (0, -1, -2)]
    assert L.movba_version() == 5
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    for name, val in (("DLT", DLT), ("STEREO1", STEREO1), ("STEREO2", STEREO2), ("REJ_W0", 16), ("REJ_PARALLAX", 17), ("REJ_DEPTH", 18),
                      ("REJ_BEHIND1", 19), ("REJ_BEHIND2", 20), ("REJ_REPROJ1", 21), ("REJ_REPROJ2", 22), ("REJ_ZERO_DIST", 23), ("REJ_FAR", 24)):
        assert int(re.search(r"#define\s+MOVBA_TRI_%s\s+(\d+)" % name, hdr).group(1)) == val == getattr(built_lib, "TRI_" + name)


# ---- host side under the sanitizers ------------------------------------------------------------------------------------
STUB = os.path.join(ROOT, "tests", "hipstub")


def _build_and_run(target, env):
    subprocess.check_call(["make", "-C", STUB, "-s", target])
    return subprocess.run([os.path.join(STUB, target)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)


def test_triangulate_host_side_under_address_and_undefined_behaviour_sanitizers():
    """Every invalid descriptor is refused before anything is written; calls that grow and shrink (staging buffer and device
    scratch regrown between them), pinned and ordinary result arrays, empty pairs; a call between an LBA upload and its run
    leaves the run's results unchanged; two threads on two handles.  The fake device runs the library's own per-match
    arithmetic (triangulate_math.h) on the CPU, so the driver also checks recovered points and codes."""
    p = _build_and_run("triangulate_asan", {"ASAN_OPTIONS": "detect_leaks=0 abort_on_error=0 exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[:4000]
    assert p.returncode == 0 and p.stdout.strip().endswith("TRIANGULATE OK"), p.stderr[-2000:]


def test_triangulate_host_side_is_race_free():
    p = _build_and_run("triangulate_tsan", {"TSAN_OPTIONS": "halt_on_error=0 exitcode=66"})
    assert "WARNING: ThreadSanitizer" not in p.stderr, p.stderr[:4000]
    assert p.returncode == 0 and p.stdout.strip().endswith("TRIANGULATE OK"), p.stderr[-2000:]
