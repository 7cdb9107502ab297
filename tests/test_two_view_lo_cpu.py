"""movba_two_view_lo without a GPU.

`two_view_lo_ref` is the yardstick of tests/test_gpu_two_view_lo.py: the numpy restatement of movba_two_view
(test_two_view_cpu.two_view_ref) with stage 2b of include/movba.h - the local optimisation of the winner - restated by its
rules on top, in two variants that share no code on the points where an implementation can go wrong:
    A  the "poly" hypothesis stage, the analytic Jacobian of the signed Sampson distance;
    B  the "action" hypothesis stage, a central-difference Jacobian through the parametrisation itself.
The refined E enters finish_ref as one extra hypothesis with the winner forced.  This file checks the restatement's own
properties, MEASURES the tolerances of the GPU test from the spread of the two variants, runs the library's arithmetic
(two_view_math.h) serially on the CPU through tests/two_view_lo/lo_main.cpp - plainly and under the sanitizers - and the
host side of the new entry point over the fake device of tests/hipstub (tests/two_view_lo/lo_host_driver.cpp).
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

import test_two_view_cpu as T  # noqa: E402

LO_ITERS = 10           # the setting examined
MAX_LO_ITERS = 32
# pairs around the sizes at which k_tv_lo's thread-strided loop changes shape: one wave, one workgroup, +- 1
SMALL = [(f"small {n}", dict(n_matches=n, inlier_frac=0.8, noise_px=0.5, seed=8600 + n, scene="general"), 32, 7)
         for n in (5, 6, 37, 63, 64, 65, 255, 256, 257)]
PAIRS = T.SCENES + SMALL

# ---- measured constants (test_lo_tolerances_are_the_measured_ones prints them and fails if they are below what it measures) ----
# largest differences between variants A and B on the committed pairs that are not tie pairs: canonical-E distance of the
# refined E, relative difference of loss0 / loss, pose (quaternion and unit translation, component-wise), points (relative),
# parallax (degrees, relative to max(1, parallax))
E_LO_SPREAD_MEASURED = 4.8e-11
LOSS_LO_SPREAD_MEASURED = 2.8e-10
POSE_LO_SPREAD_MEASURED = 3.2e-11
POS_LO_SPREAD_MEASURED = 5.4e-10
PARALLAX_LO_SPREAD_MEASURED = 1.1e-10
E_LO_TOL, LOSS_LO_TOL, POSE_LO_TOL = 10 * E_LO_SPREAD_MEASURED, 10 * LOSS_LO_SPREAD_MEASURED, 10 * POSE_LO_SPREAD_MEASURED
POS_LO_TOL, PARALLAX_LO_TOL = 10 * POS_LO_SPREAD_MEASURED, 10 * PARALLAX_LO_SPREAD_MEASURED


# ---- stage 2b restated -----------------------------------------------------------------------------------------------
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def start_ref(E0):
    """rule 1: (R, t) of E0 - the rotation with the larger trace (the first on equal traces); <[t]x R, E0> >= 0"""
    U, _, Vt = np.linalg.svd(E0)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    R = R2 if np.trace(R2) > np.trace(R1) else R1
    if ((skew(t) @ R) * E0).sum() < 0:
        t = -t
    return R, t


def tangent_ref(t):
    k = int(np.argmin(np.abs(t)))                        # (the lowest index on a tie)
    b1 = np.cross(t, np.eye(3)[k]); b1 = b1 / np.linalg.norm(b1)
    return b1, np.cross(t, b1)


def exp_so3(w):
    """exp([w]x) by its power series (the library uses Rodrigues' formula)"""
    K = skew(w)
    out, term = np.eye(3), np.eye(3)
    for n in range(1, 30):
        term = term @ K / n
        out = out + term
    return out


def step_ref(R, t, delta):
    """rule 2"""
    b1, b2 = tangent_ref(t)
    tn = t + delta[3] * b1 + delta[4] * b2
    return exp_so3(delta[:3]) @ R, tn / np.linalg.norm(tn)


def _px(pair):
    fx, fy, cx, cy = pair["cam"]
    f = 0.5 * (fx + fy)
    o1, o2 = np.asarray(pair["obs1"], float), np.asarray(pair["obs2"], float)
    Kinv = np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]])
    return Kinv, np.concatenate([o1, np.ones((len(o1), 1))], 1), np.concatenate([o2, np.ones((len(o2), 1))], 1)


def signed_sampson_px(E, px, dE=None):
    """rule 3 in pixels through F = K_f^-T E K_f^-1 -> r (M,), and with dE (5 matrices) its exact Jacobian (M, 5)"""
    Kinv, p1, p2 = px
    F = Kinv.T @ E @ Kinv
    Fp1, Ftp2 = p1 @ F.T, p2 @ F
    num = np.einsum('mi,mi->m', p2, Fp1)
    with np.errstate(all="ignore"):
        den = Fp1[:, 0] ** 2 + Fp1[:, 1] ** 2 + Ftp2[:, 0] ** 2 + Ftp2[:, 1] ** 2
        s = np.sqrt(den)
        r = num / s
        if dE is None:
            return r
        J = np.zeros((len(p1), 5))
        for j in range(5):
            G = Kinv.T @ dE[j] @ Kinv
            Gp1, Gtp2 = p1 @ G.T, p2 @ G
            dnum = np.einsum('mi,mi->m', p2, Gp1)
            dden = 2 * (Fp1[:, 0] * Gp1[:, 0] + Fp1[:, 1] * Gp1[:, 1] + Ftp2[:, 0] * Gtp2[:, 0] + Ftp2[:, 1] * Gtp2[:, 1])
            J[:, j] = dnum / s - num * dden / (2 * s ** 3)
    return r, J


def magsac_weight(r2, gate):
    """sigma-consensus++ weight of squared residuals, w / w(0); 0 beyond the gate (the weight beside test_two_view_cpu.magsac_loss)"""
    k2 = 9.210340371976184; xk = 0.5 * k2; sq_pi = math.sqrt(math.pi)
    s2 = gate / k2
    g_k = sq_pi * math.erfc(math.sqrt(xk))
    w0 = sq_pi * (1.0 - math.erfc(math.sqrt(xk)))
    r2 = np.asarray(r2, float)
    with np.errstate(all="ignore"):
        inside = r2 <= gate
    w = sq_pi * T._erfc(np.sqrt(np.where(inside, r2, 0.0) / (2 * s2))) - g_k
    return np.where(inside & (w > 0), w / w0, 0.0)


def loss_ref(r, gate):
    with np.errstate(all="ignore"):
        r2 = np.where(np.isfinite(r), r * r, np.inf)            # (a residual that is not a number scores 1, as beyond the gate)
    return float(T.magsac_loss(r2, gate).sum())


def chol_solve_ref(H, g):
    """-H^-1 g by Cholesky, None when a pivot is not positive and finite"""
    L = np.zeros((5, 5))
    for j in range(5):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0 and np.isfinite(d)):
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 5):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    with np.errstate(all="ignore"):
        return np.linalg.solve(L.T, np.linalg.solve(L, -g))


def refit_ref(pair, E0, lo_iters, jac="analytic", threshold=1.0):
    """rules 1 - 5 -> dict(E, E0, trace (the L_k), kept, steps, loss0, loss)"""
    px = _px(pair)
    gate = threshold ** 2
    R, t = start_ref(E0)
    E = E0
    trace, Es, steps = [], [E0], 0
    for k in range(lo_iters + 1):
        if jac == "analytic":
            b1, b2 = tangent_ref(t)
            dE = [skew(t) @ skew(np.eye(3)[a]) @ R for a in range(3)] + [skew(b1) @ R, skew(b2) @ R]
            r, J = signed_sampson_px(E, px, dE)
        else:
            r = signed_sampson_px(E, px)
            J = np.zeros((len(r), 5))
            h = 1e-6
            for j in range(5):
                d = np.zeros(5); d[j] = h
                Rp, tp = step_ref(R, t, d); Rm, tm = step_ref(R, t, -d)
                with np.errstate(all="ignore"):
                    J[:, j] = (signed_sampson_px(skew(tp) @ Rp, px) - signed_sampson_px(skew(tm) @ Rm, px)) / (2 * h)
        trace.append(loss_ref(r, gate))
        if k == lo_iters:
            break
        with np.errstate(all="ignore"):
            w = magsac_weight(np.where(np.isfinite(r), r * r, np.inf), gate)
        use = w > 0
        Jw = J[use] * w[use, None]
        delta = chol_solve_ref(Jw.T @ J[use], Jw.T @ r[use])
        if delta is None:
            break
        with np.errstate(all="ignore"):
            R, t = step_ref(R, t, delta)
            E = skew(t) @ R
        Es.append(E)
        steps = k + 1
    kept, best = 0, trace[0]
    for k in range(1, len(trace)):
        if trace[k] < best:                              # (the lowest k on a tie; a NaN is never kept)
            kept, best = k, trace[k]
    Ek = Es[kept]
    if kept and (Ek * E0).sum() < 0:
        Ek = -Ek
    return dict(E=Ek, E0=E0, trace=np.array(trace), kept=kept, steps=steps, loss0=trace[0], loss=best)


_hyp_cache = {}


def hypotheses_of(label, args, iters, seed, variant):
    key = (label, variant)
    if key not in _hyp_cache:
        p = synth.make_two_view(**args)
        hyp = T.hypotheses_ref(p, T.samples_ref(args["n_matches"], iters, seed), "poly" if variant == "A" else "action")
        _hyp_cache[key] = (p, hyp, T.finish_ref(p, hyp))
    return _hyp_cache[key]


_ref_cache = {}


def two_view_lo_ref(label, args, iters, seed, lo_iters=LO_ITERS, variant="A"):
    """rules 1 - 6: the restatement of movba_two_view_lo's result for one of PAIRS (or any pair given the same way)"""
    key = (label, lo_iters, variant)
    if key in _ref_cache:
        return _ref_cache[key]
    p, hyp, ref0 = hypotheses_of(label, args, iters, seed, variant)
    if ref0["winner"] is None:
        res = dict(ref0, hyp=hyp, ref0=ref0, pair=p, kept=0, steps=0, loss0=0.0, loss=0.0, E0=np.zeros((3, 3)), trace=np.zeros(1))
    else:
        E0 = hyp[ref0["winner"][0]]["E"][ref0["winner"][1]]
        fit = refit_ref(p, E0, lo_iters, "analytic" if variant == "A" else "numeric")
        extra = dict(E=fit["E"][None], root_err=np.zeros(1), loss=np.array([fit["loss"]]), count=np.zeros(1, int))
        res = T.finish_ref(p, hyp + [extra], winner=(len(hyp), 0))
        res.update(fit, hyp=hyp, ref0=ref0, pair=p, samples_used=ref0["samples_used"])
    _ref_cache[key] = res
    return res


def runner_up_gap(trace, kept):
    """how far the second-lowest L_k lies above the kept one, relative (inf: there is no other)"""
    rest = np.delete(np.asarray(trace, float), kept)
    rest = rest[np.isfinite(rest)]
    return float((rest.min() - trace[kept]) / max(trace[kept], 1.0)) if len(rest) else float("inf")


def compare_lo_with_ref(got, label, args, iters, seed, lo_iters, check_truth=False):
    """What tests/test_gpu_two_view_lo.py asserts of a movba_two_view_lo result (with lo_* keys) against the restatement:
    compare_with_ref's rules for a pair - tie pairs set aside under TIE_CAP, matches on a gate under EDGE_CAP - at the
    tolerances measured here."""
    ref = two_view_lo_ref(label, args, iters, seed, lo_iters)
    p = ref["pair"]
    tie = T.is_tie(ref["hyp"], ref["ref0"])
    edge = T.edge_matches(ref)
    assert edge.sum() <= max(T.EDGE_CAP * len(edge), 1), (label, int(edge.sum()))
    print(f"{label}: outcome {got['outcome']} (restatement {ref['outcome']}), tie {tie}, {int(edge.sum())} matches on a gate, "
          f"kept {got['lo_kept']} / {ref['kept']}, steps {got['lo_steps']} / {ref['steps']}, loss {got['loss0']:.6g} -> {got['loss']:.6g} "
          f"(restatement {ref['loss0']:.6g} -> {ref['loss']:.6g}), n_inliers {got['n_inliers0']} -> {got['n_inliers']} / {ref['n_inliers']}")
    assert got["n_inliers"] >= got["n_pass"] == int(np.asarray(got["inlier"]).sum())
    assert got["n_good"] == int((np.asarray(got["code"]) <= T.CHK_LOW_PARALLAX).sum() if got["outcome"] != T.TV_NO_MODEL else 0)
    assert np.array_equal(np.asarray(got["good"]) != 0, np.asarray(got["code"]) == T.CHK_GOOD)
    assert got["loss"] <= got["loss0"] and 0 <= got["lo_kept"] <= got["lo_steps"] <= lo_iters
    if not tie:
        assert got["samples_used"] == ref["samples_used"] and got["outcome"] == ref["outcome"], label
        if ref["winner"] is not None:
            de0 = T.match_candidates(ref["E0"][None], got["E0"][None])[0]
            de = T.match_candidates(ref["E"][None], got["E"][None])[0]
            dl0 = abs(got["loss0"] - ref["loss0"]) / max(ref["loss0"], 1.0)
            dl = abs(got["loss"] - ref["loss"]) / max(ref["loss"], 1.0)
            print(f"{label}: E0 distance {de0:.3g} (E_TOL {T.E_TOL:.3g}), E distance {de:.3g} (E_LO_TOL {E_LO_TOL:.3g}), "
                  f"loss0 difference {dl0:.3g}, loss difference {dl:.3g} (LOSS_LO_TOL {LOSS_LO_TOL:.3g})")
            assert de0 <= T.E_TOL and de <= E_LO_TOL and dl0 <= LOSS_LO_TOL and dl <= LOSS_LO_TOL, label
            if runner_up_gap(ref["trace"], ref["kept"]) > LOSS_LO_TOL:
                assert got["lo_kept"] == ref["kept"], label
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
            print(f"{label}: pose difference {max(dq, dt):.3g} (POSE_LO_TOL {POSE_LO_TOL:.3g}), worst relative point difference {wp:.3g} "
                  f"(POS_LO_TOL {POS_LO_TOL:.3g})")
            assert max(dq, dt) <= POSE_LO_TOL and wp <= POS_LO_TOL, label
            assert abs(got["n_inliers"] - ref["n_inliers"]) <= edge.sum() and abs(got["n_good"] - ref["n_good"]) <= edge.sum(), label
            assert abs(got["n_pass"] - ref["n_pass"]) <= edge.sum(), label
            dpar = abs(got["parallax_deg"] - ref["parallax"]) / max(1.0, abs(ref["parallax"]))
            print(f"{label}: parallax difference {dpar:.3g} (PARALLAX_LO_TOL {PARALLAX_LO_TOL:.3g})")
            assert dpar <= PARALLAX_LO_TOL or T.parallax_on_edge(ref, edge), label
    if check_truth:
        g = dict(R=T.q2R(got["pose"][:4]), t=got["pose"][4:]) if got["outcome"] != T.TV_NO_MODEL else {}
        (gr, gt), (rr, rt) = T.err_to_truth(g, p), T.err_to_truth(ref, p)
        print(f"{label}: error to truth: rotation {gr:.4g} deg (restatement {rr:.4g}), translation direction {gt:.4g} deg (restatement {rt:.4g})")
        assert gr <= 1.5 * rr and gt <= 1.5 * rt, label
    return dict(tie=tie, ref=ref)


# ---- the restatement itself ------------------------------------------------------------------------------------------
def test_the_analytic_jacobian_is_the_derivative_of_the_parametrisation():
    p = synth.make_two_view(60, 1.0, 0.5, 3)
    E0 = T._canon(skew(p["t"]) @ p["R"])[0]
    R, t = start_ref(E0)
    b1, b2 = tangent_ref(t)
    assert abs(b1 @ t) < 1e-15 and abs(b2 @ t) < 1e-15 and abs(np.linalg.norm(b2) - 1) < 1e-15
    dE = [skew(t) @ skew(np.eye(3)[a]) @ R for a in range(3)] + [skew(b1) @ R, skew(b2) @ R]
    px = _px(p)
    r, J = signed_sampson_px(skew(t) @ R, px, dE)
    h = 1e-6
    for j in range(5):
        d = np.zeros(5); d[j] = h
        Rp, tp = step_ref(R, t, d); Rm, tm = step_ref(R, t, -d)
        num = (signed_sampson_px(skew(tp) @ Rp, px) - signed_sampson_px(skew(tm) @ Rm, px)) / (2 * h)
        assert np.abs(num - J[:, j]).max() <= 1e-6 * max(1.0, np.abs(J[:, j]).max()), j
    assert np.abs(r * r - T.sampson2_px(E0, p["obs1"], p["obs2"], 0.5 * (p["cam"][0] + p["cam"][1]), p["cam"][2], p["cam"][3])).max() < 1e-9
    # the weight is the loss's derivative by r^2 up to the common factor: w(r) / w(0) = rho'(r^2) / rho'(0)
    r2 = np.linspace(0.05, 0.99, 12); e = 1e-6
    dr = (T.magsac_loss(r2 + e, 1.0) - T.magsac_loss(r2 - e, 1.0)) / (2 * e)
    w = magsac_weight(r2, 1.0)
    assert np.abs(dr / dr[0] - w / w[0]).max() < 1e-6 and magsac_weight(np.array([0.0]), 1.0)[0] == 1.0
    assert magsac_weight(np.array([1.5, np.inf]), 1.0).max() == 0.0


def test_the_refit_lowers_the_loss_and_keeps_an_essential_matrix():
    for label, args, iters, seed in PAIRS:
        ref = two_view_lo_ref(label, args, iters, seed)
        if ref["winner"] is None:
            print(label, "no winner")
            continue
        p, hyp = ref["pair"], ref["hyp"]
        four = refit_ref(p, ref["E0"], 4)
        sv = np.linalg.svd(ref["E"])[1]
        print(f"{label}: loss {ref['loss0']:.6g} -> {four['loss']:.6g} (4 steps) -> {ref['loss']:.6g} ({LO_ITERS} steps), kept {ref['kept']}, steps {ref['steps']}, "
              f"singular values - (1, 1, 0): {np.abs(sv - [1, 1, 0]).max():.3g}, n_inliers {ref['ref0']['n_inliers']} -> {ref['n_inliers']}")
        assert ref["loss"] <= four["loss"] <= ref["loss0"], label
        assert np.array_equal(four["trace"], ref["trace"][:len(four["trace"])]), label         # (the trace does not depend on lo_iters)
        assert abs(ref["loss0"] - hyp[ref["ref0"]["winner"][0]]["loss"][ref["ref0"]["winner"][1]]) <= 1e-9 * max(ref["loss0"], 1.0), label
        assert (ref["E"] * ref["E0"]).sum() >= 0, label
        if ref["kept"]:
            assert np.abs(sv - [1, 1, 0]).max() <= 1e-12, (label, sv)
        else:
            assert ref["E"] is ref["E0"]
        assert ref["kept"] <= ref["steps"] <= LO_ITERS


def test_the_refit_brings_general_scenes_closer_to_the_truth():
    n = 0
    for label, args, iters, seed in T.SCENES:
        ref = two_view_lo_ref(label, args, iters, seed)
        (r0, t0), (r1, t1) = T.err_to_truth(ref["ref0"], ref["pair"]), T.err_to_truth(ref, ref["pair"])
        print(f"{label}: error to truth (rotation, translation direction) in degrees: winner ({r0:.4g}, {t0:.4g}), after {LO_ITERS} steps ({r1:.4g}, {t1:.4g})")
        if args["scene"] == "general":
            assert r1 < r0 and t1 < t0, label
            n += 1
    assert n == 4


ROTATION = [(f"rotation {k}", dict(n_matches=400, inlier_frac=0.8, noise_px=0.5, seed=8300 + k, scene="rotation"), 64, 5 + k) for k in range(6)]


def test_rotation_scenes_still_never_initialise_after_the_refit():
    """(the pairs of test_gpu_two_view.test_rotation_scenes_never_initialise)  Without a baseline every t fits: the refit
    moves E along that valley, and what it arrives at must still fail CheckRT's counts or its parallax."""
    for label, args, iters, seed in ROTATION:
        ref = two_view_lo_ref(label, args, iters, seed)
        print(f"{label}: outcome {ref['ref0']['outcome']} -> {ref['outcome']}, parallax {ref['ref0']['parallax']:.4g} -> {ref['parallax']:.4g}, "
              f"n_pass {ref['ref0']['n_pass']} -> {ref['n_pass']}, loss {ref['loss0']:.6g} -> {ref['loss']:.6g}, kept {ref['kept']}")
        assert ref["outcome"] in (T.TV_FEW_GOOD, T.TV_LOW_PARALLAX, T.TV_NO_MODEL), label


# ---- the tolerances --------------------------------------------------------------------------------------------------
_lo_measured = {}


def lo_measured():
    if _lo_measured:
        return _lo_measured
    m = dict(e=0.0, loss=0.0, pose=0.0, pos=0.0, par=0.0, n_tie=0, n=0, ties=[])
    for label, args, iters, seed in PAIRS:
        a, b = two_view_lo_ref(label, args, iters, seed, LO_ITERS, "A"), two_view_lo_ref(label, args, iters, seed, LO_ITERS, "B")
        tie = T.is_tie(a["hyp"], a["ref0"])
        m["n_tie"] += tie
        if tie:
            m["ties"].append(label)
        if tie or a["winner"] is None or b["winner"] is None:
            continue
        m["n"] += 1
        row = dict(e=T.match_candidates(a["E"][None], b["E"][None])[0],
                   loss=max(abs(a["loss0"] - b["loss0"]) / max(a["loss0"], 1.0), abs(a["loss"] - b["loss"]) / max(a["loss"], 1.0)), pose=0.0, pos=0.0, par=0.0)
        if "pose" in a and "pose" in b:
            assert a["outcome"] == b["outcome"], label
            dq = min(np.abs(a["pose"][:4] - b["pose"][:4]).max(), np.abs(a["pose"][:4] + b["pose"][:4]).max())
            row["pose"] = max(dq, np.abs(a["pose"][4:] - b["pose"][4:]).max())
            row["par"] = abs(a["parallax"] - b["parallax"]) / max(1.0, abs(a["parallax"]))
            both = (a["code"] <= 2) & (b["code"] <= 2)
            if both.any():
                row["pos"] = float((np.linalg.norm(a["points"][both] - b["points"][both], axis=1) / np.linalg.norm(a["points"][both], axis=1)).max())
        print(f"{label}: A against B: E {row['e']:.3g}, loss {row['loss']:.3g}, pose {row['pose']:.3g}, points {row['pos']:.3g}, parallax {row['par']:.3g}, "
              f"kept {a['kept']} / {b['kept']}")
        for k in row:
            m[k] = max(m[k], float(row[k]))
    _lo_measured.update(m)
    return m


def test_lo_tolerances_are_the_measured_ones():
    m = lo_measured()
    print(f"measured over {m['n']} pairs ({m['n_tie']} tie pairs set aside): E spread {m['e']:.3g} (constant {E_LO_SPREAD_MEASURED:.3g}), "
          f"loss {m['loss']:.3g} ({LOSS_LO_SPREAD_MEASURED:.3g}), pose {m['pose']:.3g} ({POSE_LO_SPREAD_MEASURED:.3g}), "
          f"points {m['pos']:.3g} ({POS_LO_SPREAD_MEASURED:.3g}), parallax {m['par']:.3g} ({PARALLAX_LO_SPREAD_MEASURED:.3g})")
    assert m["e"] <= E_LO_SPREAD_MEASURED and m["loss"] <= LOSS_LO_SPREAD_MEASURED and m["pose"] <= POSE_LO_SPREAD_MEASURED
    assert m["pos"] <= POS_LO_SPREAD_MEASURED and m["par"] <= PARALLAX_LO_SPREAD_MEASURED
    # ... and the constants are the measurement, not a generous bound (another LAPACK build moves it: a factor 30)
    assert m["e"] >= E_LO_SPREAD_MEASURED / 30 and m["loss"] >= LOSS_LO_SPREAD_MEASURED / 30 and m["pose"] >= POSE_LO_SPREAD_MEASURED / 30
    assert m["pos"] >= POS_LO_SPREAD_MEASURED / 30 and m["par"] >= PARALLAX_LO_SPREAD_MEASURED / 30
    # tie pairs: the committed scenes stay under the cap; of the small pairs those of 5 and 6 matches tie by construction (every
    # candidate of a sample fits its own five matches exactly, so with at most one match more all losses are equal up to
    # rounding) and are held to the invariants only
    assert sum(t in [s[0] for s in T.SCENES] for t in m["ties"]) <= T.TIE_CAP * len(T.SCENES)
    assert set(m["ties"]) - {s[0] for s in T.SCENES} <= {"small 5", "small 6"}, m["ties"]


# ---- the library's arithmetic, serially on the CPU ---------------------------------------------------------------------
LO_DIR = os.path.join(ROOT, "tests", "two_view_lo")
HOST_FLAGS = ["-std=c++17", "-g", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "tests", "hipstub"), "-I" + os.path.join(ROOT, "include"),
              "-I" + os.path.join(ROOT, "mov-slam_amd", "csrc"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
SANITIZE = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0 abort_on_error=0 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def lo_main(tmp_path_factory):
    """tests/two_view_lo/lo_main.cpp built with the host compiler: (optimised, under the sanitizers)"""
    out = tmp_path_factory.mktemp("lo_main")
    cxx = os.environ.get("CXX", "g++")
    exes = []
    for name, flags in (("lo_main", ["-O2"]), ("lo_main_asan", SANITIZE)):
        exe = str(out / name)
        subprocess.check_call([cxx] + HOST_FLAGS + flags + [os.path.join(LO_DIR, "lo_main.cpp"), "-o", exe])
        exes.append(exe)
    return exes


def run_lo_main(exe, p, E0, lo_iters, path, threshold=1.0):
    n = len(p["obs1"])
    with open(path, "wb") as fh:
        np.array([n, lo_iters], np.int32).tofile(fh)
        np.array(list(p["cam"]) + [threshold], np.float64).tofile(fh)
        np.ascontiguousarray(E0, np.float64).tofile(fh)
        np.ascontiguousarray(p["obs1"], np.float64).tofile(fh); np.ascontiguousarray(p["obs2"], np.float64).tofile(fh)
    r = subprocess.run([exe, path], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[:4000]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    return dict(E=np.array(rows["E"], float).reshape(3, 3), trace=np.array(rows["L"], float), kept=int(rows["kept"][0]), steps=int(rows["steps"][0]),
                inliers0=int(rows["inliers0"][0]))


def test_the_librarys_refit_against_the_restatement_on_the_cpu(lo_main, tmp_path):
    """two_view_math.h's tv_lo_* from the restatement's own winner: the kept E, every L_k of the trace, kept and steps; the
    sanitizer build must print the same text as the optimised one and report nothing"""
    fin = str(tmp_path / "pair.bin")
    for label, args, iters, seed in PAIRS:
        ref = two_view_lo_ref(label, args, iters, seed)
        if ref["winner"] is None:
            continue
        for lo_iters in (LO_ITERS, 0):
            want = ref if lo_iters else refit_ref(ref["pair"], ref["E0"], 0)
            got = run_lo_main(lo_main[0], ref["pair"], ref["E0"], lo_iters, fin)
            de = T.match_candidates(want["E"][None], got["E"][None])[0]
            m = min(len(got["trace"]), len(want["trace"]))
            dl = float((np.abs(got["trace"][:m] - want["trace"][:m]) / np.maximum(want["trace"][:m], 1.0)).max())
            print(f"{label}, {lo_iters} steps: E distance {de:.3g} (E_LO_TOL {E_LO_TOL:.3g}), worst L_k difference {dl:.3g} (LOSS_LO_TOL {LOSS_LO_TOL:.3g}), "
                  f"kept {got['kept']} / {want['kept']}, steps {got['steps']} / {want['steps']}")
            assert de <= E_LO_TOL and dl <= LOSS_LO_TOL, label
            assert got["steps"] == want["steps"] and len(got["trace"]) == len(want["trace"]), label
            assert got["inliers0"] == ref["ref0"]["n_inliers"] or T.edge_matches(ref["ref0"]).any(), label
            if runner_up_gap(want["trace"], want["kept"]) > LOSS_LO_TOL:
                assert got["kept"] == want["kept"], label
            if lo_iters == 0:
                assert np.array_equal(got["E"], ref["E0"]) and got["kept"] == 0 and got["steps"] == 0
    # under the sanitizers: two scenes and every small pair, the largest step count, and a start that is no essential matrix
    for label, args, iters, seed in T.SCENES[::6] + SMALL:
        ref = two_view_lo_ref(label, args, iters, seed)
        if ref["winner"] is None:
            continue
        a = run_lo_main(lo_main[0], ref["pair"], ref["E0"], MAX_LO_ITERS, fin)
        b = run_lo_main(lo_main[1], ref["pair"], ref["E0"], MAX_LO_ITERS, fin)
        assert a["kept"] == b["kept"] and a["steps"] == b["steps"] and np.allclose(a["trace"], b["trace"], rtol=1e-9, atol=1e-12), label
        assert a["trace"][a["kept"]] <= a["trace"][0]
    p = two_view_lo_ref(*PAIRS[0])["pair"]
    for E0 in (np.zeros((3, 3)), np.full((3, 3), np.nan), np.eye(3)):
        g = run_lo_main(lo_main[1], p, E0, LO_ITERS, fin)
        print("start", E0[0], "-> kept", g["kept"], "steps", g["steps"], "trace", g["trace"][:3])
        assert g["kept"] <= g["steps"] <= LO_ITERS and np.isfinite(g["trace"]).all()


# ---- C-ABI without a device ------------------------------------------------------------------------------------------
def test_lo_symbols_constants_and_layout(built_lib):
    from movba import capi
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    assert int(re.search(r"#define\s+MOVBA_MAX_TWO_VIEW_LO_ITERS\s+(\d+)", hdr).group(1)) == 32 == capi.MAX_TWO_VIEW_LO_ITERS == MAX_LO_ITERS
    assert C.sizeof(capi.TwoViewLoInfo) == 104 and "movba_two_view_lo" in capi.EXPORTS
    assert capi.TwoViewLoInfo.E0.offset == 16 and capi.TwoViewLoInfo.kept.offset == 88 and capi.TwoViewLoInfo.n_inliers0.offset == 96
    assert C.sizeof(capi.TwoViewDesc) == 104 and C.sizeof(capi.TwoViewResult) == 216
    for hooks in (False, True):
        L = capi.lib(hooks)
        assert hasattr(L, "movba_two_view_lo")
        d, r, info = capi.TwoViewDesc(), capi.TwoViewResult(), capi.TwoViewLoInfo()
        r.status = 77; info.kept = 55
        for lo in (0, 10, -1, 33):
            assert L.movba_two_view_lo(None, C.byref(d), C.byref(r), 1, lo, C.byref(info)) == capi.ERR_ARG and r.status == 77 and info.kept == 55


def test_two_view_lo_host_side_over_the_fake_device_under_the_sanitizers():
    """The new entry point's host side (the shared front, the slot's sizing, upload and read-out) over the fake device of
    tests/hipstub, which does not run the refit: lo_iters 0 and 10 give movba_two_view's results bit for bit with kept = steps
    = 0, with and without `info`, in batches with empty pairs and pinned arrays; lo_iters -1 and 33 are refused with canaries
    untouched; n = 0."""
    subprocess.check_call(["make", "-C", LO_DIR, "-s", "lo_host_asan"])
    r = subprocess.run([os.path.join(LO_DIR, "lo_host_asan")], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[:4000]
    assert r.returncode == 0 and r.stdout.strip().endswith("TWO_VIEW_LO OK"), r.stderr[-2000:]
