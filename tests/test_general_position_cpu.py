"""General-position inputs without a GPU: the facts tests/test_gpu_general_position.py rests on, asserted on the oracle and on
the numpy restatements alone.

Every generator of movba.synth builds its cameras as small rotations about the identity: quaternions with x ~ z ~ 0 and w ~ 1,
rotation matrices with positive trace, LM steps of a few degrees.  synth.regauge() poses the SAME problem in another world
frame (X' = Rg X + tg, Tcw' = Tcw o G^-1, observations untouched).  Four frames are used throughout, one per branch of a
rotation-matrix -> quaternion conversion: 100 degrees about (1, 2, 3) keeps every keyframe's trace positive (~0.6); 175 degrees
about (almost) x, y and z puts every trace at ~ -0.99 with the largest diagonal entry on x, y and z respectively.

Asserted here: the oracle is frame-independent far inside the GPU test's tolerances; the frames reach the branches they are
meant to; the large-step window's first accepted LM step exceeds 0.5 rad (where se3_oplus leaves its power series) and its
solve converges; the triangulation restatement is invariant under the four rotations (a translation of the world is NOT an
invariance of the DLT: the constraint |x| = 1 on homogeneous 4-vectors is not translation-invariant, in the reference too);
the two-view scenes with camera 2 rolled about its optical axis stay inside the caps and the measured spreads of
tests/test_two_view_cpu.py; and the generators' default outputs are bit for bit those of the commit before this file."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, oracle_order_noise, quat_angle

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

import test_triangulate_cpu as TRI  # noqa: E402
import test_two_view_cpu as TV  # noqa: E402

# (label, axis, angle in degrees, index of the diagonal entry that is largest after the change of frame - None: positive trace)
FRAMES = [("100deg-about-123", (1.0, 2.0, 3.0), 100.0, None), ("175deg-about-x", (1.0, 0.1, 0.05), 175.0, 0),
          ("175deg-about-y", (0.1, 1.0, 0.05), 175.0, 1), ("175deg-about-z", (0.05, 0.1, 1.0), 175.0, 2)]
FRAME_IDS = [f[0] for f in FRAMES]
TG = np.array([3.0, -2.0, 5.0])

# oracle against itself across frames: two orders above what was measured (2e-14 rad, 7e-13 m, 1.5e-11 m)
INV_ROT, INV_TRANS, INV_POINT = 1e-11, 1e-10, 1e-9


def frame_R(k):
    return synth.gauge_rotation(FRAMES[k][1], FRAMES[k][2])


def back(poses, points, k, tg=TG):
    """a result in frame k mapped back to the generator's frame (G^-1 = (Rg^T, -Rg^T tg))"""
    Rg = frame_R(k)
    return synth.regauge_poses(poses, Rg.T, -Rg.T @ tg), synth.regauge_points(points, Rg.T, -Rg.T @ tg)


_windows = {}


def window(name):
    """the windows of this file and of the GPU file, built once (callers must not modify them)"""
    if name not in _windows:
        if name == "small":
            w = synth.cfg("small")
        elif name == "stereo":
            w = synth.make_window(12, 3, 1500, seed=57, run_lo=2, run_hi=7, stereo_frac=0.5)
        elif name == "cameras":
            w = synth.mixed_cameras(synth.make_window(12, 3, 1500, seed=59, run_lo=2, run_hi=7), seed=60)
        elif name == "hard":
            w, _ = load_golden("lba_hard")
        elif name == "large-steps":
            w = synth.make_window(8, 2, 300, seed=901, run_lo=3, run_hi=8, rot_sigma_deg=20.0, trans_sigma=0.3)
        else:
            raise KeyError(name)
        _windows[name] = w
    return _windows[name]


_gauged = {}


def gauged(name, k, renormalise=True):
    key = (name, k, renormalise)
    if key not in _gauged:
        _gauged[key] = synth.regauge(window(name), frame_R(k), TG, flip_every=2, renormalise=renormalise)
    return _gauged[key]


_oracle = {}


def oracle_solve(oracle_mod, name, k=None, max_iters=None, renormalise=True):
    """the oracle's solve of window `name` (k: in frame k), computed once and shared; callers must not modify it"""
    key = (name, k, max_iters, renormalise)
    if key not in _oracle:
        w = window(name) if k is None else gauged(name, k, renormalise)
        _oracle[key] = oracle_mod.solve(w, max_iters=max_iters)
    return _oracle[key]


_noise = {}


def large_step_order_noise(oracle_mod):
    """conftest.oracle_order_noise of the large-step window: (rot, trans, point)"""
    if "v" not in _noise:
        _noise["v"] = oracle_order_noise(oracle_mod, window("large-steps"))
    return _noise["v"]


def tri_scene(i):
    """test_triangulate_cpu.SCENES[i] shrunk to 6 pairs x 300 matches"""
    return synth.make_triangulation(**dict(TRI.SCENES[i][1], n_pairs=6, n_per_pair=300))


ROLLS = (180.0, 90.0, -120.0)
# (scene, roll) -> seed where 8500 exceeds a measured spread of test_two_view_cpu (the next seed in 8500 - 8520 that stays inside
# all five).  What the two variants of the restatement differ by at 8500:
#   general, 90 degrees:   E 2.0e-4, candidate loss 7.2e-5 (constants 5.1e-5, 3.6e-6)                     -> 8501
#   general, -120 degrees: candidate loss 6.6e-6                                                          -> 8502 (8501: pose 2.0e-7)
#   planar, -120 degrees:  pose 3.1e-8, points 1.3e-6, parallax 4.6e-8 (constants 4e-10, 1.8e-9, 6e-10)   -> 8506 (8501: loss 9.0e-5; 8504 stays inside but does not initialise)
#   forward, 90 degrees:   E 9.5e-5, candidate loss 1.1e-4                                                -> 8503 (8501, 8502: loss 4.7e-4, 8.2e-6)
ROLL_SEED = {("general", 90.0): 8501, ("general", -120.0): 8502, ("planar", -120.0): 8506, ("forward", 90.0): 8503}
ROLL_SCENES = [(f"{sc} roll {roll:g}", dict(n_matches=500, inlier_frac=0.7, noise_px=0.5, seed=ROLL_SEED.get((sc, roll), 8500), scene=sc,
                                            roll_deg=roll), 64, 31) for sc in ("general", "planar", "forward") for roll in ROLLS]


# ---- the generators are untouched ---------------------------------------------------------------------------------------
def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def test_default_generator_outputs_are_those_of_the_parent_commit():
    """sha256 over dtype, shape and bytes of every array, computed on the commit before regauge() and roll_deg existed"""
    w = synth.cfg("small")
    assert _digest([w.poses, w.pose_fixed, w.points, w.edge_pose, w.edge_point, w.obs, w.inv_sigma2, w.truth_poses, w.truth_points]) == \
        "bde68ec594514ef69ea0c4e2c923f69ede036d2b59e2b353abbcaa52eb19031c"
    f = synth.make_frame()
    assert _digest([f["Xw"], f["obs"], f["pose0"], f["truth"], f["is_outlier"]]) == \
        "ca41feb5e78e5fbd4d18a913a034e328acf2de4a81c96cb1b435c836cf52da5d"
    p = synth.make_two_view(500, seed=8100)
    assert _digest([p["obs1"], p["obs2"], p["R"], p["t"], p["X"], p["is_inlier"]]) == \
        "335a7678ed59af3eba63db1c873cdb9ffc436202a64df42ab42ca2d38811fffa"
    p0 = synth.make_two_view(500, seed=8100, roll_deg=0.0)
    assert all(np.array_equal(p[k], p0[k]) for k in ("obs1", "obs2", "R", "t", "X", "is_inlier"))


# ---- the change of frame itself -----------------------------------------------------------------------------------------
def test_regauge_keeps_every_residual_and_maps_back():
    w = window("stereo")
    for k in range(4):
        for renorm in (True, False):
            g = gauged("stereo", k, renorm)
            n = np.linalg.norm(g.poses[:, :4], axis=1)
            assert (g.poses[1::2, 3] < 0).all() and (g.poses[0::2, 3] >= 0).all()           # every second quaternion negated
            if renorm:
                assert np.abs(n - 1).max() < 4e-16
            else:
                assert 1e-9 < np.abs(n - 1).max() < 1.2e-7                                    # off unit like a widened float quaternion
            for ww in (w, g):
                R = np.stack([synth.R_from_quat(q / np.linalg.norm(q)) for q in ww.poses[:, :4]])
                Y = np.einsum('eij,ej->ei', R[ww.edge_pose], ww.points[ww.edge_point]) + ww.poses[ww.edge_pose, 4:]
                if ww is w:
                    Y0 = Y
            assert np.abs(Y - Y0).max() < 1e-13                                                # the same points in every camera
            pb, xb = back(g.poses, g.points, k)
            assert quat_angle(pb[:, :4], w.poses[:, :4]).max() < 1e-15 and np.abs(pb[:, 4:] - w.poses[:, 4:]).max() < 1e-14
            assert np.abs(xb - w.points).max() < 1e-13
            assert g.obs is w.obs and g.obs_right is w.obs_right and g.bf == w.bf


@pytest.mark.parametrize("k", range(4), ids=FRAME_IDS)
def test_frames_reach_the_branches_they_are_meant_to(k):
    """100 degrees: every trace positive (the first branch, but with all nine entries of R in play); 175 degrees: every trace
    below -0.9 and the largest diagonal entry the intended one, in the windows, the frame and the triangulation views"""
    want = FRAMES[k][3]
    quats = [gauged(n, k).poses[:, :4] for n in ("small", "stereo", "cameras", "hard")]
    quats.append(synth.regauge_frame(synth.make_frame(n=500, seed=1001), frame_R(k), TG)["pose0"][None, :4])
    quats.append(synth.regauge_triangulation(tri_scene(0), frame_R(k))["views"]["poses"][:, :4])
    for q in np.concatenate(quats):
        R = synth.R_from_quat(q)
        if want is None:
            assert 0.3 < np.trace(R) < 0.9
            assert np.abs(q).min() > 0.05                   # no component of the quaternion is small
        else:
            assert np.trace(R) < -0.9 and int(np.argmax(np.diag(R))) == want
            assert np.diag(R)[want] - np.sort(np.diag(R))[1] > 1.5       # ... by a margin no rounding or tie order can turn


# ---- the oracle does not care about the frame ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "stereo"])
@pytest.mark.parametrize("k", range(4), ids=FRAME_IDS)
def test_oracle_is_frame_independent(oracle_mod, name, k):
    w = window(name)
    o, og = oracle_solve(oracle_mod, name), oracle_solve(oracle_mod, name, k)
    assert o["status"] == og["status"] == 0
    assert np.array_equal(o["trace"]["accept"], og["trace"]["accept"]) and o["n_solves"] == og["n_solves"]
    assert np.array_equal(o["outlier"], og["outlier"])
    pb, xb = back(og["poses"], og["points"], k)
    rot = float(quat_angle(pb[:, :4], o["poses"][:, :4]).max())
    trans = float(np.abs(pb[:, 4:] - o["poses"][:, 4:]).max())
    point = float(np.abs(xb - o["points"]).max())
    chi2 = float(np.abs(og["chi2"] - o["chi2"]).max())
    print(f"{name} in frame {FRAME_IDS[k]}: oracle against itself: rotation {rot:.3g} rad, translation {trans:.3g} m, "
          f"points {point:.3g} m, chi2 {chi2:.3g}")
    assert rot < INV_ROT and trans < INV_TRANS and point < INV_POINT
    # the oracle normalises what it is given: unit quaternions with w >= 0 come back, fixed keyframes included
    assert (og["poses"][:, 3] >= 0).all() and np.abs(np.linalg.norm(og["poses"][:, :4], axis=1) - 1).max() < 1e-15
    fx = w.pose_fixed == 1
    gw = gauged(name, k)
    assert quat_angle(og["poses"][fx, :4], gw.poses[fx, :4]).max() < 1e-15 and np.array_equal(og["poses"][fx, 4:], gw.poses[fx, 4:])


@pytest.mark.parametrize("name", ["small", "stereo"])
def test_oracle_takes_a_quaternion_that_is_not_unit(oracle_mod, name):
    """renormalise=False: quaternions off unit by ~3e-8, same direction: the same solve"""
    o, og = oracle_solve(oracle_mod, name, 0), oracle_solve(oracle_mod, name, 0, renormalise=False)
    assert np.array_equal(o["trace"]["accept"], og["trace"]["accept"]) and np.array_equal(o["outlier"], og["outlier"])
    rot = float(quat_angle(og["poses"][:, :4], o["poses"][:, :4]).max())
    trans = float(np.abs(og["poses"][:, 4:] - o["poses"][:, 4:]).max())
    point = float(np.abs(og["points"] - o["points"]).max())
    print(f"{name}: off-unit input against unit input: rotation {rot:.3g} rad, translation {trans:.3g} m, points {point:.3g} m")
    assert rot < INV_ROT and trans < INV_TRANS and point < INV_POINT


# ---- LM steps above 0.5 rad ----------------------------------------------------------------------------------------------
def test_large_step_window_leaves_the_power_series_and_converges(oracle_mod):
    """se3_oplus takes its power series for |omega|^2 < 0.25 and the closed form (sincos, reciprocal) from there on.  The
    first accepted step of at least two keyframes must be a rotation by more than 0.5 rad: measured on the oracle with
    max_iters = 1, start estimate against result.  (The geodesic angle of exp(omega) T against T is |omega| exactly.)"""
    w = window("large-steps")
    err0 = np.rad2deg(quat_angle(w.poses[:, :4], w.truth_poses[:, :4]))
    o1 = oracle_solve(oracle_mod, "large-steps", max_iters=1)
    assert o1["trace"]["accept"][0] == 1
    step = quat_angle(o1["poses"][:, :4], w.poses[:, :4])
    o = oracle_solve(oracle_mod, "large-steps")
    err1 = np.rad2deg(quat_angle(o["poses"][:, :4], w.truth_poses[:, :4]))
    print(f"large-step window: start errors up to {err0.max():.1f} deg; first steps {np.round(np.rad2deg(np.sort(step)[::-1][:4]), 1)} deg "
          f"({int((step > 0.5).sum())} above 0.5 rad = 28.65 deg); accepts {o['trace']['accept']}; ends {err1.max():.3f} deg from truth")
    assert (step > 0.5).sum() >= 2
    assert step.max() < 2.0                 # ... and nowhere near the 120 degrees that would leave R_to_quat's first branch
    assert err1.max() < 0.5
    # the same in the 100-degree frame (the step is a left increment in the camera frame: it does not see the world frame)
    g1 = oracle_solve(oracle_mod, "large-steps", 0, max_iters=1)
    stepg = quat_angle(g1["poses"][:, :4], gauged("large-steps", 0).poses[:, :4])
    assert np.abs(stepg - step).max() < 1e-9 and np.array_equal(g1["trace"]["accept"], o1["trace"]["accept"])


def test_large_step_window_order_noise(oracle_mod):
    """How far the oracle's own result moves with the order of a point's edges: what the GPU test's tolerances rest on"""
    rot, trans, point = large_step_order_noise(oracle_mod)
    print(f"large-step window: oracle order noise: rotation {rot:.3g} rad, translation {trans:.3g} m, points {point:.3g} m")
    # the window is well conditioned: its order noise is far inside test_gpu_parity's default tolerances (1e-8, 1e-8, 1e-6)
    assert rot < 1e-10 and trans < 1e-10 and point < 1e-8


# ---- pose optimisation ---------------------------------------------------------------------------------------------------
def test_oracle_pose_optimisation_is_frame_independent(oracle_mod):
    f = synth.make_frame(n=500, seed=1001, outlier_frac=0.55)
    o = oracle_mod.pose_opt(f["Xw"], f["obs"], f["pose0"], f["cam"], 5.0, 25.0)
    for k in range(4):
        g = synth.regauge_frame(f, frame_R(k), TG, flip=(k % 2 == 1))
        og = oracle_mod.pose_opt(g["Xw"], g["obs"], g["pose0"], g["cam"], 5.0, 25.0)
        pb, _ = back(og["pose"][None], np.zeros((1, 3)), k)
        rot = float(quat_angle(pb[:, :4], o["pose"][None, :4]).max()); trans = float(np.abs(pb[0, 4:] - o["pose"][4:]).max())
        print(f"pose optimisation in frame {FRAME_IDS[k]}: {og['n_inliers']} inliers ({o['n_inliers']}), rotation {rot:.3g} rad, translation {trans:.3g} m")
        assert og["n_inliers"] == o["n_inliers"] and np.array_equal(og["outlier"], o["outlier"])
        assert rot < INV_ROT and trans < INV_TRANS


# ---- triangulation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3), ids=["mono", "stereo", "mixed"])
def test_triangulation_restatement_is_invariant_under_the_four_rotations(i):
    """codes equal except on matches on a gate (edge_alternatives at POS_TOL: a narrower band than the two-view file's EDGE_REL),
    positions Rg times the un-rotated ones within POS_TOL"""
    sc = tri_scene(i)
    ref = TRI.triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
    edge, _ = TRI.edge_alternatives(sc["views"], sc["pairs"], sc["matches"], ref, sc["reproj_gate"], sc["far_threshold"])
    assert edge.sum() <= max(TRI.EDGE_CAP * ref["q"]["M"], 1)
    for k in range(4):
        Rg = frame_R(k)
        sg = synth.regauge_triangulation(sc, Rg, flip_every=2)
        rg = TRI.triangulate_ref(sg["views"], sg["pairs"], sg["matches"], sg["reproj_gate"], sg["far_threshold"])
        same = rg["code"] == ref["code"]
        assert (same | edge).all(), np.flatnonzero(~same & ~edge)[:10]
        acc = same & np.isin(ref["code"], TRI.ACCEPTED)
        Xb = synth.regauge_points(rg["points"], Rg.T)
        rel = np.linalg.norm(Xb[acc] - ref["points"][acc], axis=1) / np.linalg.norm(ref["points"][acc], axis=1)
        print(f"{TRI.SCENES[i][0]} shrunk, frame {FRAME_IDS[k]}: {int((~same).sum())} codes differ ({int(edge.sum())} matches on a gate), "
              f"{int(acc.sum())} accepted, worst relative position difference {rel.max():.3g} (POS_TOL {TRI.POS_TOL:.3g})")
        assert rel.max() <= TRI.POS_TOL


def test_a_translation_of_the_world_is_no_invariance_of_the_dlt():
    """why the triangulation tests use tg = 0: with tg = (3, -2, 5) positions of accepted DLT points move by more than POS_TOL"""
    sc = tri_scene(0)
    ref = TRI.triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
    sg = synth.regauge_triangulation(sc, np.eye(3), TG)
    rg = TRI.triangulate_ref(sg["views"], sg["pairs"], sg["matches"], sg["reproj_gate"], sg["far_threshold"])
    acc = (rg["code"] == ref["code"]) & (ref["code"] == TRI.DLT)
    rel = np.linalg.norm(rg["points"][acc] - TG - ref["points"][acc], axis=1) / np.linalg.norm(ref["points"][acc], axis=1)
    print(f"translated world: accepted DLT positions move by up to {rel.max():.3g} (relative), median {np.median(rel):.3g}")
    assert rel.max() > 1e3 * TRI.POS_TOL


# ---- two-view with camera 2 rolled about its optical axis -------------------------------------------------------------------
_roll = {}


def roll_measured():
    if not _roll:
        _roll.update(TV._measure(ROLL_SCENES))
    return _roll


def test_roll_scenes_stay_inside_the_caps_and_the_measured_spreads():
    """(`general` rolled by 180 degrees does not initialise - outcome TV_FEW_GOOD, 73 of 201 inliers pass, on the restatement
    and on the library alike: the hypothesis stage sees ONE focal length for a camera with fx != fy, and the roll turns that
    error against itself.  The pair is compared up to its outcome, hypotheses and counts; its pose path is not exercised.)"""
    m = roll_measured()
    for (label, n_c, n_ill, n_edge, M, tie, outcome), sp in zip(m["rows"], m["so_far"]):
        print(f"{label}: {n_c} candidates, {n_ill} ill-conditioned, {n_edge} of {M} matches on a gate, tie {tie}, outcome {outcome}; "
              f"spreads so far: pose {sp[0]:.3g}, points {sp[1]:.3g}, parallax {sp[2]:.3g}")
        assert n_ill <= TV.ILL_CAP * n_c and n_edge <= max(TV.EDGE_CAP * M, 1)
    assert m["n_tie"] <= TV.TIE_CAP * len(ROLL_SCENES)
    print(f"roll scenes: pose spread {m['pose']:.3g} ({TV.POSE_SPREAD_MEASURED:.3g}), points {m['pos']:.3g} ({TV.POS_SPREAD_MEASURED:.3g}), "
          f"parallax {m['par']:.3g} ({TV.PARALLAX_SPREAD_MEASURED:.3g}), E {m['e']:.3g} ({TV.E_SPREAD_MEASURED:.3g}), "
          f"loss {m['loss']:.3g} ({TV.LOSS_SPREAD_MEASURED:.3g})")
    assert m["pose"] <= TV.POSE_SPREAD_MEASURED and m["pos"] <= TV.POS_SPREAD_MEASURED and m["par"] <= TV.PARALLAX_SPREAD_MEASURED
    # (the candidates' own spreads too: compare_with_ref holds the device to ten times these)
    assert m["e"] <= TV.E_SPREAD_MEASURED and m["loss"] <= TV.LOSS_SPREAD_MEASURED


def test_reseeded_roll_scenes_exceed_a_measured_spread_at_seed_8500():
    """the table at ROLL_SEED, checked: each scene that was given another seed is outside at least one of the five measured
    spreads at 8500 (between the two variants of the restatement: no device arithmetic could be held to ten times them)"""
    for (sc, roll), seed in ROLL_SEED.items():
        m = TV._measure([(f"{sc} roll {roll:g} at 8500", dict(n_matches=500, inlier_frac=0.7, noise_px=0.5, seed=8500, scene=sc, roll_deg=roll), 64, 31)])
        over = [k for k, c in (("e", TV.E_SPREAD_MEASURED), ("loss", TV.LOSS_SPREAD_MEASURED), ("pose", TV.POSE_SPREAD_MEASURED),
                               ("pos", TV.POS_SPREAD_MEASURED), ("par", TV.PARALLAX_SPREAD_MEASURED)) if m[k] > c]
        print(f"{sc} roll {roll:g} at seed 8500 (replaced by {seed}): E {m['e']:.3g}, loss {m['loss']:.3g}, pose {m['pose']:.3g}, "
              f"points {m['pos']:.3g}, parallax {m['par']:.3g}; over its constant: {over}")
        assert over and 8500 < seed <= 8520


def test_forward_scene_rolled_by_180_degrees_has_a_rotation_of_trace_minus_one():
    """... and the restatement initialises from it: the pose it returns has w ~ 0 (its conversion goes by the largest diagonal
    entry, z).  The x and y branches would need camera 2 to look backwards: no match is then in front of both cameras."""
    label, args, iters, seed = ROLL_SCENES[6]
    assert args["scene"] == "forward" and args["roll_deg"] == 180.0
    p = synth.make_two_view(**args)
    assert np.trace(p["R"]) < -0.99 and int(np.argmax(np.diag(p["R"]))) == 2
    r = TV.two_view_ref(p, iters, seed)
    assert r["outcome"] == TV.TV_OK and np.trace(r["R"]) < -0.99 and abs(r["pose"][3]) < 0.05
    assert np.abs(TV.q2R(r["pose"][:4]) - r["R"]).max() < 1e-14
    rot, tr = TV.err_to_truth(r, p)
    print(f"{label}: trace {np.trace(r['R']):.4f}, error to truth {rot:.3g} deg / {tr:.3g} deg")
    assert rot < 0.5


def test_the_librarys_own_conversion_at_trace_minus_one_on_the_fake_device(tmp_path):
    """tests/hipstub runs the library's two_view_math.h on the CPU: tv_R2q's last branch (m[8] the largest diagonal entry) with
    `forward` rolled by 180 degrees, and a trace just below zero with `planar` rolled by -120 degrees"""
    for idx, lo, hi in ((6, -1.0, -0.99), (5, -0.2, 0.0)):
        label, args, iters, seed = ROLL_SCENES[idx]
        p = synth.make_two_view(**args)
        got = TV.solve_on_the_fake_device(p, iters, seed, tmp_path)
        assert got["status"] == 0 and got["outcome"] == TV.TV_OK
        TV.compare_with_ref(got, p, iters, seed, label, check_truth=True)
        R = TV.q2R(got["pose"][:4])
        assert lo < np.trace(R) < hi and int(np.argmax(np.diag(R))) == 2, (label, np.trace(R))


def test_the_yardsticks_conversion_is_accurate_at_w_zero():
    for ax in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 2.0, 3.0)):
        for deg in (3.0, 100.0, 120.0, 179.9999999, 180.0):
            R = synth.gauge_rotation(ax, deg)
            assert np.abs(TV.q2R(TV.R2q(R)) - R).max() < 4e-15
