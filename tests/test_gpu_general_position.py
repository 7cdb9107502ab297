"""The HIP path on inputs in general position and on LM steps above 0.5 rad.

Every synthetic window, frame and scene of the suite has its cameras within a few degrees of the identity; the windows, frames and
scenes here are the same problems posed in another world frame (movba.synth.regauge, tests/test_general_position_cpu.py: four
frames, one per branch of a rotation-matrix -> quaternion conversion, every second quaternion negated to w < 0), and one window
whose start errors reach 51 degrees.  What is checked, and what it reaches that no other test does:

  local BA, every reduced solver (k_pcg_rows, k_band, dense_persist, dense_solve) against the oracle IN the new frame and against
  its own un-gauged solve mapped forward: quat_to_R / quat_rotate / the quaternion product of se3_oplus with all four components
  large, Jacobians and Schur blocks where all nine entries of R matter, quat_normalize_exact on w < 0 and on quaternions that
  are off unit by ~3e-8;
  large steps: the closed-form branch of se3_oplus (th2 >= 0.25: sincos and fast_rcp) in the four solvers' update code, compared
  after one and two iterations as well, so that later iterations cannot average an error of the big step away;
  marginals: pose blocks are camera-frame quantities and must not see the frame, point blocks must turn with it;
  pose optimisation: the LM (pose_kernels.hip's se3_oplus) and the hypothesis stage, whose winner goes through R2q's three
  t <= 0 branches in the 175-degree frames (asserted: the returned ransac_pose has negative trace);
  triangulation under the four rotations (a translation is no invariance of the DLT: see the CPU file);
  two-view with camera 2 rolled about its optical axis: `forward` at 180 degrees comes back TV_OK with trace(R) ~ -1, through
  the branch of tv_R2q whose largest diagonal entry is m[8].

Left unreached on purpose: the t <= 0 branches of R_to_quat INSIDE se3_oplus (a single LM step above 120 degrees: no
converging solve takes one); the m[0]- and m[4]-largest branches of tv_R2q (camera 2 would look backwards: no match is in front
of both cameras, there is no valid result to compare); the closed-form branch of se3_oplus through movba_pose_opt (steps of the
pose-only LM stay below 17 degrees from every start that converges; the LBA kernels call the same inline function)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, quat_angle

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

import test_general_position_cpu as G  # noqa: E402
import test_triangulate_cpu as TRI  # noqa: E402
import test_two_view_cpu as TV  # noqa: E402
from test_gpu_marginals import TOL as MARG_TOL, _check as check_marginals  # noqa: E402
from test_gpu_parity import GUARD, POINT_TOL, ROT_TOL, TRANS_TOL, _far_off_pose, check_against  # noqa: E402
from test_gpu_pose_batch import KEYS as POSE_KEYS  # noqa: E402
from test_marginals_cpu import rel_block_err  # noqa: E402

pytestmark = pytest.mark.gpu

FRAME_IDS = G.FRAME_IDS
SOLVERS = {"banded": dict(), "pcg": dict(solver=3), "direct": dict(direct=True), "giveup": dict(pcg_max_iters=1, solver=3)}


@pytest.fixture(scope="module")
def solvers(built_lib):
    s = {k: built_lib.Solver(**kw) for k, kw in SOLVERS.items()}
    yield s
    for v in s.values():
        v.close()


def assert_solver_that_ran(r, which):
    """as test_gpu_parity tells the reduced solvers apart"""
    assert r["n_chol_fail"] == 0 and r["n_sync_timeouts"] == 0
    if which == "banded":
        assert r["n_band"] == r["n_solves"] and r["n_direct"] == 0 and r["n_pcg_giveups"] == 0 and (r["trace"]["pcg"] == -2).all()
    elif which == "pcg":
        assert r["n_band"] == 0 and r["n_direct"] == 0 and r["n_pcg_giveups"] == 0 and r["pcg_iters"] > 0
    elif which == "direct":
        assert r["n_direct"] == r["n_solves"] and r["direct_from"] == 0 and r["n_pcg_giveups"] == 0 and r["pcg_iters"] == 0
    else:
        assert r["n_pcg_giveups"] == 1 and r["direct_from"] == 0 and r["n_direct"] == r["n_solves"] and r["n_band"] == 0


def forward(r, k):
    """a result of the un-gauged window mapped into frame k"""
    return synth.regauge_poses(r["poses"], G.frame_R(k), G.TG), synth.regauge_points(r["points"], G.frame_R(k), G.TG)


def check_against_ungauged(rg, r0, w, k, label):
    """metamorphic: the solve in frame k against the un-gauged solve of the same solver mapped forward"""
    assert np.array_equal(rg["trace"]["accept"], r0["trace"]["accept"]) and rg["n_solves"] == r0["n_solves"], label
    mism = rg["outlier"] != r0["outlier"]
    assert (np.abs(r0["chi2"][mism] - w.chi2_gate) <= GUARD).all(), label
    pf, xf = forward(r0, k)
    rot = float(quat_angle(rg["poses"][:, :4], pf[:, :4]).max())
    trans = float(np.abs(rg["poses"][:, 4:] - pf[:, 4:]).max())
    point = float(np.abs(rg["points"] - xf).max())
    print(f"{label}: against the un-gauged solve mapped forward: rotation {rot:.3g} rad, translation {trans:.3g} m, points {point:.3g} m")
    assert rot < ROT_TOL and trans < TRANS_TOL and point < POINT_TOL, label


_ungauged = {}


def ungauged_solve(solver, name):
    """the un-gauged solve of window `name` and its marginals at both dampings, computed once.  For the session's default
    `solver` fixture ONLY, not the handles of `solvers`: results are cached by window name alone, and the marginals are taken
    right behind the solve, while the handle still holds it."""
    if name not in _ungauged:
        r = solver.solve(G.window(name))
        assert r["status"] == 0
        _ungauged[name] = (r, {d: solver.marginals(d) for d in (0.0, 1e-3)} if name in ("small", "stereo") else None)
    return _ungauged[name]


# ---- local BA in the four frames -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4), ids=FRAME_IDS)
@pytest.mark.parametrize("name", ["small", "stereo", "cameras", "hard"])
def test_lba_in_the_four_frames(solver, oracle_mod, name, k):
    """... and, for `small` and `stereo`, the marginals of the solved window: each block against the numpy reference in the new
    frame, pose blocks against the un-gauged handle's (they are expressed in the camera frame), point blocks against Rg S Rg^T"""
    w0, wg = G.window(name), G.gauged(name, k)
    assert (wg.poses[1::2, 3] < 0).all() and (wg.poses[wg.pose_fixed == 1, 3] < 0).any()      # w < 0 goes in, on a fixed keyframe too
    r0, m0 = ungauged_solve(solver, name)
    rg = solver.solve(wg)
    label = f"{name} in frame {FRAME_IDS[k]}"
    check_against(rg, G.oracle_solve(oracle_mod, name, k), wg)
    check_against_ungauged(rg, r0, w0, k, label)
    assert (rg["poses"][:, 3] >= 0).all() and np.abs(np.linalg.norm(rg["poses"][:, :4], axis=1) - 1).max() < 1e-14
    if m0 is None:
        return
    Rg = G.frame_R(k)
    for d in (0.0, 1e-3):
        mg = solver.marginals(d)
        check_marginals(wg, rg, mg, d, label)
        ep = rel_block_err(mg["pose_cov"], m0[d]["pose_cov"])
        epts = rel_block_err(mg["point_cov"], np.einsum('ij,pjk,lk->pil', Rg, m0[d]["point_cov"], Rg))
        print(f"{label}: damping {d:g}: pose blocks against the un-gauged handle's {ep:.2e}, point blocks against Rg S Rg^T {epts:.2e}")
        assert ep <= MARG_TOL and epts <= MARG_TOL, label
        assert np.array_equal(np.isnan(mg["pose_cov"]), np.isnan(m0[d]["pose_cov"]))
        assert np.array_equal(np.isnan(mg["point_cov"]), np.isnan(m0[d]["point_cov"]))


@pytest.mark.parametrize("name,k", [("small", 1), ("stereo", 2), ("cameras", 3), ("hard", 0)])
def test_lba_takes_quaternions_that_are_not_unit(solver, oracle_mod, name, k):
    """renormalise=False: every quaternion off unit by what rounding it to float32 does (~3e-8), every second one negated"""
    wg = G.gauged(name, k, renormalise=False)
    n = np.linalg.norm(wg.poses[:, :4], axis=1)
    assert np.abs(n - 1).max() > 1e-9
    rg = solver.solve(wg)
    check_against(rg, G.oracle_solve(oracle_mod, name, k, renormalise=False), wg)
    check_against_ungauged(rg, ungauged_solve(solver, name)[0], G.window(name), k, f"{name} in frame {FRAME_IDS[k]}, off-unit input")
    assert (rg["poses"][:, 3] >= 0).all() and np.abs(np.linalg.norm(rg["poses"][:, :4], axis=1) - 1).max() < 1e-14


@pytest.mark.parametrize("which", list(SOLVERS))
@pytest.mark.parametrize("k", [0, 2], ids=[FRAME_IDS[0], FRAME_IDS[2]])
def test_every_reduced_solver_in_general_position(solvers, oracle_mod, which, k):
    s = solvers[which]
    w0, wg = G.window("stereo"), G.gauged("stereo", k)
    r0, rg = s.solve(w0), s.solve(wg)
    assert_solver_that_ran(rg, which)
    assert_solver_that_ran(r0, which)
    check_against(rg, G.oracle_solve(oracle_mod, "stereo", k), wg)
    check_against_ungauged(rg, r0, w0, k, f"stereo on {which} in frame {FRAME_IDS[k]}")


# ---- LM steps above 0.5 rad ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(SOLVERS))
@pytest.mark.parametrize("k", [None, 0], ids=["ungauged", FRAME_IDS[0]])
def test_large_steps_on_every_reduced_solver(solvers, oracle_mod, which, k):
    """The window of test_general_position_cpu.test_large_step_window_leaves_the_power_series_and_converges: two keyframes turn by
    29 and 31 degrees in the first accepted step (asserted there on the oracle; here on the device's own first iteration), which
    is the closed-form branch of se3_oplus.  Held to test_gpu_parity's default tolerances (1e-8 rad, 1e-8 m, 1e-6 m) after one,
    two and all ten iterations.  The oracle's own order noise on this window is 1.3e-15 rad / 1.9e-14 m / 4.6e-11 m
    (test_large_step_window_order_noise prints it): ten times that is far below the default tolerances, so nothing wider is
    justified here, and nothing wider is used."""
    s = solvers[which]
    w = G.window("large-steps") if k is None else G.gauged("large-steps", k)
    for iters in (1, 2, None):
        r = s.solve(w, max_iters=iters)
        o = G.oracle_solve(oracle_mod, "large-steps", k, max_iters=iters)
        assert_solver_that_ran(r, which)
        rot = float(quat_angle(r["poses"][:, :4], o["poses"][:, :4]).max()); trans = float(np.abs(r["poses"][:, 4:] - o["poses"][:, 4:]).max())
        print(f"large steps on {which}, {'ungauged' if k is None else FRAME_IDS[k]}, max_iters {iters}: rotation {rot:.3g} rad, "
              f"translation {trans:.3g} m, points {np.abs(r['points'] - o['points']).max():.3g} m against the oracle")
        check_against(r, o, w)
        if iters == 1:
            q0 = w.poses[:, :4] / np.linalg.norm(w.poses[:, :4], axis=1, keepdims=True)
            step = quat_angle(r["poses"][:, :4], q0)
            assert r["trace"]["accept"][0] == 1 and (step > 0.5).sum() >= 2          # the device took the closed-form branch
    err = np.rad2deg(quat_angle(r["poses"][:, :4], w.truth_poses[:, :4]))
    assert err.max() < 0.5


# ---- pose optimisation -------------------------------------------------------------------------------------------------
_frames = {}


def pose_cases(k):
    """the frames of the pose tests in frame k, as pose_opt_batch takes them: (label, kwargs, is the hypothesis stage on)"""
    if k not in _frames:
        Rg = G.frame_R(k)
        f500 = synth.regauge_frame(synth.make_frame(n=500, seed=1001), Rg, G.TG, flip=(k % 2 == 1))
        f4000 = synth.regauge_frame(synth.make_frame(n=4000, seed=77), Rg, G.TG, flip=(k % 2 == 0), renormalise=False)
        fh0 = synth.make_frame(n=500, seed=1001, outlier_frac=0.55)
        fh = dict(synth.regauge_frame(fh0, Rg, G.TG), truth0=fh0["truth"])
        bad0 = _far_off_pose(fh["truth"], 150.0, np.array([2.0, -1.5, 1.7]))
        base = lambda f, hub, gate, **kw: dict(Xw=f["Xw"], obs=f["obs"], pose0=f["pose0"], cam=f["cam"], huber_delta=hub, chi2_gate=gate, **kw)   # noqa: E731
        _frames[k] = [("500 matches, gate 25", base(f500, 5.0, 25.0), f500), ("500 matches, gate 64", base(f500, 8.0, 64.0), f500),
                      ("4000 matches", base(f4000, 5.0, 25.0), f4000),
                      ("hypothesis stage", dict(base(fh, 5.0, 25.0, ransac_iters=50, ransac_seed=7), pose0=bad0), fh)]
    return _frames[k]


@pytest.mark.parametrize("k", range(4), ids=FRAME_IDS)
def test_pose_optimisation_in_the_four_frames(solver, oracle_mod, k):
    """tolerances of test_gpu_parity.test_pose_optimization_matches_oracle / ..._beyond_the_lds_staging_limit"""
    for label, kw, f in pose_cases(k)[:3]:
        r = solver.pose_opt(**kw)
        o = oracle_mod.pose_opt(kw["Xw"], kw["obs"], kw["pose0"], kw["cam"], kw["huber_delta"], kw["chi2_gate"])
        print(f"{label} in frame {FRAME_IDS[k]}: pose difference {np.abs(r['pose'] - o['pose']).max():.3g}, inliers {r['n_inliers']} / {o['n_inliers']}")
        assert r["status"] == 0 and r["n_inliers"] == o["n_inliers"]
        assert np.abs(r["pose"] - o["pose"]).max() < 1e-9
        mism = r["outlier"] != o["outlier"]
        assert (np.abs(o["chi2"][mism] - kw["chi2_gate"]) <= GUARD).all()
        np.testing.assert_allclose(r["chi2"], o["chi2"], rtol=1e-7, atol=1e-8)


@pytest.mark.parametrize("k", range(4), ids=FRAME_IDS)
def test_pose_hypothesis_stage_in_the_four_frames(solver, oracle_mod, built_lib, k):
    """test_gpu_parity's hypothesis-stage test (55 % outliers, 50 samples, seed 7, start pose 150 degrees off) in the four
    frames: the P3P winner is a rotation MATRIX and comes back through R2q - its branch by the largest diagonal entry in the
    three 175-degree frames"""
    label, kw, f = pose_cases(k)[3]
    samples = built_lib.ransac_samples(len(kw["Xw"]), 50, 7)
    o_r = oracle_mod.pose_ransac(kw["Xw"], kw["obs"], kw["pose0"], kw["cam"], kw["chi2_gate"], samples)
    o = oracle_mod.pose_opt(kw["Xw"], kw["obs"], o_r["pose"], kw["cam"], kw["huber_delta"], kw["chi2_gate"])
    r = solver.pose_opt(**kw)
    print(f"hypothesis stage in frame {FRAME_IDS[k]}: winner's difference {np.abs(r['ransac_pose'] - o_r['pose']).max():.3g}, "
          f"final pose difference {np.abs(r['pose'] - o['pose']).max():.3g}, trace of the winner {np.trace(synth.R_from_quat(r['ransac_pose'][:4])):.4f}")
    assert r["status"] == 0 and r["ransac_inliers"] == o_r["n_inliers"] >= 0.9 * (~f["is_outlier"]).sum()
    assert np.abs(r["ransac_pose"] - o_r["pose"]).max() < 1e-7
    assert r["n_inliers"] == o["n_inliers"] and np.abs(r["pose"] - o["pose"]).max() < 1e-8
    mism = r["outlier"] != o["outlier"]
    assert (np.abs(o["chi2"][mism] - kw["chi2_gate"]) <= GUARD).all()
    Rw = synth.R_from_quat(r["ransac_pose"][:4])
    want = G.FRAMES[k][3]
    if want is None:
        assert np.trace(Rw) > 0
    else:
        assert np.trace(Rw) < -0.9 and int(np.argmax(np.diag(Rw))) == want        # the branch was really taken
    assert ((r["outlier"] == 1) == f["is_outlier"]).mean() > 0.99
    pb, _ = G.back(r["pose"][None], np.zeros((1, 3)), k)               # (the generating truth, in the generator's frame)
    assert np.abs(pb[0, 4:] - f["truth0"][4:]).max() < 0.03 and quat_angle(pb[:, :4], f["truth0"][None, :4]).max() < 2e-3


def test_pose_batch_gives_the_general_position_frames_their_solo_bits(solver):
    cases = [kw for k in range(4) for _, kw, _ in pose_cases(k)]
    solo = [solver.pose_opt(**kw) for kw in cases]
    out = solver.pose_opt_batch(cases)
    assert len(out) == len(cases) == 16
    for b, s in zip(out, solo):
        assert b["status"] == 0
        for key in POSE_KEYS:
            np.testing.assert_array_equal(b[key], s[key], err_msg=key)


# ---- triangulation -------------------------------------------------------------------------------------------------------
def _tri(solver, sc):
    return solver.triangulate(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])


@pytest.mark.parametrize("i", range(3), ids=["mono", "stereo", "mixed"])
def test_triangulation_under_the_four_rotations(solver, i):
    sc = G.tri_scene(i)
    r0 = _tri(solver, sc)
    assert r0["status"] == 0
    TRI.compare_with_ref(r0, sc, f"{TRI.SCENES[i][0]} shrunk")
    ref = TRI.triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
    edge, _ = TRI.edge_alternatives(sc["views"], sc["pairs"], sc["matches"], ref, sc["reproj_gate"], sc["far_threshold"])
    for k in range(4):
        Rg = G.frame_R(k)
        sg = synth.regauge_triangulation(sc, Rg, flip_every=2)
        assert (sg["views"]["poses"][1::2, 3] < 0).all()
        rg = _tri(solver, sg)
        label = f"{TRI.SCENES[i][0]} shrunk, frame {FRAME_IDS[k]}"
        assert rg["status"] == 0
        TRI.compare_with_ref(rg, sg, label, lost_w=True)        # (the w = 0 match has w ~ 1e-17 in a rotated frame: see there)
        same = rg["code"] == r0["code"]
        assert (same | edge).all(), (label, np.flatnonzero(~same & ~edge)[:10])
        acc = same & np.isin(r0["code"], TRI.ACCEPTED)
        want = synth.regauge_points(r0["points"][acc], Rg)
        rel = np.linalg.norm(rg["points"][acc] - want, axis=1) / np.linalg.norm(want, axis=1)
        print(f"{label}: {int((~same).sum())} codes differ from the un-rotated call ({int(edge.sum())} matches on a gate), worst relative "
              f"difference to Rg x the un-rotated positions {rel.max():.3g} (POS_TOL {TRI.POS_TOL:.3g})")
        assert rel.max() <= TRI.POS_TOL, label


# ---- two-view ----------------------------------------------------------------------------------------------------------
def test_two_view_with_camera_2_rolled_about_its_optical_axis(solver):
    """The nine pairs of test_general_position_cpu.ROLL_SCENES (rolls of 180, 90 and -120 degrees).  `forward` at 180 degrees
    must initialise with trace(R) < -0.9: tv_R2q's branch for m[8] the largest diagonal entry.  Its branches for m[0] and m[4]
    stay untested: camera 2 would have to look backwards, and then no match lies in front of both cameras.  (`general` at 180
    degrees comes back TV_FEW_GOOD from the restatement and the library alike: hypotheses, counts and outcome are compared, its
    pose path is not exercised.)"""
    pairs = []
    for _, args, iters, seed in G.ROLL_SCENES:
        p = synth.make_two_view(**args)
        p.update(ransac_iters=iters, ransac_seed=seed)
        pairs.append(p)
    got = solver.two_view(pairs, diagnostics=True)
    n_tie = 0
    for g, p, (label, args, iters, seed) in zip(got, pairs, G.ROLL_SCENES):
        assert g["status"] == 0
        n_tie += TV.compare_with_ref(g, p, iters, seed, label, check_truth=True)["tie"]
        if args["scene"] == "forward" and args["roll_deg"] == 180.0:
            tr = np.trace(TV.q2R(g["pose"][:4]))
            print(f"{label}: outcome {g['outcome']}, trace {tr:.4f}, w {g['pose'][3]:.4f}")
            assert g["outcome"] == TV.TV_OK and tr < -0.9
    assert n_tie <= TV.TIE_CAP * len(pairs)
