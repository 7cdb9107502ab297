"""The C++ Optimizer adapter (mov-slam_amd/host/Optimizer.cc: the reference's Optimizer.h call
surface over mock map classes) end to end on the GPU: LocalBundleAdjustment, GlobalBundleAdjustemnt
and PoseOptimization must leave in the map what the oracle computes from the same inputs, after the
float32 casts the reference applies on write-back (src/Optimizer.cc:827, 836)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, quat_angle
from movba import synth

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "mov-slam_amd", "host")
BIN = os.path.join(HOST, "adapter_test")


@pytest.fixture(scope="module")
def adapter_bin(built_lib):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST, "-s"])
    return BIN


def _f32_pose(p):
    """what KeyFrame::GetPose() holds: float quaternion normalised in float (Sophus), float translation."""
    p = np.asarray(p, np.float32).copy()
    q = p[..., :4]
    n = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    p[..., :4] = q / n[..., None]
    return p.astype(np.float64)


def _write_window(path, w, bad_kf=-1, levels=None):
    """bad_kf: index of a keyframe the mock map flags bad (KeyFrame::isBad()), -1 = none; levels: the pyramid level of every
    edge's keypoint (cv::KeyPoint::octave; none: level 0 everywhere) - the mock keyframes hold the 1.2 pyramid's
    mvInvLevelSigma2, synth.level_inv_sigma2()"""
    with open(path, "wb") as f:
        f.write(struct.pack("4i", w.n_poses, w.n_points, w.n_edges, bad_kf + 1))
        f.write(np.ascontiguousarray(w.pose_fixed, np.uint8).tobytes())
        f.write(np.ascontiguousarray(w.poses, np.float64).tobytes())
        f.write(np.ascontiguousarray(w.points, np.float64).tobytes())
        f.write(np.ascontiguousarray(w.edge_pose, np.int32).tobytes())
        f.write(np.ascontiguousarray(w.edge_point, np.int32).tobytes())
        f.write(np.ascontiguousarray(w.obs, np.float64).tobytes())
        has_cams = getattr(w, "cam_kf", None) is not None
        if getattr(w, "obs_right", None) is not None:
            f.write(struct.pack("d", w.bf)); f.write(np.ascontiguousarray(w.obs_right, np.float64).tobytes())
        elif has_cams or levels is not None:          # (the camera and octave trailers sit behind the stereo one)
            f.write(struct.pack("d", 0.0)); f.write(np.full(w.n_edges, -1.0).tobytes())
        if has_cams:
            f.write(struct.pack("i", 0x43414d31)); f.write(np.ascontiguousarray(w.cam_kf, np.float64).tobytes())
            bfk = w.bf_kf if getattr(w, "bf_kf", None) is not None else np.zeros(w.n_poses)
            f.write(np.ascontiguousarray(bfk, np.float64).tobytes())
        if levels is not None:
            assert len(levels) == w.n_edges
            f.write(struct.pack("i", 0x4f435431)); f.write(np.ascontiguousarray(levels, np.int32).tobytes())


def _read_out(path, w):
    b = open(path, "rb").read()
    hd = struct.unpack_from("5i", b, 0); off = 20
    poses = np.frombuffer(b, np.float32, 7 * w.n_poses, off).reshape(-1, 7); off += 28 * w.n_poses
    points = np.frombuffer(b, np.float32, 3 * w.n_points, off).reshape(-1, 3); off += 12 * w.n_points
    erased = np.frombuffer(b, np.int32, 2 * hd[3], off).reshape(-1, 2); off += 8 * hd[3]
    tail = struct.unpack_from("2i", b, off); off += 8
    counts = struct.unpack_from("2i", b, off); off += 8
    nd = np.frombuffer(b, np.float32, 5 * w.n_points, off).reshape(-1, 5); off += 20 * w.n_points
    timing = struct.unpack_from("3d", b, off); off += 24
    pt = np.frombuffer(b, np.int32, 4 * w.n_points, off).reshape(-1, 4); off += 16 * w.n_points
    kf_live = np.frombuffer(b, np.int32, w.n_poses, off); off += 4 * w.n_poses
    st = struct.unpack_from("3i", b, off)
    return dict(point_bad=pt[:, 0], point_nobs=pt[:, 1], point_nleft=pt[:, 2], point_ref=pt[:, 3], kf_live=kf_live,
                last_status=st[0], error_count=st[1], n_map_erased=st[2],num_fixedKF=hd[0], num_OptKF=hd[1], num_edges=hd[2], n_erased=hd[3], change_idx=hd[4],
                poses=poses, points=points, erased=erased, n_pose_sets=tail[0], n_normal_updates=tail[1],
                n_observation_copies=counts[0], n_center_reads=counts[1], normals=nd[:, :3], dist=nd[:, 3:], timing_ms=timing)


def _check_map(out, o, w, moved):
    assert quat_angle(out["poses"][:, :4].astype(np.float64), _f32_pose(o["poses"])[:, :4]).max() < 2e-6
    np.testing.assert_allclose(out["poses"][:, 4:], o["poses"][:, 4:].astype(np.float32), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(out["points"], o["points"].astype(np.float32), rtol=2e-6, atol=2e-6)
    assert out["n_pose_sets"] == moved and out["n_normal_updates"] == w.n_points     # BundleAdjustment keeps the reference's per-point update


def _local_subwindow(w):
    """What Optimizer::LocalBundleAdjustment selects (Optimizer.cc:464-523): the map points seen by at least one
    local (free) keyframe, and the fixed keyframes that observe those points."""
    free = w.pose_fixed == 0
    local_pt = np.zeros(w.n_points, bool); local_pt[w.edge_point[free[w.edge_pose]]] = True
    keep_e = local_pt[w.edge_point]
    used_pose = free.copy(); used_pose[w.edge_pose[keep_e]] = True
    pmap = -np.ones(w.n_poses, int); pmap[used_pose] = np.arange(used_pose.sum())
    lmap = -np.ones(w.n_points, int); lmap[local_pt] = np.arange(local_pt.sum())
    sub = synth.Window(poses=w.poses[used_pose], pose_fixed=w.pose_fixed[used_pose], points=w.points[local_pt],
                       edge_pose=pmap[w.edge_pose[keep_e]].astype(np.int32), edge_point=lmap[w.edge_point[keep_e]].astype(np.int32),
                       obs=w.obs[keep_e], inv_sigma2=w.inv_sigma2[keep_e], cam=w.cam, huber_delta=w.huber_delta,
                       chi2_gate=w.chi2_gate, max_iters=w.max_iters)
    if getattr(w, "obs_right", None) is not None:
        sub.obs_right, sub.bf = w.obs_right[keep_e], w.bf
    if getattr(w, "cam_kf", None) is not None:
        sub.cam_kf = w.cam_kf[used_pose]
        sub.bf_kf = w.bf_kf[used_pose] if getattr(w, "bf_kf", None) is not None else None
    return sub, used_pose, local_pt, keep_e


@pytest.mark.parametrize("name", ["small", "cfg2", "cfg3", "stereo", "cameras", "stereo-cameras", "levels"])
def test_local_bundle_adjustment_through_the_adapter(adapter_bin, oracle_mod, tmp_path, name):
    # "cfg3": the window the headline is quoted on (50 + 10 keyframes x 20 000 map points), map content checked like the small ones
    # "stereo": a window whose keyframes hold stereo observations (mvuRight >= 0, Optimizer.cc:673-705)
    # "cameras": every keyframe with a GeometricCamera (and mbf) of its own, three different ones in the window
    # (e->pCamera = pKFi->mpCamera, Optimizer.cc:664; e->bf = pKFi->mbf, :695)
    # "levels": keypoints on all eight pyramid levels, the edge's information looked up by octave (Optimizer.cc:657-658); the
    # oracle solves the window with inv_sigma2 from the same table
    lv = None
    if name.startswith("stereo"):
        w = synth.make_window(6, 2, 150, seed=43, run_lo=2, run_hi=5, stereo_frac=0.7)
    else:
        w = synth.cfg("small" if name in ("cameras", "levels") else name)
    if name.endswith("cameras"):
        w = synth.mixed_cameras(w, seed=44)
    if name == "levels":
        w, lv = synth.with_levels(w, seed=1)
        assert len(np.unique(w.inv_sigma2)) == 8
    w.poses = _f32_pose(w.poses)                     # the doubles the adapter derives from the float map
    fin, fout = str(tmp_path / "w.bin"), str(tmp_path / "o.bin")
    _write_window(fin, w, levels=lv)
    subprocess.check_call([adapter_bin, "lba", fin, fout])
    out = _read_out(fout, w)
    sub, used_pose, local_pt, keep_e = _local_subwindow(w)
    o = oracle_mod.solve(sub)
    K = w.n_free
    assert (out["num_fixedKF"], out["num_OptKF"], out["num_edges"]) == (int(used_pose.sum()) - K, K, sub.n_edges)
    assert out["change_idx"] == 1                     # IncreaseChangeIndex (Optimizer.cc:840)
    # expected map content: optimised values for the window, everything else untouched
    exp_poses = w.poses.copy(); exp_poses[used_pose] = o["poses"]
    exp_points = w.points.copy(); exp_points[local_pt] = o["points"]
    assert quat_angle(out["poses"][:, :4].astype(np.float64), _f32_pose(exp_poses)[:, :4]).max() < 2e-6
    np.testing.assert_allclose(out["poses"][:, 4:], exp_poses[:, 4:].astype(np.float32), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(out["points"], exp_points.astype(np.float32), rtol=2e-6, atol=2e-6)
    assert out["n_pose_sets"] == K                    # SetPose on the local keyframes only (Optimizer.cc:822-829)
    # ONE std::map copy per local map point for the whole call (the reference takes three), the camera centres
    # read once per window keyframe, and normal / depth stored from the GPU result without MapPoint::UpdateNormalAndDepth
    assert out["n_observation_copies"] == int(local_pt.sum())
    assert out["n_normal_updates"] == 0 and out["n_center_reads"] == int(used_pose.sum())
    # ... with exactly what UpdateNormalAndDepth computes: the same run with the reference's per-point update
    env = dict(os.environ, MOVBA_ADAPTER_REFERENCE_NORMALS="1")
    fout2 = str(tmp_path / "o2.bin")
    subprocess.check_call([adapter_bin, "lba", fin, fout2], env=env)
    ref = _read_out(fout2, w)
    assert ref["n_normal_updates"] == int(local_pt.sum()) and ref["n_center_reads"] > out["n_center_reads"]
    assert np.array_equal(out["normals"], ref["normals"]) and np.array_equal(out["dist"], ref["dist"])
    assert np.array_equal(out["poses"], ref["poses"]) and np.array_equal(out["points"], ref["points"])
    live = out["dist"][:, 1] > 0                       # (points left with <= 2 observations went bad: never updated)
    assert live.sum() > 0.8 * local_pt.sum() and not live[~local_pt].any()
    assert np.linalg.norm(out["normals"][live], axis=1).max() <= 1.0 + 1e-6 and (out["dist"][live, 1] > out["dist"][live, 0]).all()
    # erased (KeyFrame, MapPoint) pairs == the oracle's outliers, up to the chi2 guard band — for the points that stay in the
    # map; a point left with nObs <= 2 (a stereo observation counts twice, MapPoint.cc:162-165, 184-190) goes through
    # SetBadFlag: its remaining observations vanish without further EraseObservation calls, its observers' slots are nulled
    ep, el = w.edge_pose[keep_e], w.edge_point[keep_e]
    want = set(map(tuple, np.stack([ep, el], 1)[o["outlier"] == 1]))
    got = set(map(tuple, out["erased"]))
    guard = {(int(a), int(b)) for a, b, c in zip(ep, el, o["chi2"]) if abs(c - 5.0) < 1e-4}
    guard_pts = {b for _, b in guard}
    wt = np.ones(w.n_edges, int) if getattr(w, "obs_right", None) is None else np.where(w.obs_right >= 0, 2, 1)
    out_full = np.zeros(w.n_edges, bool); out_full[np.flatnonzero(keep_e)[o["outlier"] == 1]] = True
    nobs0 = np.bincount(w.edge_point, wt, w.n_points).astype(int)
    nobs1 = np.bincount(w.edge_point, wt * ~out_full, w.n_points).astype(int)
    bad_exp = (nobs1 <= 2) & (nobs1 < nobs0)                  # went bad in THIS call (an erase is what triggers the test)
    for l in range(w.n_points):
        if l in guard_pts:
            continue
        assert out["point_bad"][l] == int(bad_exp[l]), l
        wl, gl = {p for p in want if p[1] == l}, {p for p in got if p[1] == l}
        if bad_exp[l]:
            assert gl <= wl and out["point_nleft"][l] == 0
        else:
            assert gl == wl and out["point_nobs"][l] == nobs1[l]
            # the reference keyframe survives unless its own observation went; then it is the lowest remaining observer
            obs_l = w.edge_pose[(w.edge_point == l) & ~out_full]
            first = int(w.edge_pose[w.edge_point == l][0])
            assert out["point_ref"][l] == (first if first in obs_l else int(obs_l.min()))
    assert out["n_erased"] == len(got)
    if not guard_pts:
        assert out["n_map_erased"] == int(bad_exp.sum())          # Map::EraseMapPoint once per point that went bad
    # every observer's slot of an erased or vanished observation is nulled, the others are still set
    if not guard_pts:
        gone = out_full | bad_exp[w.edge_point]
        assert np.array_equal(out["kf_live"], np.bincount(w.edge_pose, ~gone, w.n_poses).astype(int))
    assert out["last_status"] == 0 and out["error_count"] == 0
    if name == "stereo":
        # a mixed window: monocular outliers are erased before stereo ones (Optimizer.cc:760-803), and some erased observer was
        # its point's reference keyframe
        is_st = {(int(a), int(b)) for a, b, r in zip(w.edge_pose, w.edge_point, w.obs_right) if r >= 0}
        seqs = {}
        for a, b in out["erased"]:                        # (listed per point in call order)
            seqs.setdefault(int(b), []).append((int(a), int(b)) in is_st)
        assert all(q == sorted(q) for q in seqs.values())                     # per point: monocular erasures first
        assert any(len(set(q)) == 2 for q in seqs.values())                   # ... and some point had both kinds
        firsts = {l: int(w.edge_pose[w.edge_point == l][0]) for l in set(el)}
        assert any(firsts[b] == a for a, b in got)                            # an erased observer was its point's reference keyframe


def test_adapter_dumps_replayable_windows(adapter_bin, solver, oracle_mod, tmp_path):
    """MOVBA_DUMP_DIR: the adapter writes the flattened window it solved; replaying the file through the
    C-ABI gives the same result, and the keyframe-trajectory ATE of GPU and oracle solutions agree (cfg4 harness)."""
    from movba import ate, capture
    _dump_and_replay(adapter_bin, solver, oracle_mod, tmp_path, synth.cfg("small"), None, ate, capture)
    # ... and a window with keypoints on all eight pyramid levels: the dump and capture.py carry every edge's weight through
    (tmp_path / "levels").mkdir()
    w, lv = synth.with_levels(synth.cfg("small"), seed=2)
    _dump_and_replay(adapter_bin, solver, oracle_mod, tmp_path / "levels", w, lv, ate, capture)


def _dump_and_replay(adapter_bin, solver, oracle_mod, tmp_path, w, lv, ate, capture):
    w.poses = _f32_pose(w.poses)
    fin, fout = str(tmp_path / "w.bin"), str(tmp_path / "o.bin")
    _write_window(fin, w, levels=lv)
    env = dict(os.environ, MOVBA_DUMP_DIR=str(tmp_path))
    subprocess.check_call([adapter_bin, "lba", fin, fout], env=env)
    dumped = capture.load_window(str(tmp_path / "lba_000000.mbw"))
    sub, used_pose, local_pt, keep_e = _local_subwindow(w)
    assert dumped.n_poses == sub.n_poses and dumped.n_points == sub.n_points and dumped.n_edges == sub.n_edges
    np.testing.assert_array_equal(dumped.poses, sub.poses)
    # map points arrive in the adapter's first-seen order (Optimizer.cc:479-504), not by id: same multiset of edges
    np.testing.assert_array_equal(np.sort(dumped.obs.ravel()), np.sort(sub.obs.ravel()))
    # ... each with its own weight: an edge is known by its keyframe and its observation
    rows = lambda x: np.stack([x.edge_pose.astype(np.float64), x.obs[:, 0], x.obs[:, 1], x.inv_sigma2], 1)
    a, b = rows(dumped), rows(sub)
    assert len(np.unique(b[:, :3], axis=0)) == sub.n_edges
    np.testing.assert_array_equal(a[np.lexsort(a[:, 2::-1].T)], b[np.lexsort(b[:, 2::-1].T)])
    assert len(np.unique(dumped.inv_sigma2)) == (1 if lv is None else 8)
    r, o = solver.solve(dumped), oracle_mod.solve(dumped)
    assert np.abs(r["poses"] - o["poses"]).max() < 1e-8
    # ATE of the optimised keyframe trajectory against the generating truth: GPU within 1e-6 relative of the oracle
    truth = np.zeros((sub.n_poses, 7)); T = w.truth_poses[used_pose]
    rows_t = ate.kf_trajectory_rows(T, range(sub.n_poses))
    truth[:, :3] = ate.kitti_to_tartan_xyz(rows_t[:, 1:]); truth[:, 6] = 1
    a_gpu = ate.ate_tartanair(truth, ate.kf_trajectory_rows(r["poses"], range(sub.n_poses)))["ate"]
    a_cpu = ate.ate_tartanair(truth, ate.kf_trajectory_rows(o["poses"], range(sub.n_poses)))["ate"]
    assert abs(a_gpu - a_cpu) <= 1e-6 * max(a_cpu, 1e-12) + 1e-12


def test_global_bundle_adjustment_through_the_adapter(adapter_bin, oracle_mod, tmp_path):
    """Tracking::CreateInitialMapMonocular -> GlobalBundleAdjustemnt (Tracking.cc:688): only the init keyframe
    is fixed, nothing is erased, results are written directly when nLoopKF is the origin keyframe."""
    w = synth.cfg("small")
    w.poses = _f32_pose(w.poses)
    fin, fout = str(tmp_path / "w.bin"), str(tmp_path / "o.bin")
    _write_window(fin, w)
    subprocess.check_call([adapter_bin, "gba", fin, fout])
    out = _read_out(fout, w)
    wg = synth.cfg("small"); wg.poses = w.poses
    wg.pose_fixed = np.zeros_like(w.pose_fixed); wg.pose_fixed[0] = 1
    o = oracle_mod.solve(wg, max_iters=10)
    _check_map(out, o, w, moved=w.n_poses)
    assert out["n_erased"] == 0 and out["change_idx"] == 0


@pytest.mark.parametrize("is_lost", [0, 1])
def test_pose_optimization_through_the_adapter(adapter_bin, oracle_mod, tmp_path, is_lost):
    f = synth.make_frame()
    pose0 = _f32_pose(f["pose0"])
    fin, fout = str(tmp_path / "p.bin"), str(tmp_path / "po.bin")
    n = len(f["Xw"])
    with open(fin, "wb") as fh:
        fh.write(struct.pack("2i", n, is_lost))
        fh.write(np.ascontiguousarray(f["Xw"], np.float64).tobytes())
        fh.write(np.ascontiguousarray(f["obs"], np.float64).tobytes())
        fh.write(np.ascontiguousarray(pose0, np.float64).tobytes())
    subprocess.check_call([adapter_bin, "pose", fin, fout])
    b = open(fout, "rb").read()
    ninl = struct.unpack_from("i", b, 0)[0]
    pose = np.frombuffer(b, np.float32, 7, 4)
    outl = np.frombuffer(b, np.uint8, n + 3, 32)
    rep = 8.0 if is_lost else 5.0                    # reprojectErrorLost / reprojectionError defaults (Optimizer.h:55)
    # iterationCount = 50 P3P hypotheses from the adapter's fixed seed, then the LM from the best of them
    from movba import capi
    samples = capi.ransac_samples(n, 50, 20221105)
    # (confidence = 0.95 as Optimizer.h:55 defaults it: the stopping rule; one local-optimisation step of 10 iterations)
    o_r = oracle_mod.pose_ransac(f["Xw"], f["obs"], pose0, f["cam"], rep * rep, samples, confidence=0.95, lo_its=10)
    assert o_r["n_inliers"] >= 0.8 * (~f["is_outlier"]).sum() and o_r["samples_used"] < 50
    o = oracle_mod.pose_opt(f["Xw"], f["obs"], o_r["pose"], f["cam"], rep, rep * rep, rounds=4, its=10)
    assert ninl == o["n_inliers"]
    assert np.abs(pose.astype(np.float64) - _f32_pose(o["pose"])).max() < 2e-6
    assert np.array_equal(outl[:n], o["outlier"]) and (outl[n:] == 1).all()   # slots without a MapPoint stay "outlier"


def test_local_bundle_adjustment_with_a_bad_observer(adapter_bin, oracle_mod, tmp_path):
    """A fixed keyframe flagged bad (KeyFrame::isBad(), Optimizer.cc:515): it gets no vertex and its observations no edges,
    so some local points have fewer edges than observations — the flattener's gap-closing path — and the result is the
    optimum of the window without those edges; the bad keyframe itself is left alone."""
    _bad_observer(adapter_bin, oracle_mod, tmp_path, synth.cfg("small"), None)


def test_local_bundle_adjustment_with_a_bad_observer_and_level_weights(adapter_bin, oracle_mod, tmp_path):
    """The same with keypoints on all eight pyramid levels: closing the gaps moves inv_sigma2 along with the observations
    (Optimizer.cc:685-699); an edge left with a neighbour's weight gives another optimum (tests/test_level_weights_cpu.py)."""
    w, lv = synth.with_levels(synth.cfg("small"), seed=2)
    _bad_observer(adapter_bin, oracle_mod, tmp_path, w, lv)


def _bad_observer(adapter_bin, oracle_mod, tmp_path, w, lv):
    w.poses = _f32_pose(w.poses)
    fixed_idx = np.flatnonzero(w.pose_fixed == 1)
    b = int(fixed_idx[np.argmax(np.bincount(w.edge_pose, minlength=w.n_poses)[fixed_idx])])
    fin, fout = str(tmp_path / "w.bin"), str(tmp_path / "o.bin")
    _write_window(fin, w, bad_kf=b, levels=lv)
    subprocess.check_call([adapter_bin, "lba", fin, fout])
    out = _read_out(fout, w)
    keep = w.edge_pose != b
    assert (~keep).sum() > 0
    w2 = synth.cfg("small"); w2.poses = w.poses
    w2.edge_pose, w2.edge_point, w2.obs, w2.inv_sigma2 = w.edge_pose[keep], w.edge_point[keep], w.obs[keep], w.inv_sigma2[keep]
    sub, used_pose, local_pt, keep_e = _local_subwindow(w2)
    assert not used_pose[b]
    o = oracle_mod.solve(sub)
    K = w.n_free
    assert (out["num_fixedKF"], out["num_OptKF"], out["num_edges"]) == (int(used_pose.sum()) - K, K, sub.n_edges)
    exp_poses = w.poses.copy(); exp_poses[used_pose] = o["poses"]
    exp_points = w.points.copy(); exp_points[local_pt] = o["points"]
    assert quat_angle(out["poses"][:, :4].astype(np.float64), _f32_pose(exp_poses)[:, :4]).max() < 2e-6
    np.testing.assert_allclose(out["poses"][:, 4:], exp_poses[:, 4:].astype(np.float32), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(out["points"], exp_points.astype(np.float32), rtol=2e-6, atol=2e-6)
    ep, el = w2.edge_pose[keep_e], w2.edge_point[keep_e]
    want = set(map(tuple, np.stack([ep, el], 1)[o["outlier"] == 1]))
    got = set(map(tuple, out["erased"]))
    guard = {(int(a), int(c)) for a, c, x in zip(ep, el, o["chi2"]) if abs(x - 5.0) < 1e-4}
    # (a point that went bad on the way — nObs <= 2 — lost its remaining observations without further EraseObservation calls)
    alive = lambda pairs: {p for p in pairs if not out["point_bad"][p[1]]}
    assert (alive(want) ^ alive(got)) <= guard and got <= (want | guard)


@pytest.mark.parametrize("name", ["small", "cfg2", "stereo"])
def test_adapter_with_the_for_each_observation_accessor(adapter_bin, tmp_path, name):
    """-DMOVBA_MAPPOINT_HAS_FOR_EACH_OBSERVATION (the second optional accessor INTEGRATION.md offers MapPoint.h): the
    observations are visited under the point's lock instead of being copied as a std::map: no copy at all, same map."""
    exe = os.path.join(HOST, "adapter_test_foreach")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "-s"])
    w = synth.make_window(6, 2, 150, seed=43, run_lo=2, run_hi=5, stereo_frac=0.7) if name == "stereo" else synth.cfg(name)
    w.poses = _f32_pose(w.poses)
    fin, fa, fb = str(tmp_path / "w.bin"), str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    _write_window(fin, w)
    subprocess.check_call([adapter_bin, "lba", fin, fa])
    subprocess.check_call([exe, "lba", fin, fb])
    a, b = _read_out(fa, w), _read_out(fb, w)
    assert a["n_observation_copies"] > 0 and b["n_observation_copies"] == 0
    for k in ("poses", "points", "erased", "normals", "dist"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("num_fixedKF", "num_OptKF", "num_edges", "n_erased", "change_idx", "n_pose_sets", "n_normal_updates", "n_center_reads"):
        assert a[k] == b[k], k
