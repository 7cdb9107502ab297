"""movba_stereo_points on the device against the restatement of tests/stereo_ref.py, every comparison exact equality, bit for bit,
but sel_point, which equals the header's own host walk bit for bit and the restatement within the derived bound 16 x 2^-53 x (|x| +
|y| + |z| + |Ow_k|): every gate at its boundary (next_pt.x -0.0, cols - 1, cols; a row difference of 4.0 and the float above; a
disparity of 0 with its double subtraction, the float below 0, max_disparity and the float below it; pt_status 0); distances
0.99999994, 1.0 and 2.0 around the truncation; the median rule with 1 and 2 candidates, an odd and an even count, median 0, (float)
dist == thDist, and points without a candidate; 0, 1, 63, 64, 65, 1 025, 4 097 and 16 384 points in a frame; the walk's lengths with
99 .. 102 candidates and 0, 100, 101, 150 close ones, max_point 0 and 1, equal depths, has_point mixed and absent, ALL, CLOSE and
NONE in one call; 1 024 tiny frames with runs of empty ones; a frame alone against the same frame in a batch; the same call
twice; pinned numbers; pinned result memory; a solved window on the same handle left as it was; a refusal and an empty call on a
live handle; and a synthetic rectified pair taken through Solver.lk_track, Solver.stereo_points and Solver.triangulate.
(tests/test_stereo_points_cpu.py holds the library's steps to the same cases under AddressSanitizer first, and checks that the
cases are what is said here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lk_ref as K
import stereo_ref as S
from conftest import ROOT
from movba import capi, synth

pytestmark = pytest.mark.gpu
F = np.float32


def test_every_gate_at_its_boundary_and_the_truncated_distances(solver):
    got = solver.stereo_points(S.gates_case())
    assert got["status"] == 0
    S.compare(got, S.gates_ref(), "gates")
    assert set(got["code"].tolist()) == {S.OK, S.REJ_STATUS, S.REJ_ROW, S.REJ_DISPARITY, S.REJ_FAR}
    for params in (dict(max_row_diff=1.5), dict(min_disparity=2.0), dict(min_disparity=-3.0, max_row_diff=0.0)):
        S.compare(solver.stereo_points(S.gates_case(), **params), S.ref_stereo(S.gates_case(), **params), f"gates, {params}")


def test_the_median_rule(solver):
    got = solver.stereo_points(S.median_case())
    S.compare(got, S.median_ref(), "median")
    assert got["median_dist"].tolist() == [3, 3, 3, 4, 0, S.exact_threshold()[0], -1, -1] and got["n_stereo"][4] == 0


def test_partly_filled_waves_several_waves_and_lds_at_its_limit(solver):
    got = solver.stereo_points(S.counts_case())
    S.compare(got, S.counts_ref(), "counts")
    assert np.diff(got["pt_ptr"])[:len(S.COUNTS)].tolist() == list(S.COUNTS)
    S.compare(solver.stereo_points(S.counts_case()), got, "the same call twice", point="exact")
    for key, value in S.PINNED["counts"].items():
        assert S.digest(got)[key] == value, key


def test_the_walks_lengths_equal_depths_and_the_three_selections(solver):
    got = solver.stereo_points(S.walk_case())
    S.compare(got, S.walk_ref(), "walk")
    assert np.diff(got["sel_ptr"])[:len(S.WALK)].tolist() == list(S.WALK_LENGTHS)
    for key, value in S.PINNED["walk"].items():
        assert S.digest(got)[key] == value, key
    for max_point in (0, 1, 7):
        S.compare(solver.stereo_points(S.walk_case(), max_point=max_point), S.ref_stereo(S.walk_case(), max_point=max_point), f"walk, max_point {max_point}")


def test_1024_frames_with_runs_of_empty_ones(solver):
    frames = S.frames_case()
    got = solver.stereo_points(frames)
    S.compare(got, S.frames_ref(), "frames")
    for f in S.FRAMES_ALONE:
        S.compare(solver.stereo_points([frames[f]]), S.frame_part(got, f), f"frames, frame {f} alone", point="exact")


def test_a_frame_alone_equals_the_frame_in_a_batch(solver):
    frames, ref = S.counts_case(), S.counts_ref()
    whole = solver.stereo_points(frames)
    for f in range(len(frames)):
        alone = solver.stereo_points([frames[f]])
        S.compare(alone, S.frame_part(ref, f), f"counts, frame {f} alone")
        S.compare(alone, S.frame_part(whole, f), f"counts, frame {f} alone against the batch", point="exact")
    # the other way round and in another order: the result follows the frame
    mixed = [frames[7], S.walk_case()[7], frames[2], S.gates_case()[1]]
    got = solver.stereo_points(mixed)
    S.compare(S.frame_part(got, 0), S.frame_part(whole, 7), "frame 7 first", point="exact")
    S.compare(S.frame_part(got, 1), S.frame_part(S.walk_ref(), 7), "a walk frame second")
    S.compare(S.frame_part(got, 2), S.frame_part(whole, 2), "frame 2 third", point="exact")
    S.compare(S.frame_part(got, 3), S.frame_part(S.gates_ref(), 1), "a gates frame last")


def test_sel_point_equals_the_headers_host_walk_bit_for_bit(solver, tmp_path):
    """tests/stereo_points/stereo_main.cpp runs stereo_points.h's serial walk: every field, sel_point included, is the device's to
    the bit - with poses near and far from the origin and without poses, where sel_point is (double)sel_cam"""
    st_dir = os.path.join(ROOT, "tests", "stereo_points")
    subprocess.check_call(["make", "-C", st_dir, "-s", "stereo_main"])         # (the plain build: no sanitizer runs beside the device)
    exe = os.path.join(st_dir, "stereo_main")
    for name in ("counts", "counts_nopose", "walk"):
        frames = S.CASES[name][0]()
        got = solver.stereo_points(frames)
        host = S.run_stereo_main(exe, frames, tmp_path)
        S.compare(got, host, name + ", the host walk", point="exact")
        total = int(got["sel_ptr"][-1])
        assert np.array_equal(got["sel_point"][:total].view(np.uint64), host["sel_point"][:total].view(np.uint64)), name
    got = solver.stereo_points(S.counts_nopose_case())
    total = int(got["sel_ptr"][-1])
    assert total > 500 and (got["sel_point"][:total] == got["sel_cam"][:total].astype(np.float64)).all()
    S.compare(got, S.counts_nopose_ref(), "counts without poses", point="exact")


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        for name in ("gates", "counts", "walk"):
            case, ref = S.CASES[name]
            pinned = s.stereo_points(case(), pinned=True)
            S.compare(pinned, s.stereo_points(case()), name + ", pinned", point="exact")
            S.compare(pinned, ref(), name + ", pinned against the restatement")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """A solved window's download before and after a call is bit-identical, later runs too; and the call gives after a solve,
    after a reset and between upload and run what it gives on a fresh handle."""
    w = synth.cfg("small")
    frames = S.walk_case()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")
    s = built_lib.Solver()
    try:
        first = s.solve(w)
        before = s.download()
        S.compare(s.stereo_points(frames), S.walk_ref(), "after the solve")
        after = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(first[k]), np.asarray(before[k])) and np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
        assert s._L.movba_lba_reset(s._h) == 0
        S.compare(s.stereo_points(frames, pinned=True), S.walk_ref(), "after the reset, pinned")
        s.run()
        again = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(again[k]), np.asarray(first[k])), k
        s.upload(w)
        S.compare(s.stereo_points(frames), S.walk_ref(), "between upload and run")
        s.run()
        fresh = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(fresh[k]), np.asarray(first[k])), k
    finally:
        s.close()


def test_a_refusal_and_an_empty_call_on_a_live_handle(solver):
    frames = S.gates_case()
    d, keep = capi.stereo_desc(frames)
    keep["select"][0] = 3
    r, out = capi.stereo_result(d.n_frames, len(keep["pt"]), alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
    r.status = 99
    assert solver._L.movba_stereo_points(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.stereo_points([dict(frames[0], bf=F(0))])
    # no frames: MOVBA_OK, and not one result entry is written
    d.n_frames = 0
    r.status = 99
    assert solver._L.movba_stereo_points(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    assert solver.stereo_points([])["status"] == 0
    # frames without points
    none = [S.make_frame(np.zeros((0, 2)), np.zeros((0, 2)), select=sel) for sel in (S.CLOSE, S.ALL, S.NONE)]
    got = solver.stereo_points(none)
    assert got["status"] == 0 and got["sel_ptr"].tolist() == [0, 0, 0, 0] and got["median_dist"].tolist() == [-1, -1, -1] and got["n_stereo"].tolist() == [0, 0, 0]
    S.compare(solver.stereo_points(frames), S.gates_ref(), "after the refusal")


def test_a_rectified_pair_chains_from_lk_track_through_stereo_points_into_triangulate(solver):
    """Frame.cc:281-354 on a synthetic rectified pair: the right image is the left one's texture moved left by 1.5, 3 and 4.5 pixels
    in three bands of rows (the texture's finest waves are under two pixels long, which larger shifts alias with).  Solver.lk_track (window 21, the reference's parameters) tracks a grid of points left to right; its pt,
    next_pt and pt_status go into Solver.stereo_points as they are, which is held to the restatement fed the same arrays; and
    u_right and depth, converted to float64, are the ur1 and depth1 of Solver.triangulate, which un-projects the same points."""
    rows, cols, band = 144, 192, 48
    disparities = (1.5, 3.0, 4.5)
    left = K.texture(rows, cols, 5, (0, 0), 1)
    right = np.vstack([K.texture(rows, cols, 5, (int(-8 * dsp), 0), 1)[k * band:(k + 1) * band] for k, dsp in enumerate(disparities)])
    pts = np.array([(x, y) for y in range(8, rows, 9) for x in range(24, cols - 8, 11)], F)
    lk = solver.lk_track([dict(prev=left, next=right, win=21, pt=pts)])
    K.compare(lk, K.ref_lk([dict(prev=left, next=right, win=21, pt=pts)]), "chain: the track")
    fx, fy, cx, cy = F(210.0), F(208.0), F(95.5), F(71.5)
    bf = F(21.0)                                                # a baseline of 0.1
    b = bf / fx
    fr = dict(pt=pts, next_pt=lk["next_pt"], pt_status=lk["pt_status"], rows=rows, cols=cols, bf=bf, max_disparity=bf / b, th_depth=F(35.0) * b,
              cam=(fx, fy, cx, cy), select=S.ALL)
    got = solver.stereo_points([fr])
    want = S.ref_stereo([fr])
    S.compare(got, want, "chain: the depths", point="exact")
    inner = np.array([band // 4 <= y % band < 3 * band // 4 for _, y in pts])          # away from the seams between the bands
    ok = got["code"] == S.OK
    assert ok[inner].mean() > 0.9 and got["n_stereo"][0] == ok.sum() == got["sel_ptr"][1] and got["median_dist"][0] in (2, 3)
    truth = np.array([disparities[int(y) // band] for _, y in pts], F)
    measured = pts[:, 0] - got["u_right"]
    assert np.abs(measured - truth)[ok & inner].max() < 0.25 and np.abs(got["depth"] * measured - bf)[ok].max() < 1e-4
    # the layouts join without reshaping: every point of the frame, stereo or not, is a match of one keyframe pair
    total = int(got["sel_ptr"][1])
    other = np.array([0, 0, 0, 1, -0.05, 0, 0], np.float64)     # Tcw of a keyframe 5 cm to the right: less parallax than the rig's
    X = np.full((len(pts), 3), np.nan)
    X[got["sel_src"][:total]] = got["sel_point"][:total]
    obs2 = np.where(np.isnan(X[:, :1]), pts.astype(np.float64) - (1.0, 0.0),
                    np.stack([fx * (X[:, 0] - 0.05) / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], axis=1))
    views = dict(poses=np.stack([np.array([0, 0, 0, 1, 0, 0, 0], np.float64), other]), cam=np.array([[fx, fy, cx, cy]] * 2, np.float64),
                 bf=np.array([bf, bf], np.float64), b=np.array([b, b], np.float64))
    tri = solver.triangulate(views, dict(pair_view=np.array([[0, 1]], np.int32), pair_ptr=np.array([0, len(pts)], np.int32)),
                             dict(obs1=pts.astype(np.float64), obs2=obs2, ur1=got["u_right"].astype(np.float64), depth1=got["depth"].astype(np.float64)))
    assert tri["status"] == 0 and (tri["code"][ok] == capi.TRI_STEREO1).all() and (tri["code"][~ok] != capi.TRI_STEREO1).all()
    # (the same point un-projected in fp64 there and in fp32 here: a subtraction, a reciprocal and two products, four roundings of
    # 2^-24 each per component, a fifth for their second-order terms and the fp64 side; the poses are the identity)
    assert np.allclose(tri["points"][got["sel_src"][:total]], got["sel_point"][:total], rtol=5 * 2.0 ** -24, atol=0)
