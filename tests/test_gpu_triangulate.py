"""movba_triangulate on the device against the numpy restatement of tests/test_triangulate_cpu.py (triangulate_ref): decision by
decision and position by position (compare_with_ref: codes equal except on matches that sit on a gate, positions within
POS_TOL, NaN where the restatement has NaN, n_accepted the count of accepted codes), independence of a match from everything
but itself and its two views (bit-identical however the matches are split, ordered or accompanied), pinned result arrays,
invalid calls, a window on the same handle left as it was, and the accepted points taken through movba_lba_solve."""
import copy
import ctypes as C

import numpy as np
import pytest

from movba import synth
from test_triangulate_cpu import ACCEPTED, SCENES, compare_with_ref, quirk_cases, scene, triangulate_ref

pytestmark = pytest.mark.gpu


def _run(solver, sc, **kw):
    return solver.triangulate(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"], **kw)


def _same_bits(a, b, label=""):
    assert np.array_equal(a["code"], b["code"]), label
    assert np.array_equal(a["points"].view(np.uint64), b["points"].view(np.uint64)), label


@pytest.mark.parametrize("label,args", SCENES + [
    ("one pair", dict(n_pairs=1, n_per_pair=3000, seed=7110)),
    ("pairs of very different sizes, empty ones among them", dict(n_pairs=12, n_per_pair=[5000, 0, 1, 0, 0, 37, 255, 256, 257, 0, 9000, 2], seed=7111, stereo=True, stereo_frac=0.5)),
    ("forty tiny pairs in one workgroup", dict(n_pairs=40, n_per_pair=[1 + (k % 5) for k in range(40)], seed=7112)),
    ("one match", dict(n_pairs=1, n_per_pair=1, seed=7113)),
    ("200 000 matches", dict(n_pairs=100, n_per_pair=2000, seed=7114, stereo=True, stereo_frac=0.3)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_scenes_match_the_restatement(solver, label, args):
    sc = scene(args)
    r = _run(solver, sc)
    assert r["status"] == 0
    compare_with_ref(r, sc, label)
    _same_bits(_run(solver, sc), r, "two calls")


def test_hand_made_quirk_cases(solver):
    for label, (sc, ref), want in quirk_cases():
        r = _run(solver, sc)
        assert r["code"][0] == ref["code"][0] and (want is None or r["code"][0] == want), label
        assert np.array_equal(np.isnan(r["points"]), np.isnan(ref["points"])), label
        if not np.isnan(ref["points"]).any():
            assert np.allclose(r["points"], ref["points"], rtol=1e-9, atol=0), label


def _subset(sc, pairs_idx):
    """the scene restricted to the given pairs, in the given order"""
    ptr = sc["pairs"]["pair_ptr"]
    idx = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in pairs_idx]) if len(pairs_idx) else np.zeros(0, np.int64)
    sizes = [int(ptr[p + 1] - ptr[p]) for p in pairs_idx]
    out = dict(sc)
    out["pairs"] = dict(pair_view=sc["pairs"]["pair_view"][list(pairs_idx)],
                        pair_ptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    out["matches"] = {k: v[idx] for k, v in sc["matches"].items()}
    return out, idx


def test_a_match_depends_on_nothing_but_itself_and_its_views(solver):
    sc = scene(dict(n_pairs=9, n_per_pair=[700, 3, 0, 1200, 64, 1, 300, 0, 513], seed=7120, stereo=True, stereo_frac=0.5))
    whole = _run(solver, sc)
    compare_with_ref(whole, sc, "whole")
    # split into several calls
    for part in ([0, 1, 2], [3], [4, 5, 6, 7, 8], [8]):
        sub, idx = _subset(sc, part)
        r = _run(solver, sub)
        assert np.array_equal(r["code"], whole["code"][idx]) and np.array_equal(r["points"].view(np.uint64), whole["points"][idx].view(np.uint64)), part
    # every pair cut in two at an odd place: its matches land in other lanes, waves and workgroups
    ptr = sc["pairs"]["pair_ptr"]
    cuts = np.unique(np.concatenate([ptr, (ptr[:-1] + (np.diff(ptr) * 0.37).astype(np.int32))]))
    pair_of_piece = np.searchsorted(ptr, cuts[:-1], side="right") - 1
    pieces = dict(sc)
    pieces["pairs"] = dict(pair_view=sc["pairs"]["pair_view"][pair_of_piece], pair_ptr=cuts.astype(np.int32))
    _same_bits(_run(solver, pieces), whole, "pairs cut in two")
    # the pairs permuted
    perm = np.random.default_rng(5).permutation(9)
    sub, idx = _subset(sc, perm)
    r = _run(solver, sub)
    assert np.array_equal(r["code"], whole["code"][idx]) and np.array_equal(r["points"].view(np.uint64), whole["points"][idx].view(np.uint64))
    # unrelated pairs added in front and behind (other views, other cameras' worth of matches)
    other = scene(dict(n_pairs=4, n_per_pair=[130, 0, 2000, 77], seed=7121, stereo=True))
    both = synth.concat_triangulations([other, sc, other])
    r = _run(solver, both)
    n0 = int(other["pairs"]["pair_ptr"][-1]); n1 = int(ptr[-1])
    assert np.array_equal(r["code"][n0:n0 + n1], whole["code"])
    assert np.array_equal(r["points"][n0:n0 + n1].view(np.uint64), whole["points"].view(np.uint64))
    assert np.array_equal(r["points"][:n0].view(np.uint64), r["points"][n0 + n1:].view(np.uint64))


def test_pinned_and_ordinary_result_arrays_give_the_same_bits(built_lib):
    s = built_lib.Solver()
    try:
        for _, args in SCENES[:2]:
            sc = scene(args)
            a = _run(s, sc)
            b = _run(s, sc, pinned=True)
            _same_bits(a, b)
            assert a["n_accepted"] == b["n_accepted"]
            # one pinned, one not
            pts = s._pinned(a["points"].shape)
            c = _run(s, sc, points=pts)
            _same_bits(a, c)
    finally:
        s.close()


def test_invalid_calls_write_nothing(built_lib):
    s = built_lib.Solver()
    try:
        sc = scene(dict(n_pairs=3, n_per_pair=[40, 0, 60], seed=7130, stereo=True))
        n = 100

        def refused(mutate):
            sc2 = copy.deepcopy(sc)
            mutate(sc2)
            d, keep = built_lib.tri_desc(sc2["views"], sc2["pairs"], sc2["matches"], sc2["reproj_gate"], sc2["far_threshold"])
            pts = np.full((n, 3), -7.0); code = np.full(n, 99, np.uint8)
            r = built_lib.TriResult()
            r.points = pts.ctypes.data_as(C.POINTER(C.c_double)); r.code = code.ctypes.data_as(C.POINTER(C.c_uint8))
            r.n_accepted = -5; r.status = 99
            rc = s._L.movba_triangulate(s._h, C.byref(d), C.byref(r))
            assert rc == built_lib.ERR_ARG and r.status == built_lib.ERR_ARG and r.n_accepted == -5
            assert (pts == -7.0).all() and (code == 99).all()

        refused(lambda x: x["pairs"]["pair_ptr"].__setitem__(0, 1))
        refused(lambda x: x["pairs"]["pair_ptr"].__setitem__(1, 101))
        refused(lambda x: x["pairs"]["pair_view"].__setitem__((2, 1), 4))
        refused(lambda x: x["pairs"]["pair_view"].__setitem__((0, 0), -1))
        refused(lambda x: x["views"].pop("bf"))
        refused(lambda x: x["views"].pop("b"))
        refused(lambda x: x["matches"].pop("depth1"))
        refused(lambda x: x.__setitem__("reproj_gate", float("nan")))
        refused(lambda x: x.__setitem__("reproj_gate", float("inf")))
        refused(lambda x: x.__setitem__("far_threshold", float("nan")))
        empty = scene(dict(n_pairs=2, n_per_pair=0, seed=1))
        r = _run(s, empty)
        assert r["status"] == 0 and r["n_accepted"] == 0 and len(r["code"]) == 0
        compare_with_ref(_run(s, sc), sc, "after the refused calls")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    w = synth.cfg("cfg2")
    sc = scene(SCENES[2][1])
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")

    def sequence(with_calls):
        s = built_lib.Solver()
        try:
            out = []
            s.upload(w)
            if with_calls:
                compare_with_ref(_run(s, sc), sc, "between upload and run")
            s.run()
            if with_calls:
                _run(s, sc)
            out.append(s.download())
            if with_calls:
                _run(s, sc, pinned=True)
            out.append(s.download())
            assert s._L.movba_lba_reset(s._h) == 0
            s.run()
            out.append(s.download())
            out.append(s.solve(w))
            return out
        finally:
            s.close()

    plain, mixed = sequence(False), sequence(True)
    for a, b in zip(plain, mixed):
        for k in keys:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_accepted_points_are_taken_by_the_local_bundle_adjustment(built_lib):
    """New map points for the newest keyframe of a synthetic window against all the others, triangulated from the window's
    own (noisy) keyframe estimates, appended to the window with their two observations and solved: status 0, and the new
    points' edges are inliers at the window's gate in at least the share the restatement's points reach in the same solve."""
    w = synth.cfg("small")
    NP = w.n_poses
    rng = np.random.default_rng(7140)
    cur = NP - 1
    n_each = 60
    fx, fy, cx, cy = w.cam
    Rt = [(synth.R_from_quat(q[:4]), q[4:]) for q in w.truth_poses]
    obs1, obs2, pv, sizes = [], [], [], []
    for nb in range(NP - 1):
        depth = rng.uniform(5.0, 20.0, n_each); u = rng.uniform(120, 520, n_each); v = rng.uniform(90, 390, n_each)
        Xc = np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], 1)
        Xw = (Xc - Rt[cur][1]) @ Rt[cur][0]
        Y = Xw @ Rt[nb][0].T + Rt[nb][1]
        o2 = np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1)
        obs1.append(np.stack([u, v], 1) + rng.normal(0, 0.5, (n_each, 2))); obs2.append(o2 + rng.normal(0, 0.5, (n_each, 2)))
        pv.append((cur, nb)); sizes.append(n_each)
    sc = dict(views=dict(poses=w.poses, cam=np.tile(np.array(w.cam), (NP, 1))),
              pairs=dict(pair_view=np.array(pv, np.int32), pair_ptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)),
              matches=dict(obs1=synth._f32(np.concatenate(obs1)), obs2=synth._f32(np.concatenate(obs2))),
              reproj_gate=5.0, far_threshold=0.0)
    s = built_lib.Solver()
    try:
        got = _run(s, sc)
        compare_with_ref(got, sc, "new points of the newest keyframe")
        ref = triangulate_ref(sc["views"], sc["pairs"], sc["matches"], 5.0, 0.0)

        def inlier_share(res):
            acc = np.flatnonzero(np.isin(res["code"], ACCEPTED))
            assert len(acc) > 100
            pair = np.repeat(np.arange(NP - 1), sizes)[acc]
            w2 = copy.copy(w)
            w2.points = np.concatenate([w.points, res["points"][acc]])
            new_id = w.n_points + np.arange(len(acc))
            ep = np.stack([sc["pairs"]["pair_view"][pair, 1], sc["pairs"]["pair_view"][pair, 0]], 1).reshape(-1)   # neighbour < current
            el = np.repeat(new_id, 2)
            ob = np.stack([sc["matches"]["obs2"][acc], sc["matches"]["obs1"][acc]], 1).reshape(-1, 2)
            w2.edge_pose = np.concatenate([w.edge_pose, ep.astype(np.int32)]); w2.edge_point = np.concatenate([w.edge_point, el.astype(np.int32)])
            w2.obs = np.concatenate([w.obs, ob]); w2.inv_sigma2 = np.concatenate([w.inv_sigma2, np.ones(len(ep))])
            r = s.solve(w2)
            assert r["status"] == 0
            return float(1.0 - r["outlier"][w.n_edges:].mean()), len(acc)

        share, n_acc = inlier_share(got)
        share_ref, n_ref = inlier_share(ref)
        print(f"{n_acc} accepted points ({n_ref} by the restatement): inlier share of their edges after the solve {share:.4f} (restatement's points {share_ref:.4f})")
        assert n_acc == n_ref and share >= share_ref
    finally:
        s.close()
