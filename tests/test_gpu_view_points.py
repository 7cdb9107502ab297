"""movba_view_points on the device against the numpy restatement of tests/view_points_ref.py: the nine-view parity call decision
by decision and value by value, items placed exactly on every gate, the radix select's median to the bit on lists of every
awkward size and content, independence of a view from everything but its own list (bit-identical alone, in reverse order, twice,
into pinned memory, without the optional arrays), a window on the same handle left as it was, and the baseline test in front
of movba_triangulate taken from this call's medians."""
import numpy as np
import pytest

import view_points_ref as V
from movba import synth

pytestmark = pytest.mark.gpu

ITEM_KEYS = ("code", "z", "uv", "dist", "view_cos", "level", "ur", "track_depth")


def _same_call_bits(a, b, label=""):
    for key in ITEM_KEYS + ("n_accepted", "median_depth"):
        if key in a and key in b:
            assert V.same_bits(a[key], b[key]), (label, key)


def test_parity_with_the_restatement(solver):
    """Nine views - three of each mode, lists of 0, 1, 63, 64, 65, 255, 256, 257 and 1000 - over 1200 shared points around
    general-position poses: codes and levels equal on every item the restatement keeps (none is dropped for the committed
    seed; the cap is 1 %), values within 1e-12 relative to max(1, |value|) - some twenty fp64 operations on inputs with |z| >=
    0.1, contraction allowed to differ - counts exact."""
    points, views = V.parity_case()
    ref = V.parity_ref()
    assert int(ref["near"].sum()) == 0
    got = solver.view_points(points, views)
    V.compare(got, ref, "parity")
    assert np.array_equal(got["n_accepted"], ref["n_accepted"])


def test_gates_decide_as_written(solver):
    """Identity pose, fx = fy = 1, integer-valued coordinates: every quantity is exact, and the items sit exactly on the gates.
    u == maxX is accepted in FRUSTUM and rejected in FUSE, u == minX accepted in both; z == 0, dist == 0.8 min, dist == 1.2 max
    and viewCos == cos_limit decide as the comparisons say; a ratio on a level boundary clamps at 0 and at n_levels - 1; NaN
    in a point or a normal is carried through as the comparisons carry it."""
    points, views, labels, want = V.gate_case()
    got = solver.view_points(points, views)
    ref = V.ref_view_points(points, views)
    n = len(labels)
    for i, label in enumerate(labels):
        frustum, fuse, level = want[label]
        print(label, got["code"][i], got["code"][n + i], got["level"][i])
        assert got["code"][i] == frustum and got["code"][n + i] == fuse, label
        if level is not None:
            assert got["level"][i] == level, label
    assert np.array_equal(got["code"], ref["code"]) and np.array_equal(got["level"], ref["level"])
    assert np.array_equal(got["n_accepted"], ref["n_accepted"])
    for key in V.VALUE_KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), key


def test_median_is_the_exact_order_statistic(solver):
    """DEPTH views of 1, 2, 3, 255, 256, 257 and 4097 items with q of 1, 2 and 3, lists of all-equal depths, duplicates across
    the wanted rank, mixed signs, +-0, +-inf and NaN, an empty list (-1.0), and one list of 40 000 items - above the limit of
    the calls that count ranks - in one call: median_depth to the bit."""
    points, views, lists = V.median_case()
    assert max(len(z) for z in lists) == 40000
    got = solver.view_points(points, views, arrays=("z",))
    ref = V.ref_view_points(points, views)
    assert V.same_bits(got["z"], ref["z"])
    for k, z in enumerate(lists):
        assert V.same_bits(got["median_depth"][k:k + 1], ref["median_depth"][k:k + 1]), (k, len(z), views[k]["q"], got["median_depth"][k], ref["median_depth"][k])
    assert np.array_equal(got["n_accepted"], [len(z) for z in lists]) and (got["code"] == V.DEPTH_ITEM).all()
    empty = [k for k, z in enumerate(lists) if len(z) == 0]
    assert empty and (got["median_depth"][empty] == -1.0).all()


def test_a_view_depends_on_its_own_list_alone(built_lib):
    points, views = V.parity_case()
    s = built_lib.Solver()
    try:
        whole = s.view_points(points, views)
        ptr = whole["view_ptr"]
        _same_call_bits(s.view_points(points, views), whole, "two calls")
        for k, v in enumerate(views):
            alone = s.view_points(points, [v])
            seg = slice(ptr[k], ptr[k + 1])
            for key in ITEM_KEYS:
                assert V.same_bits(alone[key], whole[key][seg]), (k, key)
            assert alone["n_accepted"][0] == whole["n_accepted"][k] and V.same_bits(alone["median_depth"], whole["median_depth"][k:k + 1]), k
        rev = s.view_points(points, views[::-1])
        rptr = rev["view_ptr"]
        for k in range(len(views)):
            j = len(views) - 1 - k
            for key in ITEM_KEYS:
                assert V.same_bits(rev[key][rptr[j]:rptr[j + 1]], whole[key][ptr[k]:ptr[k + 1]]), (k, key)
        assert V.same_bits(rev["n_accepted"][::-1], whole["n_accepted"]) and V.same_bits(rev["median_depth"][::-1], whole["median_depth"])
        # a list split over two views: the items keep their bits
        big = max(range(len(views)), key=lambda k: len(views[k]["items"]))
        a, b = dict(views[big]), dict(views[big])
        a["items"], b["items"] = views[big]["items"][:377], views[big]["items"][377:]
        split = s.view_points(points, [a, b])
        for key in ITEM_KEYS:
            assert V.same_bits(split[key], whole[key][ptr[big]:ptr[big + 1]]), key
        assert split["n_accepted"].sum() == whole["n_accepted"][big]
        _same_call_bits(s.view_points(points, views, pinned=True), whole, "pinned")
        few = s.view_points(points, views, arrays=("uv", "level"))
        assert "z" not in few
        _same_call_bits(few, whole, "optional arrays left out")
        none = s.view_points(points, views, arrays=())
        _same_call_bits(none, whole, "every optional array left out")
        _same_call_bits(s.view_points(points, views, pinned=True, arrays=("dist",)), whole, "pinned, one optional array")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    w = synth.cfg("small")
    points, views = V.parity_case()
    ref = V.parity_ref()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")

    def sequence(with_calls):
        s = built_lib.Solver()
        try:
            out = []
            out.append(s.solve(w))
            before = s.marginals()
            if with_calls:
                V.compare(s.view_points(points, views), ref, "after the solve")
            out.append(s.download())
            after = s.marginals()
            assert after["status"] == before["status"]
            assert V.same_bits(after["pose_cov"], before["pose_cov"]) and V.same_bits(after["point_cov"], before["point_cov"])
            if with_calls:
                s.view_points(points, views, pinned=True)
            assert s._L.movba_lba_reset(s._h) == 0
            s.run()
            out.append(s.download())
            s.upload(w)
            if with_calls:
                V.compare(s.view_points(points, views), ref, "between upload and run")
            s.run()
            out.append(s.download())
            return out, before
        finally:
            s.close()

    (plain, cov0), (mixed, cov1) = sequence(False), sequence(True)
    assert V.same_bits(cov0["pose_cov"], cov1["pose_cov"]) and V.same_bits(cov0["point_cov"], cov1["point_cov"])
    for a, b in zip(plain, mixed):
        for k in keys:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # the run after the reset is the solo result
    for k in keys:
        assert np.array_equal(np.asarray(mixed[2][k]), np.asarray(mixed[0][k])), k


def test_baseline_test_in_front_of_triangulate(built_lib):
    """A keyframe and five neighbours (synth.make_triangulation): every neighbour's map points are those of its pair, for two
    of them ten times as far away.  baseline / median_depth from this call selects the neighbours that LocalMapping.cc:268-287,
    restated in numpy, selects - not all and not none - and movba_triangulate on the selected pairs gives what it gives for
    them in the call over all pairs."""
    sc = synth.make_triangulation(5, 200, 7301, mismatch_frac=0.0, special_frac=0.0)
    poses, cam = sc["views"]["poses"], sc["views"]["cam"]
    ptr = sc["pairs"]["pair_ptr"]
    X = sc["truth"].copy()
    for p in (1, 3):
        X[ptr[p]:ptr[p + 1]] *= 10.0 + 30.0 * p
    views = [dict(mode=V.DEPTH, pose=poses[p + 1], cam=cam[p + 1], q=2, items=np.arange(ptr[p], ptr[p + 1], dtype=np.int32)) for p in range(5)]
    s = built_lib.Solver()
    try:
        got = s.view_points(dict(points=X), views)
        centres = np.array([-(V.rotation(q).T @ q[4:]) for q in poses])
        baseline = np.linalg.norm(centres[1:] - centres[0], axis=1)
        ratio = baseline / got["median_depth"]
        # LocalMapping.cc:268-287, monocular: ComputeSceneMedianDepth(2), ratioBaselineDepth < 0.01 skips the neighbour
        med = np.array([np.sort(X[ptr[p]:ptr[p + 1]] @ V.rotation(poses[p + 1])[2] + poses[p + 1][6])[(200 - 1) // 2] for p in range(5)])
        want = ~(baseline / med < 0.01)
        print("baseline / median depth", ratio, "selected", want)
        assert np.array_equal(~(ratio < 0.01), want) and 0 < want.sum() < 5
        np.testing.assert_allclose(got["median_depth"], med, rtol=1e-12)
        whole = s.triangulate(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
        sel = np.flatnonzero(want)
        idx = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in sel])
        sub = s.triangulate(sc["views"], dict(pair_view=sc["pairs"]["pair_view"][sel], pair_ptr=np.arange(len(sel) + 1, dtype=np.int32) * 200),
                            {k: v[idx] for k, v in sc["matches"].items()}, sc["reproj_gate"], sc["far_threshold"])
        assert sub["status"] == 0 and np.array_equal(sub["code"], whole["code"][idx]) and V.same_bits(sub["points"], whole["points"][idx])
        assert sub["n_accepted"] > 0
    finally:
        s.close()
