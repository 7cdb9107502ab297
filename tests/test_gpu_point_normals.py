"""movba_point_normals and movba_lba_point_normals on the device against the restatement of tests/point_normals_ref.py: the
parity call value by value, the exact case to the bit, independence of a point from everything but its own list (bit-identical
alone, in reverse order, split over calls, twice, into pinned memory), the resident variant against the array variant fed the
downloaded estimate and the caller-order lists - after a solve of a monocular, a shuffled and a stereo window and after a
batched run, without flags, with the downloaded ones and with flags that empty points - its MOVBA_ERR_STATE, a window left as it
was, and the chain init_map -> point_normals -> view_points that the call closes."""
import copy

import numpy as np
import pytest

import point_normals_ref as N
import test_init_map_cpu as M
import view_points_ref as V
from movba import capi, synth

pytestmark = pytest.mark.gpu


def _same_call_bits(a, b, label=""):
    for key in N.KEYS:
        assert N.same_bits(a[key], b[key]), (label, key)


def test_parity_with_the_restatement(solver):
    """300 views at general-position poses with |t| <= 10, 1000 points at least 0.5 from every centre, lists of 0, 1, 2, 63, 64,
    65, 255, 256, 257 and 300 observers, ref_level over 0 .. 7: values within 1e-12 relative to max(1, |value|) - the bound
    test_gpu_view_points.py uses for the same pose -> centre -> norm chain with contraction free to differ; a 300-term sum of
    numbers of magnitude at most 1 adds at most about 300 x 300 x 1.1e-16 = 1e-11 absolute before the division by n, 3e-14 to the
    normal - no item dropped, NaN in both for the empty lists."""
    got = solver.point_normals(**N.parity_case())
    assert got["status"] == 0
    N.compare(got, N.parity_ref(), "parity")


@pytest.mark.parametrize("table", ["1.2", "pow2", "one-level"])
def test_exact_case_to_the_bit(solver, table):
    """Identity rotations, integer translations, integer points whose differences to the centres are 3-D Pythagorean triples,
    tables of 1.2^k, of powers of two and of a single level: every intermediate is exact or one correctly rounded IEEE operation,
    so the device equals numpy bit for bit - which pins the division (not a reciprocal) and the sequential order.  Point 5 lies in
    an observer's centre that is also its reference (NaN normal, distances 0), point 6 in an observer's centre with another
    reference.  (A NaN equals any NaN: IEEE 754 leaves the sign of a generated NaN open.)"""
    case = N.exact_case(dict([("1.2", N.SCALE_12), ("pow2", N.SCALE_POW2), ("one-level", np.array([2.0]))])[table])
    got, ref = solver.point_normals(**case), N.ref_point_normals(**case)
    for key in N.KEYS:
        print(key, "differing entries", int((~(np.isnan(got[key]) & np.isnan(ref[key])) & (got[key] != ref[key])).sum()))
    _same_call_bits(got, ref, table)
    assert np.isnan(got["normals"][[5, 6]]).all() and got["max_distance"][5] == 0.0 and got["min_distance"][5] == 0.0


def test_a_point_depends_on_its_own_list_alone(built_lib):
    case = N.parity_case()
    n = len(case["points"])
    s = built_lib.Solver()
    try:
        whole = s.point_normals(**case)
        _same_call_bits(s.point_normals(**case), whole, "two calls")
        _same_call_bits(s.point_normals(**case, pinned=True), whole, "pinned")
        rev = s.point_normals(**N.subset(case, range(n - 1, -1, -1)))
        for key in N.KEYS:
            assert N.same_bits(rev[key][::-1], whole[key]), ("reversed point order", key)
        a, b = s.point_normals(**N.subset(case, range(0, 377))), s.point_normals(**N.subset(case, range(377, n)))
        for key in N.KEYS:
            assert N.same_bits(np.concatenate([a[key], b[key]]), whole[key]), ("split over two calls", key)
        # alone, one point per call: one of every list length and both kinds of empty list
        for p in list(range(20)) + [n - 1]:
            alone = s.point_normals(**N.subset(case, [p]))
            for key in N.KEYS:
                assert N.same_bits(alone[key], whole[key][p:p + 1]), ("alone", p, key)
        # a reversed list is another order of the same sum: rounding only
        flipped = s.point_normals(**dict(case, lists=[l[::-1] for l in case["lists"]]))
        ok = ~np.isnan(whole["normals"])
        diff = float(np.abs(flipped["normals"][ok] - whole["normals"][ok]).max())
        print("reversed lists: largest change of a normal", diff)
        assert np.array_equal(np.isnan(flipped["normals"]), ~ok) and diff <= 1e-13
        assert N.same_bits(flipped["max_distance"], whole["max_distance"]) and N.same_bits(flipped["min_distance"], whole["min_distance"])
    finally:
        s.close()


def _shuffled(w, seed=3):
    """the same window with its edges in another caller order: no longer grouped by point"""
    pm = np.random.default_rng(seed).permutation(w.n_edges)
    w2 = copy.copy(w)
    w2.edge_pose, w2.edge_point, w2.obs, w2.inv_sigma2 = w.edge_pose[pm], w.edge_point[pm], w.obs[pm], w.inv_sigma2[pm]
    if getattr(w, "obs_right", None) is not None:
        w2.obs_right = w.obs_right[pm]
    return w2


def _emptying_mask(w, seed=8):
    """flags that take every edge of every fourth map point and a fifth of the others"""
    rng = np.random.default_rng(seed)
    return ((w.edge_point % 4 == 0) | (rng.random(w.n_edges) < 0.2)).astype(np.uint8)


def _check_resident(s, w, res, label):
    """lba_point_normals on the solved window of s against point_normals fed the download `res`, three masks"""
    ref_pose, ref_level = N.window_refs(w)
    some_empty = False
    for name, mask in (("no flags", None), ("downloaded flags", res["outlier"]), ("emptying flags", _emptying_mask(w))):
        got = s.lba_point_normals(ref_pose, ref_level, N.SCALE_12, outlier=mask)
        lists = N.window_lists(w, mask)
        want = s.point_normals(res["points"], res["poses"], lists, ref_pose, ref_level, N.SCALE_12)
        assert got["status"] == 0 and want["status"] == 0
        _same_call_bits(got, want, (label, name))
        empty = np.array([len(l) == 0 for l in lists])
        assert np.array_equal(np.isnan(got["max_distance"]), empty), (label, name)
        some_empty = some_empty or bool(empty.any())
        N.compare(got, N.ref_point_normals(res["points"], res["poses"], lists, ref_pose, ref_level, N.SCALE_12), f"{label}, {name}")
        _same_call_bits(s.lba_point_normals(ref_pose, ref_level, N.SCALE_12, outlier=mask, pinned=True), got, (label, name, "pinned"))
    assert some_empty


def _windows():
    small = synth.cfg("small")
    return dict(small=small, shuffled=_shuffled(small), stereo=synth.make_window(6, 2, 150, seed=43, run_lo=2, run_hi=5, stereo_frac=0.7))


@pytest.mark.parametrize("name", ["small", "shuffled", "stereo"])
def test_resident_variant_equals_the_array_variant(built_lib, name):
    w = _windows()[name]
    s = built_lib.Solver()
    try:
        ref_pose, ref_level = N.window_refs(w)
        with pytest.raises(capi.MovbaError, match="call order"):             # nothing uploaded
            s._keep = capi.make_desc(w)
            s.lba_point_normals(ref_pose, ref_level, N.SCALE_12)
        s.upload(w)
        with pytest.raises(capi.MovbaError, match="call order"):             # uploaded, not run
            s.lba_point_normals(ref_pose, ref_level, N.SCALE_12)
        s.run()
        res = s.download()
        assert res["status"] == 0
        _check_resident(s, w, res, name)
        # the refusals that need a window
        for bad in (dict(ref_pose=np.where(np.arange(w.n_points) == 7, w.n_poses, ref_pose)), dict(ref_pose=np.where(np.arange(w.n_points) == 0, -1, ref_pose)),
                    dict(ref_level=np.where(np.arange(w.n_points) == 3, 8, ref_level)), dict(scale_factors=N.SCALE_12[:7]),
                    dict(scale_factors=np.where(np.arange(8) == 2, 0.0, N.SCALE_12))):
            args = dict(dict(ref_pose=ref_pose, ref_level=ref_level, scale_factors=N.SCALE_12), **bad)
            with pytest.raises(capi.MovbaError, match="argument"):
                s.lba_point_normals(**args)
        again = s.download()
        for k in ("poses", "points", "chi2", "outlier"):
            assert np.array_equal(again[k], res[k]), k
    finally:
        s.close()


def test_resident_variant_after_a_batched_run(built_lib):
    import torch
    ws = [synth.cfg("small"), synth.cfg("small", seed=12)]
    st = torch.cuda.Stream(device=0)            # (the handles of a batch share one stream)
    solvers = [built_lib.Solver(device=0, stream=st.cuda_stream) for _ in ws]
    try:
        for s, w in zip(solvers, ws):
            s.upload(w)
        capi.run_batch(solvers)
        for k, (s, w) in enumerate(zip(solvers, ws)):
            res = s.download()
            assert res["status"] == 0
            _check_resident(s, w, res, f"batch window {k}")
    finally:
        for s in solvers:
            s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """The sequence of test_gpu_view_points.py's test of the same name, with both calls in the places of movba_view_points:
    download, marginals, reset + run and a fresh upload + run give the bits they give without the calls."""
    w = synth.cfg("small")
    case = N.parity_case()
    ref_pose, ref_level = N.window_refs(w)
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")

    def sequence(with_calls):
        s = built_lib.Solver()
        try:
            out = []
            out.append(s.solve(w))
            before = s.marginals()
            if with_calls:
                first = s.lba_point_normals(ref_pose, ref_level, N.SCALE_12, outlier=out[0]["outlier"])
                N.compare(s.point_normals(**case), N.parity_ref(), "after the solve")
                _same_call_bits(s.lba_point_normals(ref_pose, ref_level, N.SCALE_12, outlier=out[0]["outlier"]), first, "around the array call")
            out.append(s.download())
            after = s.marginals()
            assert after["status"] == before["status"]
            assert V.same_bits(after["pose_cov"], before["pose_cov"]) and V.same_bits(after["point_cov"], before["point_cov"])
            if with_calls:
                s.lba_point_normals(ref_pose, ref_level, N.SCALE_12, pinned=True)
                s.point_normals(**case, pinned=True)
            assert s._L.movba_lba_reset(s._h) == 0
            if with_calls:
                with pytest.raises(capi.MovbaError, match="call order"):
                    s.lba_point_normals(ref_pose, ref_level, N.SCALE_12)
            s.run()
            out.append(s.download())
            if with_calls:
                _same_call_bits(s.lba_point_normals(ref_pose, ref_level, N.SCALE_12, outlier=out[0]["outlier"]), first, "after reset + run")
            s.upload(w)
            if with_calls:
                N.compare(s.point_normals(**case), N.parity_ref(), "between upload and run")
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
    for k in keys:
        assert np.array_equal(np.asarray(mixed[2][k]), np.asarray(mixed[0][k])), k


def test_the_hole_between_init_map_and_view_points_is_closed(built_lib):
    """movba_init_map on a committed two-view scene (255 matches, general), movba_point_normals over its map with both
    keyframes as observers and keyframe 1 as the reference, movba_view_points FRUSTUM from keyframe 1 with cos_limit 0.5 and
    bounds that cover the observations: every used point is MOVBA_VP_VISIBLE.  Its predicted level is ref_level or ref_level + 1
    (clamped): seen from its own reference keyframe max_distance / dist is scale_factors[ref_level] up to rounding, which puts
    PredictScale's ceil exactly on its boundary - the set is asserted, not one value."""
    k = next(i for i, sp in enumerate(M._SPECS) if sp["n_used"] == 255)
    pair = M.PAIRS()[k]
    s = built_lib.Solver()
    try:
        im = s.init_map([{key: v for key, v in pair.items() if not key.startswith("truth") and key != "spec"}])[0]
        assert im["status"] == 0 and im["outcome"] == capi.IM_OK
        use = M.used(pair)
        X = im["points"][use]
        n = len(X)
        poses = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], im["pose"]])
        ref_level = (np.arange(n) % N.N_LEVELS).astype(np.int32)
        nrm = s.point_normals(X, poses, [[0, 1]] * n, np.zeros(n, np.int32), ref_level, N.SCALE_12)
        assert nrm["status"] == 0 and not np.isnan(nrm["normals"]).any()
        obs = np.asarray(pair["obs1"], np.float64)[use]
        bounds = (obs[:, 0].min() - 1.0, obs[:, 0].max() + 1.0, obs[:, 1].min() - 1.0, obs[:, 1].max() + 1.0)
        view = dict(mode=capi.VIEW_FRUSTUM, pose=poses[0], cam=tuple(pair["cam"]), bounds=bounds, cos_limit=0.5, n_levels=N.N_LEVELS,
                    log_scale_factor=float(np.log(1.2)), items=np.arange(n, dtype=np.int32))
        vp = s.view_points(dict(points=X, normals=nrm["normals"], max_distance=nrm["max_distance"], min_distance=nrm["min_distance"]), [view])
        codes, counts = np.unique(vp["code"], return_counts=True)
        print(dict(zip(codes.tolist(), counts.tolist())), "levels above ref_level:", int((vp["level"] != ref_level).sum()))
        assert (vp["code"] == capi.VP_VISIBLE).all() and vp["n_accepted"][0] == n
        assert ((vp["level"] == ref_level) | (vp["level"] == np.minimum(ref_level + 1, N.N_LEVELS - 1))).all()
        assert (vp["view_cos"] >= 0.5).all()
    finally:
        s.close()
