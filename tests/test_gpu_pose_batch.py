"""movba_pose_opt_batch on the device: every frame of a batch gets the bits of its solo movba_pose_opt call, whatever else is in
the batch, in which order, and whatever the handle holds besides."""
import threading

import numpy as np
import pytest

from movba import synth

pytestmark = pytest.mark.gpu

GUARD = 1e-6            # (as test_gpu_parity: outlier flags may differ where chi2 sits on the gate)
KEYS = ("pose", "outlier", "chi2", "n_inliers", "ransac_inliers", "ransac_pose", "ransac_samples_used", "lm_iters",
        "lo_accepted", "lo_inliers", "status")


def _frame(n, k, variant):
    f = synth.make_frame(n=n, seed=4100 + 37 * k)
    hub, gate = ((5.0, 25.0), (8.0, 64.0))[k % 2]
    kw = dict(Xw=f["Xw"], obs=f["obs"], pose0=f["pose0"], cam=f["cam"], huber_delta=hub, chi2_gate=gate)
    isg = np.random.default_rng(k).choice([1.0, 1 / 1.44, 1 / 2.0736], size=n)
    if variant == 0:            # LM alone, 4 x 10
        pass
    elif variant == 1:          # LM alone, 1 x 10, level weights
        kw.update(rounds=1, its=10, inv_sigma2=isg)
    elif variant == 2:          # the full pipeline: 50 samples, confidence 0.95, LO 10
        kw.update(ransac_iters=50, ransac_seed=11 + k, confidence=0.95, lo_iters=10)
    elif variant == 3:          # samples without the stopping rule or LO, 1 x 10
        kw.update(ransac_iters=20, ransac_seed=3 + k, rounds=1, its=10)
    else:                       # more samples, the stopping rule without LO, level weights
        kw.update(ransac_iters=80, ransac_seed=97 + k, confidence=0.99, inv_sigma2=isg)
    return kw


def _mixed_frames():
    """25 frames: sizes 4 ... 4 000 matches (the last beyond the LDS staging limit) x five settings, both gates."""
    fr = []
    for a, n in enumerate((4, 50, 500, 1200, 4000)):
        for v in range(5):
            fr.append(_frame(n, 5 * a + v, v))
    return fr


def _assert_same(got, want):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


@pytest.fixture(scope="module")
def mixed(solver):
    fr = _mixed_frames()
    return fr, [solver.pose_opt(**f) for f in fr]


def test_batch_gives_every_frame_its_solo_bits(solver, mixed):
    fr, solo = mixed
    out = solver.pose_opt_batch(fr)
    assert len(out) == len(fr)
    for k, (b, s) in enumerate(zip(out, solo)):
        assert b["status"] == 0, k
        _assert_same(b, s)
    assert any(s["ransac_inliers"] > 0 for s in solo)


def test_batch_lm_frames_match_the_oracle(solver, oracle_mod, mixed):
    """The batch's LM-only 4 x 10 frames (50 ... 4 000 matches, both gates) against the oracle at the tolerances of
    test_pose_optimization_matches_oracle.  The 1 x 10 frames are held to their solo bits only: one round of ten iterations
    stops before the LM has converged, where the oracle's own pose moves by up to 8e-10 when the observations change by one
    part in 1e15, so no device arithmetic can be held to it at 1e-9; 4-match frames are an exactly determined LM."""
    fr, _ = mixed
    out = solver.pose_opt_batch(fr)
    checked = 0
    for f, b in zip(fr, out):
        if f.get("ransac_iters", 0) or len(f["Xw"]) < 50 or f.get("rounds", 4) != 4:
            continue
        o = oracle_mod.pose_opt(f["Xw"], f["obs"], f["pose0"], f["cam"], f["huber_delta"], f["chi2_gate"], f.get("rounds", 4),
                                f.get("its", 10), f.get("inv_sigma2"))
        assert b["n_inliers"] == o["n_inliers"]
        assert np.abs(b["pose"] - o["pose"]).max() < 1e-9
        mism = b["outlier"] != o["outlier"]
        assert (np.abs(o["chi2"][mism] - f["chi2_gate"]) <= GUARD).all()
        np.testing.assert_allclose(b["chi2"], o["chi2"], rtol=1e-7, atol=1e-8)
        checked += 1
    assert checked == 4


def test_per_frame_status_and_invalid_calls(solver, built_lib):
    good = [_frame(500, 1, 2), _frame(50, 2, 0)]
    few = [_frame(n, 10 + n, 0 if n % 2 else 2) for n in (4, 4, 4, 4)]
    for f, n in zip(few, (0, 1, 2, 3)):
        f["Xw"], f["obs"] = f["Xw"][:n], f["obs"][:n]
        if f.get("inv_sigma2") is not None:
            f["inv_sigma2"] = f["inv_sigma2"][:n]
    batch = [few[0], good[0], few[1], few[2], good[1], few[3]]
    out = solver.pose_opt_batch(batch)
    for k in (0, 2, 3, 5):
        assert out[k]["status"] == 3 and out[k]["n_inliers"] == 0
        np.testing.assert_array_equal(out[k]["pose"], batch[k]["pose0"])
    _assert_same(out[1], solver.pose_opt(**good[0]))
    _assert_same(out[4], solver.pose_opt(**good[1]))
    # one invalid descriptor: the whole call is refused, nothing solved
    bad = dict(good[1], rounds=0)
    with pytest.raises(built_lib.MovbaError):
        solver.pose_opt_batch([good[0], bad])
    with pytest.raises(built_lib.MovbaError):
        solver.pose_opt(**bad)
    d0, r0, k0 = built_lib._pose_desc(**good[0])
    d1, r1, k1 = built_lib._pose_desc(**good[1])
    d1.Xw = None
    descs = (built_lib.PoseDesc * 2)(d0, d1)
    res = (built_lib.PoseResult * 2)(r0, r1)
    assert solver._L.movba_pose_opt_batch(solver._h, descs, res, 2) == -1
    assert res[0].status == -1 and res[1].status == -1 and not k0["chi2"].any()
    with pytest.raises(built_lib.MovbaError):
        solver.pose_opt_batch([good[1]] * (1024 + 1))         # MOVBA_MAX_POSE_BATCH + 1
    assert solver.pose_opt_batch([]) == []


def test_order_and_split_do_not_matter(solver, mixed):
    fr, solo = mixed
    perm = np.random.default_rng(5).permutation(len(fr))
    out = solver.pose_opt_batch([fr[k] for k in perm])
    for j, k in enumerate(perm):
        _assert_same(out[j], solo[k])
    half = len(fr) // 2
    a, b = solver.pose_opt_batch(fr[:half]), solver.pose_opt_batch(fr[half:])
    for got, want in zip(a + b, solo):
        _assert_same(got, want)


def test_batch_between_upload_and_run_on_one_handle(solver):
    """The batch uses the handle's pinned staging buffer like movba_pose_opt: between movba_lba_upload and movba_lba_run it
    waits for the window's arrays to have left it; a later download exports the window's results again."""
    w = synth.cfg("cfg3")
    ref = solver.solve(w)
    fr = [_frame(4000, 60 + k, k % 5) for k in range(6)] + [_frame(500, 70 + k, k % 5) for k in range(10)]
    p_ref = [solver.pose_opt(**f) for f in fr]
    assert solver.upload(w) == 0
    out = solver.pose_opt_batch(fr)
    assert solver.run() == 0
    r = solver.download()
    for got, want in zip(out, p_ref):
        _assert_same(got, want)
    for key in ("poses", "points", "outlier", "chi2"):
        np.testing.assert_array_equal(r[key], ref[key])
    solver.pose_opt_batch(fr)
    again = solver.download()
    for key in ("poses", "points", "outlier", "chi2"):
        np.testing.assert_array_equal(again[key], ref[key])


def test_batches_on_one_thread_while_another_solves_a_window(built_lib):
    """Tracking of several sessions batched on one handle while LocalMapping solves on a second handle: both get the bits of
    their solo runs."""
    w = synth.cfg("cfg2")
    fr = [_frame(700, 80 + k, k % 5) for k in range(12)]
    a, b = built_lib.Solver(), built_lib.Solver()
    try:
        ref_lba = a.solve(w)
        ref_pose = [b.pose_opt(**f) for f in fr]
        errs = []

        def mapping():
            try:
                a.prepare(w, pinned=True)
                for _ in range(25):
                    r = a.solve_prepared()
                    if not (np.array_equal(r["poses"], ref_lba["poses"]) and np.array_equal(r["outlier"], ref_lba["outlier"])
                            and np.array_equal(r["chi2"], ref_lba["chi2"])):
                        errs.append("lba result changed")
            except Exception as exc:            # noqa: BLE001
                errs.append(repr(exc))

        def tracking():
            try:
                for _ in range(40):
                    out = b.pose_opt_batch(fr)
                    for got, want in zip(out, ref_pose):
                        if not all(np.array_equal(got[key], want[key]) for key in KEYS):
                            errs.append("pose result changed")
            except Exception as exc:            # noqa: BLE001
                errs.append(repr(exc))

        ts = [threading.Thread(target=mapping), threading.Thread(target=tracking)]
        for t in ts: t.start()
        for t in ts: t.join()
        assert not errs, errs[:3]
    finally:
        a.close(); b.close()


def _side_calls(small):
    """movba_pose_opt, movba_triangulate, movba_two_view, movba_pose_opt_batch and movba_pose_opt again, as functions of a
    Solver.  small: at most 64 matches per frame or pair and 32 hypotheses (each call fits the 1 MiB the pose scratch and the
    staging buffer start with).  Otherwise every call needs more than 1 MiB of both: a frame of 20 000 matches (57 bytes per
    match on the device and in the staging buffer), 5 stereo pairs of 4 000 (64 bytes on the device, 89 in the staging
    buffer), 6 frame pairs of 4 000 with 64 samples (41 bytes per match and 864 per sample on the device, 59 per match in the
    staging buffer), 6 frames of 4 000 and one that is staged in LDS."""
    n = 60 if small else 20000
    first = dict(_frame(n, 200, 0), ransac_iters=20 if small else 32, ransac_seed=5, confidence=0.95, lo_iters=10)
    last = _frame(n, 201, 1)            # (LM alone: staged in LDS when small, no device copy at all)
    tri = synth.make_triangulation(2, 30, seed=71, stereo=True) if small else synth.make_triangulation(5, 4000, seed=72, stereo=True)
    tv = [dict(synth.make_two_view(60 if small else 4000, seed=300 + k, scene=synth.TWO_VIEW_SCENES[k % 4]),
               ransac_iters=32 if small else 64, ransac_seed=1 + k) for k in range(2 if small else 6)]
    if small:
        batch = [_frame(50, 210 + k, v) for k, v in enumerate((0, 1, 3))]
    else:
        batch = [_frame(4000, 220 + k, k % 5) for k in range(6)] + [_frame(500, 230, 2)]
    return [lambda s: s.pose_opt(**first),
            lambda s: s.triangulate(tri["views"], tri["pairs"], tri["matches"], tri["reproj_gate"], tri["far_threshold"]),
            lambda s: s.two_view(tv),
            lambda s: s.pose_opt_batch(batch),
            lambda s: s.pose_opt(**last)]


def _assert_same_bits(got, want, where):
    if isinstance(want, list):
        assert len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_same_bits(g, w, f"{where}[{k}]")
        return
    assert got.keys() == want.keys(), where
    for key in want:
        g, w = np.atleast_1d(got[key]), np.atleast_1d(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (where, key)
        # (raw bytes: rejected matches carry NaN points)
        assert np.array_equal(np.ascontiguousarray(g).reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)), (where, key)


def test_side_calls_interleaved_on_one_handle_give_a_fresh_handles_bits(built_lib):
    """The four entry points that share the handle's pose scratch and staging buffer, one after the other on ONE handle: a
    round of small calls, then a round in which every call needs more of both buffers than the first round left behind, so
    the buffers are reallocated while they hold the other entry points' stale contents.  Every result array of every call is,
    bit for bit, that of the same call on a fresh handle that has done nothing else."""
    calls = _side_calls(True) + _side_calls(False)
    want = []
    for call in calls:
        fresh = built_lib.Solver()
        try:
            want.append(call(fresh))
        finally:
            fresh.close()
    one = built_lib.Solver()
    try:
        got = [call(one) for call in calls]
    finally:
        one.close()
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same_bits(g, w, f"call {k}")
