"""movba_two_view_lo on the GPU against the numpy restatement of tests/test_two_view_lo_cpu.py (stage 2b restated; tolerances
measured and pairs defined there), against ground truth, against movba_two_view itself (lo_iters = 0 and kept = 0 are that
call bit for bit), and its invariances: batch = solo calls = permuted batch = repeated call with `info` included, pinned =
ordinary result memory, an uploaded window left untouched, lo_iters outside its range refused."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import capi, synth  # noqa: E402

import test_two_view_cpu as T  # noqa: E402
import test_two_view_lo_cpu as L  # noqa: E402
from test_gpu_two_view import pair_of, same_bits  # noqa: E402  (same_bits: every key of test_gpu_two_view.KEYS)

pytestmark = pytest.mark.gpu

LO_KEYS = ("lo_kept", "lo_steps", "loss0", "loss", "n_inliers0", "E0")


def same_bits_lo(a, b):
    return same_bits(a, b) and all(np.array_equal(np.asarray(a[k], np.float64).view(np.uint64), np.asarray(b[k], np.float64).view(np.uint64))
                                   for k in LO_KEYS)


def _batch64():
    """scenes and sizes mixed: pairs under 5 matches, of exactly 5, of one wave and a bit, of several passes of the workgroup"""
    scenes = ("general", "planar", "forward", "rotation")
    return [pair_of(dict(n_matches=[500, 37, 260, 4, 1200, 5][k % 6], inlier_frac=0.6 + 0.05 * (k % 5), noise_px=0.5, seed=8400 + k,
                         scene=scenes[k % 4]), [32, 48, 17][k % 3], 100 + k) for k in range(64)]


@pytest.fixture(scope="module")
def batch(solver):
    """the 64 pairs, movba_two_view's results and movba_two_view_lo's at 0, 4 and 10 steps: computed once, never changed"""
    pairs = _batch64()
    return dict(pairs=pairs, plain=solver.two_view(pairs), lo={k: solver.two_view(pairs, lo_iters=k) for k in (0, 4, L.LO_ITERS)})


def test_results_against_the_restatement_with_the_refit(solver):
    """the committed scenes at 10 steps and the small pairs: E0, E, loss0, loss, kept (where the trace decides it), pose, points,
    parallax within 10 x the measured spread, masks and codes equal off the gates, tie pairs set aside (the scenes under
    TIE_CAP; the pairs of 5 and 6 matches tie by construction); against ground truth no more than 1.5 x the restatement's error"""
    pairs = [pair_of(args, iters, seed) for _, args, iters, seed in L.PAIRS]
    got = solver.two_view(pairs, lo_iters=L.LO_ITERS)
    ties = []
    for g, (label, args, iters, seed) in zip(got, L.PAIRS):
        assert g["status"] == 0
        # (5 and 6 matches: every candidate fits its own sample and the losses tie, so which one wins - and how far it is
        # from the truth - is rounding; those two pairs are held to the invariants)
        if L.compare_lo_with_ref(g, label, args, iters, seed, L.LO_ITERS, check_truth=label not in ("small 5", "small 6"))["tie"]:
            ties.append(label)
    scenes = {s[0] for s in T.SCENES}
    assert len(scenes & set(ties)) <= T.TIE_CAP * len(T.SCENES) and set(ties) - scenes <= {"small 5", "small 6"}, ties
    # what the refit is for: on the general scenes the pose is closer to the truth than movba_two_view's
    plain = solver.two_view(pairs[:4])
    for g, q, p in zip(got[:4], plain, pairs[:4]):
        (gr, gt), (pr, pt) = (T.err_to_truth(dict(R=T.q2R(x["pose"][:4]), t=x["pose"][4:]), p) for x in (g, q))
        print(f"error to truth (rotation, translation direction): {pr:.4g}, {pt:.4g} -> {gr:.4g}, {gt:.4g}")
        assert gr < pr and gt < pt


def test_rotation_scenes_never_initialise_after_the_refit(solver):
    """(test_two_view_lo_cpu.test_rotation_scenes_still_never_initialise_after_the_refit shows the same of the restatement)"""
    pairs = [pair_of(args, iters, seed) for _, args, iters, seed in L.ROTATION]
    for k, g in enumerate(solver.two_view(pairs, lo_iters=L.LO_ITERS)):
        print("rotation", k, "outcome", g["outcome"], "parallax", g["parallax_deg"], "n_pass", g["n_pass"], "of", g["n_inliers"], "kept", g["lo_kept"])
        assert g["status"] == 0 and g["outcome"] in (T.TV_FEW_GOOD, T.TV_LOW_PARALLAX, T.TV_NO_MODEL)


def test_no_steps_is_movba_two_view_bit_for_bit(batch):
    for k, (g, q, p) in enumerate(zip(batch["lo"][0], batch["plain"], batch["pairs"])):
        assert same_bits(g, q), f"pair {k}: lo_iters = 0 differs from movba_two_view"
        assert g["lo_kept"] == 0 and g["lo_steps"] == 0 and g["loss"] == g["loss0"]
        if g["outcome"] == T.TV_NO_MODEL:
            assert g["loss0"] == 0.0 and g["n_inliers0"] == 0 and not g["E0"].any()
        else:
            assert np.array_equal(g["E0"], q["E"]) and g["n_inliers0"] == q["n_inliers"] and g["loss0"] >= 0.0
    assert sum(g["status"] == 3 for g in batch["lo"][0]) == sum(len(p["obs1"]) < 5 for p in batch["pairs"]) > 0
    # for every step count E0 and n_inliers0 are movba_two_view's E and n_inliers (a pair whose kept E has no match within the
    # threshold reports no model and a zeroed info: there is none in this batch)
    for lo_iters, res in batch["lo"].items():
        for k, (g, q) in enumerate(zip(res, batch["plain"])):
            assert g["status"] == q["status"] and g["samples_used"] == q["samples_used"]
            if q["outcome"] != T.TV_NO_MODEL:
                assert np.array_equal(g["E0"].view(np.uint64), q["E"].view(np.uint64)) and g["n_inliers0"] == q["n_inliers"], (lo_iters, k)


def test_invariants_of_the_kept_iterate(batch):
    n_kept = 0
    for lo_iters, res in batch["lo"].items():
        for k, (g, q) in enumerate(zip(res, batch["plain"])):
            assert g["loss"] <= g["loss0"] and 0 <= g["lo_kept"] <= g["lo_steps"] <= lo_iters, (lo_iters, k)
            if g["lo_kept"] == 0:
                assert same_bits(g, q), f"pair {k}, {lo_iters} steps: kept = 0 but the result is not movba_two_view's"
            else:
                n_kept += 1
                assert g["loss"] < g["loss0"] and (g["E"] * g["E0"]).sum() >= 0
                assert np.abs(np.linalg.svd(g["E"])[1] - [1, 1, 0]).max() <= 1e-12
    assert n_kept >= 40
    for k, (a, b, c) in enumerate(zip(batch["lo"][L.LO_ITERS], batch["lo"][4], batch["lo"][0])):
        assert a["loss"] <= b["loss"] <= c["loss"], k
        assert a["loss0"] == b["loss0"] == c["loss0"], k


def test_a_batch_equals_its_solo_calls_and_permutes_with_its_pairs(solver, batch):
    pairs, res = batch["pairs"], batch["lo"][L.LO_ITERS]
    again = solver.two_view(pairs, lo_iters=L.LO_ITERS)
    assert all(same_bits_lo(a, b) for a, b in zip(res, again)), "two calls differ"
    for k, p in enumerate(pairs):
        assert same_bits_lo(res[k], solver.two_view([p], lo_iters=L.LO_ITERS)[0]), f"pair {k} differs between the batch and its solo call"
    perm = np.random.default_rng(3).permutation(64)
    shuffled = solver.two_view([pairs[i] for i in perm], lo_iters=L.LO_ITERS)
    assert all(same_bits_lo(shuffled[j], res[i]) for j, i in enumerate(perm)), "results do not follow a permutation of the pairs"


def test_pinned_and_ordinary_result_memory_give_the_same_bits(solver, batch):
    b = solver.two_view(batch["pairs"][:12], pinned=True, lo_iters=L.LO_ITERS)
    assert all(same_bits_lo(x, y) for x, y in zip(batch["lo"][L.LO_ITERS][:12], b))


def test_an_uploaded_window_solves_to_the_same_bits_after_a_call(built_lib, batch):
    w = synth.cfg("small")
    s = built_lib.Solver()
    try:
        s.upload(w); s.run()
        want = s.download()
        s.upload(w)
        g = s.two_view(batch["pairs"][:8], lo_iters=L.LO_ITERS)
        assert all(same_bits_lo(x, y) for x, y in zip(g, batch["lo"][L.LO_ITERS][:8]))
        s.run()
        got = s.download()
        for k in ("poses", "points", "chi2", "outlier"):
            assert np.array_equal(np.asarray(want[k]).view(np.uint8), np.asarray(got[k]).view(np.uint8)), k
        assert want["n_solves"] == got["n_solves"]
    finally:
        s.close()


def test_step_counts_outside_the_range_are_refused_with_nothing_written(solver, batch):
    p = batch["pairs"][0]
    for lo_iters in (-1, L.MAX_LO_ITERS + 1):
        d, r, keep = capi.two_view_desc(p)
        for key in ("inlier", "good", "code"):
            keep[key][:] = 99
        keep["points"][:] = -7.0
        info = capi.TwoViewLoInfo()
        info.kept, info.loss0 = 55, -3.0
        r.status, r.outcome, r.n_inliers = 77, 88, -5
        assert solver._L.movba_two_view_lo(solver._h, C.byref(d), C.byref(r), 1, lo_iters, C.byref(info)) == capi.ERR_ARG
        assert r.status == capi.ERR_ARG and r.outcome == 88 and r.n_inliers == -5 and info.kept == 55 and info.loss0 == -3.0
        assert all((keep[key] == 99).all() for key in ("inlier", "good", "code")) and (keep["points"] == -7.0).all()
        with pytest.raises(Exception):
            solver.two_view([p], lo_iters=lo_iters)
    assert solver.two_view([], lo_iters=L.LO_ITERS) == [] and solver.two_view([], lo_iters=0) == []
    g = solver.two_view([p], lo_iters=L.MAX_LO_ITERS)[0]
    assert g["status"] == 0 and g["lo_kept"] <= g["lo_steps"] <= L.MAX_LO_ITERS and g["loss"] <= batch["lo"][L.LO_ITERS][0]["loss"]
