"""movba_two_view on the GPU against the numpy restatement of tests/test_two_view_cpu.py (tolerances, caps and committed
scenes are defined and justified there), against ground truth, and its invariances: batch = solo calls, permutation, repetition,
pinned = ordinary result memory, and an uploaded window left untouched."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

import test_two_view_cpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("status", "outcome", "pose", "E", "parallax_deg", "n_inliers", "n_pass", "n_good", "samples_used", "inlier", "points", "good", "code")


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else np.float64(a[k]).view(np.uint64),
                              np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else np.float64(b[k]).view(np.uint64))
               for k in KEYS)


def pair_of(args, iters, seed):
    p = synth.make_two_view(**args)
    p.update(ransac_iters=iters, ransac_seed=seed)
    return p


def test_hypotheses_and_results_against_the_restatement(solver):
    """per sample: hyp_nsol / hyp_E / hyp_loss within 10 x the measured spread, cap (i); per pair: outcome, winner, pose,
    parallax, points within tolerance, masks and codes equal off the gates (cap (ii)), counts consistent with the masks; tie
    pairs under cap (iii); against ground truth: no more than 1.5 x the restatement's own error"""
    pairs = [pair_of(args, iters, seed) for _, args, iters, seed in T.SCENES]
    got = solver.two_view(pairs, diagnostics=True)
    n_tie = 0
    for g, p, (label, args, iters, seed) in zip(got, pairs, T.SCENES):
        assert g["status"] == 0
        n_tie += T.compare_with_ref(g, p, iters, seed, label, check_truth=True)["tie"]
    assert n_tie <= T.TIE_CAP * len(pairs)


def test_rotation_scenes_never_initialise(solver):
    pairs = [pair_of(dict(n_matches=400, inlier_frac=0.8, noise_px=0.5, seed=8300 + k, scene="rotation"), 64, 5 + k) for k in range(6)]
    for k, g in enumerate(solver.two_view(pairs)):
        print("rotation", k, "outcome", g["outcome"], "parallax", g["parallax_deg"], "n_pass", g["n_pass"], "of", g["n_inliers"])
        assert g["status"] == 0 and g["outcome"] in (T.TV_FEW_GOOD, T.TV_LOW_PARALLAX, T.TV_NO_MODEL)


def _batch64():
    scenes = ("general", "planar", "forward", "rotation")
    return [pair_of(dict(n_matches=[500, 37, 260, 4, 1200, 5][k % 6], inlier_frac=0.6 + 0.05 * (k % 5), noise_px=0.5, seed=8400 + k,
                         scene=scenes[k % 4]), [32, 48, 17][k % 3], 100 + k) for k in range(64)]


def test_a_batch_equals_its_solo_calls_and_permutes_with_its_pairs(solver):
    pairs = _batch64()
    batch = solver.two_view(pairs)
    again = solver.two_view(pairs)
    assert all(same_bits(a, b) for a, b in zip(batch, again)), "two calls differ"
    outcomes = [g["outcome"] for g in batch]
    print("outcomes of the 64 pairs:", {o: outcomes.count(o) for o in set(outcomes)}, "empty:", sum(g["status"] == 3 for g in batch))
    assert sum(g["status"] == 3 for g in batch) == sum(len(p["obs1"]) < 5 for p in pairs) > 0
    assert outcomes.count(T.TV_OK) >= 20
    for k, p in enumerate(pairs):
        solo = solver.two_view([p])[0]
        assert same_bits(batch[k], solo), f"pair {k} differs between the batch and its solo call"
    perm = np.random.default_rng(3).permutation(64)
    shuffled = solver.two_view([pairs[i] for i in perm])
    assert all(same_bits(shuffled[j], batch[i]) for j, i in enumerate(perm)), "results do not follow a permutation of the pairs"


def test_pinned_and_ordinary_result_memory_give_the_same_bits(solver):
    pairs = _batch64()[:12]
    a = solver.two_view(pairs, diagnostics=True)
    b = solver.two_view(pairs, pinned=True, diagnostics=True)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    for x, y in zip(a, b):
        for k in ("hyp_nsol", "hyp_E", "hyp_loss"):
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8))


def test_placement_mixed_per_pair_and_per_array_gives_the_same_bits(solver):
    """pair 0: points and code pinned, inlier and good ordinary; pair 1 (12 matches) the other way round; pair 2 (4 matches:
    not solved) all ordinary - every result field and array as with everything in ordinary memory"""
    pairs = [pair_of(args, iters, seed) for _, args, iters, seed in T.SCENES[:3]]
    for p, m in ((pairs[1], 12), (pairs[2], 4)):
        p["obs1"], p["obs2"] = p["obs1"][:m], p["obs2"][:m]
    want = solver.two_view(pairs)
    got = solver.two_view(pairs, pinned=[{"points", "code"}, {"inlier", "good"}, set()])
    assert [g["status"] for g in want] == [0, 0, 3] and [len(g["code"]) for g in want] == [500, 12, 4]
    for k, (a, b) in enumerate(zip(want, got)):
        assert same_bits(a, b), f"pair {k} differs between mixed and ordinary result memory"


def test_an_uploaded_window_solves_to_the_same_bits_after_a_call(built_lib):
    w = synth.cfg("small")
    s = built_lib.Solver()
    try:
        s.upload(w); s.run()
        want = s.download()
        s.upload(w)
        g = s.two_view(_batch64()[:8])
        assert g[0]["status"] == 0
        s.run()
        got = s.download()
        for k in ("poses", "points", "chi2", "outlier"):
            assert np.array_equal(np.asarray(want[k]).view(np.uint8), np.asarray(got[k]).view(np.uint8)), k
        assert want["n_solves"] == got["n_solves"]
    finally:
        s.close()


def test_invalid_descriptors_are_refused_on_the_device_build(solver):
    p = _batch64()[0]
    for key, val in (("ransac_iters", 0), ("ransac_iters", 1025), ("threshold", 0.0), ("max_depth", float("nan")), ("cam", (0.0, 450.0, 320.0, 240.0))):
        with pytest.raises(Exception):
            solver.two_view([dict(p, **{key: val})])
    assert solver.two_view([]) == []
