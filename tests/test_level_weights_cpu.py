"""Windows whose edges carry the reference's pyramid-level weights (inv_sigma2 = mvInvLevelSigma2[octave], src/Optimizer.cc:657-658,
685-687, 724-725; synth.with_levels), and what tests/test_gpu_level_weights.py rests on (no GPU).

Every generator of movba.synth ends in inv_sigma2 = ones, and an array of ones is the same under any permutation, stale copy or
mix-up between windows.  The windows below are the ones the GPU file solves against the oracle; here the oracle alone shows

  teeth       a weight array that is wrong by ONE swapped pair of adjacent edges, or shifted by one edge, moves the poses by at
              least 100 x ROT_TOL or 100 x TRANS_TOL: a kernel or an upload route that reads a neighbour's weight cannot pass
              check_against;
  clean side  the oracle's own spread under the edge orders the reference produces (order_noise.spread, as
              test_order_noise_cpu.py uses it) stays below a tenth of ROT_TOL, TRANS_TOL and POINT_TOL, its decisions do not
              depend on the order and no chi2 lies within GUARD of the gate: check_against's defaults hold on these windows,
              without noise_guard.

The level seeds are conditions on the inputs: a seed is taken when the oracle alone meets both sides."""
import copy

import numpy as np
import pytest

import order_noise
import point_normals_ref
from conftest import load_golden, quat_angle
from movba import synth
from order_noise import GUARD, MODULE_TOL, spread

ROT_TOL, TRANS_TOL, POINT_TOL = MODULE_TOL["rot"], MODULE_TOL["trans"], MODULE_TOL["point"]
TEETH = 100

TABLE = [1, 0.69444442, 0.48225307, 0.33489791, 0.23256798, 0.16150554, 0.11215661, 0.07788653]


def _batch_shape():
    return synth.make_window(16, 2, 600, seed=71, run_lo=2, run_hi=7)


def _max_iters(w, n):
    w.max_iters = n
    return w


# name -> (the window with unit weights, level seed, further arguments of the solve)
WINDOWS = {
    "small": (lambda: synth.cfg("small"), 1, {}),
    "small-2": (lambda: synth.cfg("small"), 2, {}),
    "stereo": (lambda: synth.make_window(12, 3, 1500, seed=57, run_lo=2, run_hi=7, stereo_frac=0.5), 1, {}),
    "cameras": (lambda: synth.mixed_cameras(synth.cfg("small"), seed=44), 1, {}),
    # the first size beyond the on-chip PCG
    "81kf": (lambda: _max_iters(synth.make_window(81, 4, 1500, 9, run_lo=2, run_hi=8), 3), 1, {}),
    # 18 to 26 observers per point: k_point's loop behind the two prefetched edges
    "long-tracks": (lambda: synth.make_window(24, 4, 300, seed=5, run_lo=18, run_hi=26), 1, {}),
    # test_more_keyframes_than_the_point_kernels_stage_in_lds's window; two iterations: after four the oracle's own spread under
    # edge permutation is 2e-9 ... 3e-9 m in translation with unit weights and with levels alike, after two it is 1e-11 m
    "beyond-lds": (lambda: _max_iters(synth.make_window(12, 900, 3000, seed=21, run_lo=2, run_hi=6), 2), 1, {}),
    "cfg2": (lambda: synth.cfg("cfg2"), 1, {}),
    # lba_hard's inputs: with these levels and two trials per iteration the solve ends on a rejected trial
    "hard": (lambda: load_golden("lba_hard")[0], 44, dict(max_trials=2)),
    # four windows of ONE shape, and one of another
    "batch-0": (_batch_shape, 1, {}), "batch-1": (_batch_shape, 2, {}), "batch-2": (_batch_shape, 3, {}), "batch-3": (_batch_shape, 4, {}),
    "batch-other": (lambda: synth.make_window(9, 3, 350, seed=72, run_lo=3, run_hi=6), 1, {}),
    # the inputs of tests/golden/lba_levels.npz (make_golden.py: cfg("small")'s shape, a tenth of the observations stereo)
    "golden": (lambda: synth.make_window(8, 2, 200, 11, run_lo=2, run_hi=6, stereo_frac=0.1), 3, {}),
}
NAMES = list(WINDOWS)

_windows = {}


def window(name):
    """-> (levelled window, levels, the solve's further arguments); built once, callers must not modify it"""
    if name not in _windows:
        make, seed, kw = WINDOWS[name]
        w, lv = synth.with_levels(make(), seed)
        _windows[name] = (w, lv, kw)
    return _windows[name]


_oracle = {}


def oracle_solve(oracle_mod, name, **more):
    """the oracle's solve of window `name`, computed once and shared; callers must not modify it"""
    key = (name, tuple(sorted(more.items())))
    if key not in _oracle:
        w, _, kw = window(name)
        _oracle[key] = oracle_mod.solve(w, **dict(kw, **more))
    return _oracle[key]


class _WithArguments:
    """oracle_mod with the window's further solve arguments bound (order_noise.spread calls solve(w))"""

    def __init__(self, oracle_mod, kw):
        self._o, self._kw = oracle_mod, kw

    def solve(self, w):
        return self._o.solve(w, **self._kw)


def wrong_pair(w, lv):
    """the first two adjacent edges of one map point that lie on different levels, one of them at least on a free keyframe"""
    free = w.pose_fixed[w.edge_pose] == 0
    ok = (lv[:-1] != lv[1:]) & (w.edge_point[:-1] == w.edge_point[1:]) & (free[:-1] | free[1:])
    return int(np.flatnonzero(ok)[0])


def pose_move(a, b):
    return float(quat_angle(a["poses"][:, :4], b["poses"][:, :4]).max()), float(np.abs(a["poses"][:, 4:] - b["poses"][:, 4:]).max())


def test_table_is_the_extractors_float_table():
    t = synth.level_inv_sigma2()
    assert t.dtype == np.float64 and np.array_equal(t, t.astype(np.float32).astype(np.float64))      # floats, widened
    # (TABLE's figures have eight digits: within half a float ulp, 2^-24 relative; the same recurrence in double is 2e-7 ... 5e-7 off)
    assert np.abs(t / np.array(TABLE) - 1).max() <= 2.0 ** -24
    assert np.abs(1.0 / (1.2 ** np.arange(8)) ** 2 / np.array(TABLE) - 1).max() > 2.0 ** -23
    s = synth.level_scale_factors()
    assert s.dtype == np.float32 and s[0] == 1 and all(s[i] == np.float32(s[i - 1] * np.float32(1.2)) for i in range(1, 8))
    assert all(np.float32(t[i]) == np.float32(1.0) / np.float32(s[i] * s[i]) for i in range(8))
    # one definition: the scale factors of the point-normals cases are the same recurrence in double
    assert np.array_equal(point_normals_ref.SCALE_12, synth.level_scale_factors(8, 1.2, np.float64))
    assert np.array_equal(point_normals_ref.SCALE_12, np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)])))


def test_with_levels_copies_and_leaves_the_generators_alone():
    w0 = synth.cfg("small")
    w, lv = synth.with_levels(w0, 1)
    assert np.array_equal(w0.inv_sigma2, np.ones(w0.n_edges)) and w.inv_sigma2 is not w0.inv_sigma2
    assert lv.dtype == np.int32 and lv.shape == (w0.n_edges,) and np.array_equal(w.inv_sigma2, synth.level_inv_sigma2()[lv])
    for f in ("poses", "pose_fixed", "points", "edge_pose", "edge_point", "obs"):
        assert np.array_equal(getattr(w, f), getattr(w0, f)) and getattr(w, f) is not getattr(w0, f)
    w2, lv2 = synth.with_levels(w0, 1)
    assert np.array_equal(lv, lv2) and not np.array_equal(lv, synth.with_levels(w0, 2)[1])
    # independent draws with p(l) ~ 0.75^l: level 0 the most frequent, about a quarter of the edges
    n = np.bincount(lv, minlength=8)
    assert n.argmax() == 0 and 0.2 < n[0] / n.sum() < 0.35


@pytest.mark.parametrize("name", NAMES)
def test_every_window_uses_all_eight_levels(name):
    w, lv, _ = window(name)
    assert (np.bincount(lv, minlength=8) > 0).all() and lv.max() == 7
    assert len(np.unique(w.inv_sigma2)) == 8


def test_the_four_windows_of_one_shape_differ_in_their_weights_only():
    ws = [window(f"batch-{i}")[0] for i in range(4)]
    for w in ws[1:]:
        assert np.array_equal(w.obs, ws[0].obs) and np.array_equal(w.edge_pose, ws[0].edge_pose) and np.array_equal(w.poses, ws[0].poses)
        assert (w.inv_sigma2 != ws[0].inv_sigma2).mean() > 0.5
    assert window("batch-other")[0].n_edges != ws[0].n_edges


def test_the_golden_fixture_holds_the_levelled_window(oracle_mod):
    """tests/golden/lba_levels.npz: in test_oracle_golden.py's list (the oracle against the independent numpy LM) and in
    test_gpu_parity.test_golden_fixtures; its inputs are the window `golden` above, so teeth and clean side hold for it"""
    import test_oracle_golden
    assert "lba_levels" in test_oracle_golden.CASES
    g, out = load_golden("lba_levels")
    w, lv, _ = window("golden")
    for f in ("poses", "pose_fixed", "points", "edge_pose", "edge_point", "obs", "inv_sigma2", "obs_right"):
        assert np.array_equal(getattr(g, f), getattr(w, f)), f
    assert g.bf == w.bf and tuple(g.cam) == tuple(w.cam) and 0 < (g.obs_right >= 0).sum() < g.n_edges
    test_oracle_golden.test_oracle_matches_golden(oracle_mod, "lba_levels")


def test_long_track_window_has_points_with_more_than_sixteen_observers():
    w, _, _ = window("long-tracks")
    assert np.bincount(w.edge_point).max() > 16


def test_hard_window_ends_on_a_rejected_trial(oracle_mod):
    """the window of the GPU file's stale-error test: the last trial is rejected, so the two flag values give different chi2"""
    a, b = oracle_solve(oracle_mod, "hard"), oracle_solve(oracle_mod, "hard", stale_error_quirk=False)
    assert a["trace"]["accept"][-1] == 0 and a["trace"]["accept"][-2] == 0 and (a["trace"]["accept"] == 1).sum() >= 3
    assert np.array_equal(a["poses"], b["poses"]) and np.abs(a["chi2"] - b["chi2"]).max() > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_teeth_one_swapped_pair_or_a_shift_by_one_edge_moves_the_poses(oracle_mod, name):
    w, lv, kw = window(name)
    o = oracle_solve(oracle_mod, name)
    e = wrong_pair(w, lv)
    assert w.inv_sigma2[e] != w.inv_sigma2[e + 1]
    swapped, rolled = copy.deepcopy(w), copy.deepcopy(w)
    swapped.inv_sigma2[[e, e + 1]] = w.inv_sigma2[[e + 1, e]]
    rolled.inv_sigma2 = np.roll(w.inv_sigma2, 1)
    assert (swapped.inv_sigma2 != w.inv_sigma2).sum() == 2 and np.array_equal(np.sort(rolled.inv_sigma2), np.sort(w.inv_sigma2))
    for label, bad in (("one swapped pair", swapped), ("rolled by one", rolled)):
        rot, trans = pose_move(oracle_mod.solve(bad, **kw), o)
        print(f"{name}, {label}: poses move by {rot:.3g} rad ({rot / ROT_TOL:.0f} x ROT_TOL), {trans:.3g} m ({trans / TRANS_TOL:.0f} x TRANS_TOL)")
        assert rot >= TEETH * ROT_TOL or trans >= TEETH * TRANS_TOL, (name, label)


@pytest.mark.parametrize("name", NAMES)
def test_clean_side_the_oracles_own_spread_is_a_tenth_of_the_tolerances(oracle_mod, name):
    w, _, kw = window(name)
    sp = spread(_WithArguments(oracle_mod, kw) if kw else oracle_mod, w, n=16)
    print(f"{name}: spread under 16 edge orders: rotation {sp.rot:.3g} rad, translation {sp.trans:.3g} m, points {sp.point:.3g} m, "
          f"lambda {sp.lam:.3g}, F1 {sp.f1:.3g}, chi2 {sp.chi2:.3g}")
    assert sp.n == 16 and sp.same_decisions
    assert sp.rot < ROT_TOL / 10 and sp.trans < TRANS_TOL / 10 and sp.point < POINT_TOL / 10
    # check_against's defaults for the traces and the per-edge chi2 hold with the same margin
    assert sp.lam < order_noise.USUAL_LAM / 10 and sp.f1 < 1e-8 / 10 and sp.chi2 < order_noise.USUAL_CHI2[0] / 10
    o = oracle_solve(oracle_mod, name)
    assert order_noise.noise_floor_trial(o) == len(o["trace"]["accept"])                  # the accept sequence is decided, not noise
    fin = np.isfinite(o["chi2"])
    near = float(np.abs(o["chi2"][fin] - w.chi2_gate).min())
    print(f"{name}: nearest chi2 lies {near:.3g} from the gate")
    assert near > GUARD
    if kw:
        o2 = oracle_solve(oracle_mod, name, stale_error_quirk=False)
        assert float(np.abs(o2["chi2"] - w.chi2_gate).min()) > GUARD
