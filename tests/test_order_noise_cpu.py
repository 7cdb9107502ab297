"""What the order-noise bounds of tests/test_gpu_parity.py rest on (no GPU): tests/order_noise.py measures what it says it
measures, reproducibly; the oracle takes the same decisions under every edge order tried, on all 14 sweep windows; ordinary
windows keep the usual tolerances; the six older sweep windows are never held looser than before."""
import inspect

import numpy as np
import pytest

import order_noise
import test_gpu_parity as parity
from conftest import load_golden, oracle_order_noise
from movba import synth
from order_noise import Spread, chi2_mixed, permuted, spread, tolerances, unpermute, within_point_permutation

USUAL_REST = dict(lam_rtol=1e-7, f1_rtol=1e-6, chi2_tol=(1e-6, 1e-7))


def sweep_window(K, F, P, lo, hi, stereo, seed):
    return synth.make_window(K, F, P, seed=seed, run_lo=lo, run_hi=max(lo, hi), stereo_frac=stereo)


def test_the_classes_are_those_of_the_parity_module_and_check_against_defaults_are_unchanged():
    assert order_noise.MODULE_TOL == dict(rot=parity.ROT_TOL, trans=parity.TRANS_TOL, point=parity.POINT_TOL)
    assert parity.WEAK_TOL is order_noise.WEAK_TOL == dict(rot=1e-6, trans=1e-6, point=1e-4) and parity.GUARD == order_noise.GUARD
    assert parity.noise_floor_trial is order_noise.noise_floor_trial
    d = {k: p.default for k, p in inspect.signature(parity.check_against).parameters.items() if p.default is not p.empty}
    assert d == dict(rot=1e-8, trans=1e-8, point=1e-6, noise_guard=False, lam_rtol=1e-7, chi2_tol=(1e-6, 1e-7), f1_rtol=None)


def test_f1_rtol_none_is_the_former_bound_of_the_cost_trace(oracle_mod):
    """check_against(f1_rtol=None): 1e-6 under noise_guard, 1e-8 without, as before the argument existed; a given value holds."""
    w = synth.cfg("small")
    o = oracle_mod.solve(w)

    def moved(eps):
        r = dict(o, trace=dict(o["trace"], f1=o["trace"]["f1"] * (1 + eps)))
        return r
    parity.check_against(moved(5e-9), o, w)
    parity.check_against(moved(5e-7), o, w, noise_guard=True)
    parity.check_against(moved(1.5e-6), o, w, noise_guard=True, f1_rtol=2e-6)
    for eps, kw in ((5e-8, {}), (1.5e-6, dict(noise_guard=True)), (5e-7, dict(noise_guard=True, f1_rtol=1e-7))):
        with pytest.raises(AssertionError):
            parity.check_against(moved(eps), o, w, **kw)


def test_pool_and_serial_give_the_same_bits_and_first4_is_conftests_measure(oracle_mod):
    w = sweep_window(12, 3, 80, 2, 2, 0.0, 982937)
    assert w.n_edges == 160
    pooled = spread(oracle_mod, w, n=16, workers=8, cache=False)
    assert pooled == spread(oracle_mod, w, n=16, workers=1, cache=False)
    assert pooled == spread(oracle_mod, w, n=16, workers=8, cache=False)
    assert pooled == spread(oracle_mod, w, n=16) and spread(oracle_mod, w, n=16) is spread(oracle_mod, sweep_window(12, 3, 80, 2, 2, 0.0, 982937), n=16)
    assert pooled.first4 == oracle_order_noise(oracle_mod, w, n=4)
    assert (pooled.rot, pooled.trans, pooled.point) == oracle_order_noise(oracle_mod, w, n=16)
    # the window moves in every quantity: none of the comparisons above is 0 == 0
    assert min(pooled[:6]) > 1e-9 and all(a >= b for a, b in zip(pooled[:3], pooled.first4))


@pytest.mark.parametrize("K,F,P,lo,hi,stereo,seed", parity.BAND_SWEEP_WINDOWS + parity.LONG_SWEEP_WINDOWS)
def test_the_oracle_takes_the_same_decisions_under_every_edge_order(oracle_mod, K, F, P, lo, hi, stereo, seed):
    """The GPU cases compare the accept trace (up to the noise floor), n_solves and the outlier flags (outside the guard band)
    EXACTLY while widening everything else to the oracle's spread: that is only fair where the oracle's own decisions do not
    depend on the edge order."""
    sp = spread(oracle_mod, sweep_window(K, F, P, lo, hi, stereo, seed), n=16)
    assert sp.same_decisions and sp.n == 16
    assert all(np.isfinite(v) and v >= 0 for v in sp[:6])


@pytest.mark.parametrize("name", ["small", "cfg2", "lba_stereo"])
def test_ordinary_windows_keep_the_usual_tolerances(oracle_mod, name):
    w = load_golden(name)[0] if name.startswith("lba_") else synth.cfg(name)
    sp = spread(oracle_mod, w, n=16)
    assert sp.same_decisions
    assert order_noise.usual(w) == order_noise.MODULE_TOL
    assert 3 * sp.rot <= 1e-8 and 3 * sp.trans <= 1e-8 and 3 * sp.point <= 1e-6 and 3 * sp.lam <= 1e-7 and 3 * sp.f1 <= 1e-6 and 3 * sp.chi2 <= 1e-6
    assert tolerances(w, sp) == dict(order_noise.MODULE_TOL, **USUAL_REST)


@pytest.mark.parametrize("K,F,P,lo,hi,stereo,seed", parity.BAND_SWEEP_WINDOWS)
def test_the_older_sweep_windows_are_never_held_looser_than_before(oracle_mod, K, F, P, lo, hi, stereo, seed):
    """test_banded_factorisation_on_the_windows_the_sweep_found: the measured lambda / chi2 bounds lie at or below the constants
    that test had picked (1e-5, (1e-3, 1e-4)), the cost trace needs no more than its 1e-6, and what the test finally asks is
    at or below what it asked of THIS window before (the usual values where the picked ones did not apply); poses as before."""
    w = sweep_window(K, F, P, lo, hi, stereo, seed)
    sp = spread(oracle_mod, w, n=16)
    t16 = tolerances(w, sp)
    assert t16["lam_rtol"] <= 1e-5 and t16["chi2_tol"][0] <= 1e-3 and t16["chi2_tol"][1] <= 1e-4 and 3 * sp.f1 <= 1e-6
    tol, usual, noise = parity._band_sweep_bounds(w, oracle_mod)
    was_noisy = 3 * noise[1] > usual["trans"]
    assert tol["lam_rtol"] <= (1e-5 if was_noisy else 1e-7) and tol["f1_rtol"] == 1e-6
    assert tol["chi2_tol"][0] <= (1e-3 if was_noisy else 1e-6) and tol["chi2_tol"][1] <= (1e-4 if was_noisy else 1e-7)
    assert noise == sp.first4 and usual == order_noise.usual(w)
    assert {k: tol[k] for k in ("rot", "trans", "point")} == parity._sweep_tolerances(w, oracle_mod)[0]


def test_tolerances_are_the_larger_of_usual_and_factor_times_spread():
    w = synth.cfg("small")
    sp = Spread(rot=1e-9, trans=1e-8, point=1e-9, lam=1e-7, f1=1e-8, chi2=2e-6, same_decisions=True, first4=(0.0, 0.0, 0.0), n=16)
    t = tolerances(w, sp)
    assert t == dict(rot=1e-8, trans=3 * 1e-8, point=1e-6, lam_rtol=3 * 1e-7, f1_rtol=1e-6, chi2_tol=(3 * 2e-6, 3 * 2e-6 / 10))
    assert tolerances(w, sp, factor=3) == t and tolerances(w, sp, factor=1)["chi2_tol"] == (2e-6, 2e-6 / 10)
    # the classes by the least-observed free keyframe
    nth = np.cumsum(np.eye(w.n_poses, dtype=int)[w.edge_pose], 0)[np.arange(w.n_edges), w.edge_pose]      # edge e is its keyframe's nth
    assert order_noise.usual(w) == order_noise.MODULE_TOL
    assert order_noise.usual(permuted(w, np.flatnonzero(nth <= 12))) == order_noise.MODULE_TOL
    assert order_noise.usual(permuted(w, np.flatnonzero(nth <= 11))) == order_noise.WEAK_TOL
    assert order_noise.usual(permuted(w, np.flatnonzero(nth <= 3))) == order_noise.WEAK_TOL
    assert order_noise.usual(permuted(w, np.flatnonzero(nth <= 2))) == order_noise.DEGENERATE_TOL


def test_per_edge_results_of_a_permuted_solve_are_put_back_in_caller_order(oracle_mod):
    """unpermute against the definition, and on a real solve: a permuted window's chi2 comes back in ITS edge order; put back,
    it matches the caller-order solve to the window's own spread, applied the wrong way round it is off by far more."""
    pm = np.array([2, 0, 3, 1])
    a = np.array([10.0, 11.0, 12.0, 13.0])
    assert np.array_equal(unpermute(a[pm], pm), a) and not np.array_equal(a[pm][pm], a)
    w = sweep_window(40, 1, 1500, 3, 3, 0.0, 166442)          # every point seen three times: orders inside a point that are not swaps
    sp = spread(oracle_mod, w, n=16)
    pm = within_point_permutation(w, 5)
    assert np.array_equal(w.edge_point[pm], np.sort(w.edge_point)) and not np.array_equal(pm[pm], np.arange(w.n_edges))   # (its own inverse would hide an inverted un-permutation)
    w2 = permuted(w, pm)
    assert np.array_equal(w2.obs, w.obs[pm]) and np.array_equal(w2.edge_pose, w.edge_pose[pm])
    o, o2 = oracle_mod.solve(w), oracle_mod.solve(w2)
    back = np.empty_like(o2["chi2"])
    for i, e in enumerate(pm): back[e] = o2["chi2"][i]           # edge i of the permuted window IS edge pm[i] of the caller's
    assert np.array_equal(unpermute(o2["chi2"], pm), back)
    assert chi2_mixed(back, o["chi2"]) <= sp.chi2 < 1e-6
    assert chi2_mixed(o2["chi2"][pm], o["chi2"]) > 1e3 * sp.chi2


def test_the_chi2_metric_is_assert_allcloses_own_criterion():
    ref = np.array([0.0, 0.05, 1.0, 7.3, 100.0])
    d = np.array([2e-7, -1e-7, 3e-6, 1e-5, -2e-4])                         # largest |d| / (0.1 + |ref|) at ref = 1: 3e-6 / 1.1
    s = chi2_mixed(ref + d, ref)
    assert np.isclose(s, 3e-6 / 1.1, rtol=1e-9)
    np.testing.assert_allclose(ref + d, ref, rtol=s * (1 + 1e-9), atol=s * (1 + 1e-9) / 10)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(ref + d, ref, rtol=s * (1 - 1e-6), atol=s * (1 - 1e-6) / 10)
    # edges whose chi2 is not finite on either side (a point on a keyframe's z = 0 plane) are left out
    c, r = np.array([1.0, np.inf, 5.0, np.nan]), np.array([1.0, np.inf, np.inf, 2.0])
    assert chi2_mixed(c, r) == 0.0
