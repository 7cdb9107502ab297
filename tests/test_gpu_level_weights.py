"""The HIP path on windows whose edges carry the reference's pyramid-level weights (synth.with_levels: inv_sigma2 =
mvInvLevelSigma2[octave], eight levels from 1 down to 0.078), on every route inv_sigma2 travels and at every place it is consumed.

Every other synthetic window of the suite has weight 1 on every edge, which is the same array under any permutation, stale copy
or mix-up between windows.  tests/test_level_weights_cpu.py holds what makes these cases conclusive: on each window below ONE
swapped pair of neighbouring weights moves the oracle's poses by at least 100 x the tolerance, and the oracle's own spread under
edge permutation is a tenth of the tolerance or less - so check_against runs with its defaults and without noise_guard.

  upload     ordinary arrays grouped by point (staged), edges in any order (host gather), arrays in the library's pinned memory
             (copy engine), the host's grouping and structure passes
  re-use     one handle, window after window, across a regrown arena; weights overwritten in place between two calls on pinned
             arrays; the per-window tables of a batched run over windows of ONE shape
  consumers  k_point's two prefetched edges and its loop behind them (more than 16 observers), k_point_kf (a camera per
             keyframe), k_point_b (batched), the point kernels without the LDS image of the rotations, every reduced solver
             behind them, finalize_body's chi2 from either state buffer, the marginals' rho'(chi2) inv_sigma2"""
import numpy as np
import pytest

from order_noise import permuted, unpermute

import test_level_weights_cpu as L
from test_gpu_general_position import SOLVERS, assert_solver_that_ran
from test_gpu_marginals import _check as check_marginals
from test_gpu_parity import GUARD, POINT_TOL, ROT_TOL, TRANS_TOL, _shared_stream_solvers, check_against  # noqa: F401

pytestmark = pytest.mark.gpu

KEYS = ("poses", "points", "chi2", "outlier")


@pytest.fixture(scope="module")
def solvers(built_lib):
    s = {k: built_lib.Solver(**kw) for k, kw in SOLVERS.items()}
    yield s
    for v in s.values():
        v.close()


def same_bits(a, b, label):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (label, k)
    for k in ("accept", "f1", "lam", "pcg"):
        assert np.array_equal(a["trace"][k], b["trace"][k]), (label, k)
    assert a["n_solves"] == b["n_solves"] and a["status"] == b["status"] == 0, label


def copied(r):
    """a result whose arrays are the caller's own (solve_prepared hands out views of the prepared buffers)"""
    return dict(r, **{k: np.array(r[k]) for k in KEYS})


_fresh = {}


def fresh(built_lib, name):
    """window `name` solved by a handle that has seen nothing else, computed once"""
    if name not in _fresh:
        s = built_lib.Solver()
        try:
            _fresh[name] = s.solve(L.window(name)[0])
        finally:
            s.close()
    return _fresh[name]


# ---- every reduced solver ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(SOLVERS))
@pytest.mark.parametrize("name", ["small", "stereo", "cameras"])
def test_every_reduced_solver_on_levelled_windows(solvers, oracle_mod, name, which):
    """`cameras`: a camera per keyframe, the k_point_kf variants of the point kernels"""
    w, _, _ = L.window(name)
    r = solvers[which].solve(w)
    assert_solver_that_ran(r, which)
    check_against(r, L.oracle_solve(oracle_mod, name), w)


def test_default_handle_on_the_first_size_beyond_the_on_chip_pcg(solver, oracle_mod, built_lib):
    """81 free keyframes: dense_solve.hip on the handle every caller gets, three iterations"""
    w, _, _ = L.window("81kf")
    assert w.n_free == 81 and w.max_iters == 3 and not built_lib.structure_probe(w)["pcg_on_chip"]
    r = solver.solve(w)
    assert_solver_that_ran(r, "direct")
    check_against(r, L.oracle_solve(oracle_mod, "81kf"), w)


def test_long_tracks_run_the_loop_behind_the_two_prefetched_edges(solver, solvers, oracle_mod):
    """18 to 26 observers per point: k_point walks the edges beyond its two prefetched ones and beyond one pass of 16"""
    w, _, _ = L.window("long-tracks")
    assert np.bincount(w.edge_point).max() > 16
    o = L.oracle_solve(oracle_mod, "long-tracks")
    check_against(solver.solve(w), o, w)
    r = solvers["direct"].solve(w)
    assert_solver_that_ran(r, "direct")
    check_against(r, o, w)


def test_more_keyframes_than_the_point_kernels_stage_in_lds(solver, oracle_mod):
    """test_gpu_parity's window of 912 keyframes: rotations read through L2; two iterations (see the CPU file)"""
    w, _, _ = L.window("beyond-lds")
    assert w.n_poses > 900 and w.max_iters == 2
    check_against(solver.solve(w), L.oracle_solve(oracle_mod, "beyond-lds"), w)


# ---- upload routes ---------------------------------------------------------------------------------------------------
def test_the_three_upload_routes_give_the_same_bits_and_match_the_oracle(built_lib, solver, oracle_mod):
    """Staged copy of ordinary arrays grouped by point, the copy engine on arrays in the library's pinned memory, and the host
    gather for edges in any order: each against the oracle, and against each other bit for bit.  The order of a point's edges
    is part of the arithmetic (in the oracle too: test_level_weights_cpu measures 6e-14 m on this window), and the gather keeps
    the caller's order inside a point (a stable counting sort, structure.cpp): so the shuffled window's bits are those of the
    window handed over GROUPED in that order - which goes the staged route - and not those of cfg2's own order, from which it
    differs in the last digits (printed)."""
    w, _, _ = L.window("cfg2")
    o = L.oracle_solve(oracle_mod, "cfg2")
    staged = solver.solve(w)                                   # ordinary arrays grouped by point
    check_against(staged, o, w)
    # caller arrays in the library's pinned memory: read where they lie
    s = built_lib.Solver()
    try:
        s.prepare(w, pinned=True)
        pinned = copied(s.solve_prepared())
    finally:
        s.close()
    check_against(pinned, o, w)
    same_bits(pinned, staged, "pinned arrays")
    # edges in any order: the host gathers them by point, weights along with observations and right-image coordinates
    pm = np.random.default_rng(5).permutation(w.n_edges)
    wp = permuted(w, pm)
    assert not np.array_equal(wp.edge_point, np.sort(wp.edge_point)) and np.array_equal(wp.inv_sigma2, w.inv_sigma2[pm])
    in_callers_order = lambda r, p: dict(r, chi2=unpermute(r["chi2"], p), outlier=unpermute(r["outlier"], p))      # noqa: E731
    gathered = in_callers_order(solver.solve(wp), pm)
    check_against(gathered, o, w)
    grouped = pm[np.argsort(w.edge_point[pm], kind="stable")]          # what the gather makes of pm
    wg = permuted(w, grouped)
    assert np.array_equal(wg.edge_point, w.edge_point) and not np.array_equal(wg.edge_pose, w.edge_pose)
    same_bits(gathered, in_callers_order(solver.solve(wg), grouped), "edges in any order")
    print(f"shuffled against cfg2's own order: poses {np.abs(gathered['poses'] - staged['poses']).max():.3g}, points "
          f"{np.abs(gathered['points'] - staged['points']).max():.3g}, chi2 {np.abs(gathered['chi2'] - staged['chi2']).max():.3g}")


@pytest.mark.parametrize("hook", ["host_grouping", "host_structure"])
def test_host_passes_carry_the_weights_like_the_device_passes(built_lib, solver, oracle_mod, hook):
    """as test_gpu_parity's two equivalence tests: the test build with the host pass forced, bit-equal to the product library"""
    w, _, _ = L.window("stereo")
    a = solver.solve(w)
    hs = built_lib.Solver(hooks=True)
    try:
        hs.hook(hook, 1)
        b = hs.solve(w)
    finally:
        hs.close()
    same_bits(b, a, hook)
    check_against(b, L.oracle_solve(oracle_mod, "stereo"), w)


# ---- nothing stale -----------------------------------------------------------------------------------------------------
def test_a_handle_keeps_nothing_of_the_window_before(built_lib, oracle_mod):
    """`small` and `small-2` are ONE window with two sets of levels: every array but inv_sigma2 is the same, so a weight kept
    from the call before is the only thing that can differ.  Again after cfg2 has regrown the arena."""
    a1, a2, big = L.window("small")[0], L.window("small-2")[0], L.window("cfg2")[0]
    assert np.array_equal(a1.obs, a2.obs) and (a1.inv_sigma2 != a2.inv_sigma2).mean() > 0.5 and big.n_edges > 5 * a1.n_edges
    assert not np.array_equal(fresh(built_lib, "small")["poses"], fresh(built_lib, "small-2")["poses"])
    s = built_lib.Solver()
    try:
        same_bits(s.solve(a1), fresh(built_lib, "small"), "first window")
        same_bits(s.solve(a2), fresh(built_lib, "small-2"), "same window, other levels")
        same_bits(s.solve(big), fresh(built_lib, "cfg2"), "larger window")
        same_bits(s.solve(a1), fresh(built_lib, "small"), "first window behind the larger one")
        r = s.solve(a2)
        same_bits(r, fresh(built_lib, "small-2"), "other levels behind the larger one")
        check_against(r, L.oracle_solve(oracle_mod, "small-2"), a2)
    finally:
        s.close()


def test_weights_overwritten_in_pinned_arrays_between_two_calls_are_read_again(built_lib):
    a1, a2 = L.window("small")[0], L.window("small-2")[0]
    s = built_lib.Solver()
    try:
        s.prepare(a1, pinned=True)
        d, keep, r, out = s._prep
        same_bits(copied(s.solve_prepared()), fresh(built_lib, "small"), "as prepared")
        keep["isg"][...] = a2.inv_sigma2
        same_bits(copied(s.solve_prepared()), fresh(built_lib, "small-2"), "weights overwritten in place")
        keep["isg"][...] = a1.inv_sigma2
        same_bits(copied(s.solve_prepared()), fresh(built_lib, "small"), "and back")
    finally:
        s.close()


# ---- batched run -------------------------------------------------------------------------------------------------------
def test_batched_run_over_windows_of_one_shape_gives_each_its_own_weights(built_lib, oracle_mod):
    """Four windows that differ in inv_sigma2 ONLY (a window reading its neighbour's table would read in bounds), one of
    another shape between them: each bit-equal to its solo run, one against the oracle."""
    names = ["batch-0", "batch-1", "batch-other", "batch-2", "batch-3"]
    ws = [L.window(n)[0] for n in names]
    st, hs = _shared_stream_solvers(built_lib, len(ws))
    try:
        solo = [s.solve(w) for s, w in zip(hs, ws)]
        for i in (1, 3, 4):
            assert not np.array_equal(solo[i]["poses"], solo[0]["poses"]) and not np.array_equal(solo[i]["chi2"], solo[0]["chi2"])
        for s, w in zip(hs, ws):
            s.upload(w)
        assert built_lib.run_batch(hs) == 0
        res = [s.download() for s in hs]
        for n, a, b in zip(names, solo, res):
            same_bits(b, a, n)
        check_against(res[1], L.oracle_solve(oracle_mod, "batch-1"), ws[1])
        # the same handles, every window handed to another one of them, in another order
        order = [3, 4, 0, 1, 2]
        for s, j in zip(hs, order):
            s.upload(ws[j])
        assert built_lib.run_batch(hs[::-1]) == 0
        for s, j in zip(hs, order):
            same_bits(s.download(), solo[j], f"{names[j]} on another handle")
    finally:
        for s in hs:
            s.close()


# ---- marginals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "stereo"])
def test_marginals_of_levelled_windows(solver, oracle_mod, name):
    w, _, _ = L.window(name)
    r = solver.solve(w)
    check_against(r, L.oracle_solve(oracle_mod, name), w)
    for damping in (0.0, 1e-3):
        check_marginals(w, r, solver.marginals(damping), damping, f"levelled {name}")


# ---- stale-error quirk ---------------------------------------------------------------------------------------------------
def test_stale_error_quirk_after_a_rejected_last_trial_on_a_levelled_window(solver, oracle_mod, built_lib):
    """lba_hard's inputs with levels, two trials per iteration: the solve ends on a rejected trial (asserted on the oracle in
    the CPU file), and finalize_body computes chi2 = inv_sigma2 |e|^2 from the rejected trial's state (flag set, as g2o leaves it)
    or from the restored one (flag clear) - the weight has to be the right edge's for either state buffer."""
    w, _, kw = L.window("hard")
    got = {}
    for quirk in (True, False):
        r = solver.solve(w, flags=built_lib.FLAG_STALE_ERROR_QUIRK if quirk else 0, **kw)
        o = L.oracle_solve(oracle_mod, "hard", stale_error_quirk=quirk)
        assert r["last_rejected"] == 1 and o["trace"]["accept"][-1] == 0
        check_against(r, o, w)
        got[quirk] = r
    assert np.array_equal(got[True]["poses"], got[False]["poses"]) and np.abs(got[True]["chi2"] - got[False]["chi2"]).max() > 1e-3
