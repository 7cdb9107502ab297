"""movba_init_map on the GPU: against the restatement of tests/test_init_map_cpu.py (the oracle's bundle adjustment + numpy) on the
committed cases, against the library's own local-BA path on the same windows (two independent routes to one answer), its
invariances to the bit (batch = solo calls, permutation, repetition, pinned = ordinary result memory, mask = compacted layout),
the chain behind movba_two_view_lo, normalisation only, the refusals and an uploaded window left untouched.  Tolerances are
tests/order_noise.py's: max(the suite's usual ones, 3 x the oracle's own spread on that window); costs are compared down to the
rounding floor of fp64 residuals (test_init_map_cpu.cost_floor)."""
import numpy as np
import pytest

import order_noise
import test_init_map_cpu as M
import test_two_view_cpu as T
from movba import capi, synth

pytestmark = pytest.mark.gpu

SCALARS = ("status", "outcome", "median_depth", "n_used", "iters_done", "n_solves", "last_rejected", "n_chol_fail", "lam", "cost0", "cost")
ARRAYS = ("pose", "points", "chi2")
TRACE = ("lam", "f0", "f1", "rho", "accept")


def call_args(pair):
    """the keys Solver.init_map reads (the cases carry their truth beside them)"""
    return {k: v for k, v in pair.items() if not k.startswith("truth") and k != "spec"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.size else a.reshape(-1).view(np.uint8)


def same_bits(a, b, slots=None):
    """every field of two results equal to the bit, traces included; slots: (mask of a, mask of b) - the per-match arrays are
    compared in those slots only"""
    for k in SCALARS:
        if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes():
            return False
    for k in ARRAYS:
        x, y = (a[k], b[k]) if slots is None or k == "pose" else (a[k][slots[0]], b[k][slots[1]])
        if x.shape != y.shape or not np.array_equal(bits(x), bits(y)):
            return False
    return all(np.array_equal(bits(a["trace"][k]), bits(b["trace"][k])) for k in TRACE)


@pytest.fixture(scope="module")
def solved(solver):
    """the committed cases through ONE call, shared by the tests below (nothing changes it)"""
    return solver.init_map([call_args(p) for p in M.PAIRS()], trace=True)


@pytest.mark.parametrize("k", range(len(M._SPECS)), ids=[f"{s['scene']}-{s['n_used']}" for s in M._SPECS])
def test_against_the_restatement(solved, oracle_mod, k):
    pair, ref = M.PAIRS()[k], M.ref_of(oracle_mod, k)
    w = ref["window"]
    tol = order_noise.tolerances(w, order_noise.spread(oracle_mod, w))
    M.check(pair, solved[k], ref, w, tol, ref["oracle"])


@pytest.mark.parametrize("k", range(len(M._SPECS)), ids=[f"{s['scene']}-{s['n_used']}" for s in M._SPECS])
def test_against_the_local_ba_path(solved, solver, oracle_mod, k):
    """The same window through movba_lba_solve (chi2 at the returned estimate) with stages 3 and 4 on the host."""
    pair = M.PAIRS()[k]
    w = M.window_of(pair)
    r = solver.solve(w, flags=0, max_iters=w.max_iters)
    assert r["status"] == 0
    ref = M.finish(pair, r["poses"], r["points"], r["chi2"])
    ref.update(cost0=r["cost0"], cost=r["cost"])
    tol = order_noise.tolerances(w, order_noise.spread(oracle_mod, w))
    M.check(pair, solved[k], ref, w, tol, r)


def _batch64():
    """64 mixed pairs: the committed cases, pairs without a match, pairs whose mask is all zero, and more sizes around the wave and
    workgroup boundaries, with and without a mask"""
    out = [call_args(p) for p in M.PAIRS()]
    sizes = [1, 2, 5, 6, 12, 63, 64, 65, 130, 255, 256, 257, 300]
    scenes = ("general", "planar", "forward")
    k = 0
    while len(out) < 64:
        if k % 9 == 4:
            p = call_args(M.make_pair(7, "general", seed=300 + k))
            p.update(obs1=np.zeros((0, 2)), obs2=np.zeros((0, 2)), points=np.zeros((0, 3)))
        elif k % 9 == 7:
            p = call_args(M.make_pair(9, "planar", seed=300 + k))
            p["use"] = np.zeros(9, np.uint8)
        else:
            p = call_args(M.make_pair(sizes[k % len(sizes)], scenes[k % 3], seed=300 + k, mismatch=0.03 if k % 4 == 1 else 0.0,
                                      mask=k % 5 == 2, sigmas=k % 7 == 3, max_iters=[20, 7, 3][k % 3]))
        out.append(p)
        k += 1
    return out


def test_a_batch_equals_its_solo_calls_permutes_repeats_and_ignores_where_results_live(solver):
    pairs = _batch64()
    a = solver.init_map(pairs, trace=True)
    assert sum(r["status"] == capi.EMPTY for r in a) >= 8 and all(r["status"] in (0, capi.EMPTY) for r in a)
    for r, p in zip(a, pairs):
        if r["status"] == capi.EMPTY:
            assert r["n_used"] == 0 and r["n_solves"] == 0 and len(r["trace"]["lam"]) == 0 and np.isnan(r["median_depth"])
            assert r["outcome"] == M.IM_FEW_TRACKED and not r["points"].any() and not r["chi2"].any()       # (no array written)
    for k, p in enumerate(pairs):
        assert same_bits(solver.init_map([p], trace=True)[0], a[k]), k
    pm = np.random.default_rng(5).permutation(len(pairs))
    b = solver.init_map([pairs[i] for i in pm], trace=True)
    assert all(same_bits(b[j], a[i]) for j, i in enumerate(pm))
    assert all(same_bits(x, y) for x, y in zip(solver.init_map(pairs, trace=True), a))
    assert all(same_bits(x, y) for x, y in zip(solver.init_map(pairs, pinned=True, trace=True), a))


def test_placement_mixed_per_pair_and_per_array_gives_the_same_bits(solver):
    """pair 0: points pinned, chi2 ordinary; pair 1: chi2 pinned, points ordinary; pair 2: a mask that leaves no used match;
    pair 3: chi2 left out - every result field and array as with everything in ordinary memory"""
    cases = M.PAIRS()
    pairs = [call_args(cases[5]), call_args(cases[6]), dict(call_args(cases[3]), use=np.zeros(12, np.uint8)),
             dict(call_args(cases[10]), chi2=False)]
    want = solver.init_map(pairs, trace=True)
    got = solver.init_map(pairs, pinned=[{"points"}, {"chi2"}, set(), set()], trace=True)
    assert [r["status"] for r in want] == [0, 0, capi.EMPTY, 0] and want[3]["chi2"] is None and got[3]["chi2"] is None
    assert want[3]["points"][M.used(pairs[3])].any() and not want[2]["points"].any()
    none = np.zeros((0, 2))
    for k, (a, b) in enumerate(zip(want, got)):
        assert same_bits(dict(a, chi2=none) if k == 3 else a, dict(b, chi2=none) if k == 3 else b), k


def test_the_mask_layout_gives_the_bits_of_the_compacted_layout(solver):
    compact = [call_args(M.make_pair(n, sc, seed=500 + n, mismatch=0.03)) for n, sc in ((1, "general"), (65, "planar"), (257, "forward"), (300, "general"))]
    spread = [M.spread_out(p, 3) for p in compact] + [M.spread_out(p, 4, fill=1e300) for p in compact]
    got = solver.init_map(compact + spread, trace=True)
    for j, p in enumerate(spread):
        c = got[j % len(compact)]
        assert same_bits(c, got[len(compact) + j], slots=(slice(None), M.used(p))), j


def test_chain_behind_two_view_lo(solver, oracle_mod):
    """movba_two_view_lo's pose, points and good handed over unchanged."""
    scenes = [(label, args, iters, seed) for label, args, iters, seed in T.SCENES if label.startswith("general")]
    tvs = [dict(synth.make_two_view(**args), ransac_iters=iters, ransac_seed=seed) for _, args, iters, seed in scenes]
    first = solver.two_view(tvs, pinned=True, lo_iters=10)
    pairs = []
    for tv, f in zip(tvs, first):
        assert f["status"] == 0 and f["outcome"] == T.TV_OK
        g = f["good"] != 0
        pairs.append(dict(obs1=tv["obs1"], obs2=tv["obs2"], points=f["points"], use=f["good"], pose2=f["pose"], cam=tv["cam"],
                          truth_R=tv["R"], truth_t=tv["t"], truth_X=tv["X"][g], truth_inlier=tv["is_inlier"][g]))
    got = solver.init_map([call_args(p) for p in pairs], pinned=True)
    for p, g, (label, *_) in zip(pairs, got, scenes):
        u = M.used(p)
        ref = M.ref_init_map(oracle_mod, p)
        assert g["status"] == 0 and g["outcome"] == M.IM_OK == ref["outcome"] and g["cost"] <= g["cost0"]
        z = np.sort(g["points"][u][:, 2])
        assert abs(z[(g["n_used"] - 1) // 2] - 1.0) <= 4 * np.finfo(float).eps
        eg, er = M.truth_error(p, g["pose"], g["points"][u]), M.truth_error(p, ref["pose"], ref["points"][u])
        print(label, "error to truth (rotation, translation direction, map): init_map", eg, "restatement", er)
        assert all(a <= 1.5 * b for a, b in zip(eg, er))


def test_zero_iterations_normalise_only(solver):
    pairs = [dict(call_args(M.make_pair(n, "general", seed=600 + n, mask=n == 65)), max_iters=0) for n in (60, 65, 300)]
    for p, g in zip(pairs, solver.init_map(pairs, trace=True)):
        u = M.used(p)
        X = np.asarray(p["points"])[u]
        med = np.sort(X[:, 2])[(len(X) - 1) // 2]
        q = np.asarray(p["pose2"][:4]); q = q / np.linalg.norm(q)
        assert g["status"] == 0 and g["outcome"] == M.IM_OK and g["n_solves"] == 0 and g["iters_done"] == 0 and len(g["trace"]["lam"]) == 0
        assert g["median_depth"] == med and g["cost0"] == g["cost"] > 0
        assert np.array_equal(g["points"][u], X * (1.0 / med)) and np.array_equal(g["pose"][4:], np.asarray(p["pose2"][4:]) * (1.0 / med))
        assert np.abs(g["pose"][:4] - q).max() < 1e-15


def _refused(solver, pair, n=1, null=None):
    """one call with the descriptor of `pair`; -> (return code, result struct, result arrays)"""
    d, r, keep = capi.init_map_desc(pair)
    keep["points"][...] = 7.0; keep["chi2"][...] = 7.0
    r.median_depth = 7.0; r.n_used = 7
    if null:
        setattr(d if null != "rpoints" else r, "points" if null == "rpoints" else null, None)
    descs = (capi.InitMapDesc * 1)(d); res = (capi.InitMapResult * 1)(r)
    rc = solver._L.movba_init_map(solver._h, descs, res, n, None)
    return rc, res[0], keep


def test_refusals_write_nothing_but_the_status(solver, built_lib):
    good = call_args(M.make_pair(20, "general", seed=700))
    bad = [dict(good, max_iters=-1), dict(good, max_iters=capi.MAX_INIT_MAP_ITERS + 1), dict(good, max_trials=-1), dict(good, min_tracked=-1),
           dict(good, cam=(0.0, 457.0, 367.0, 248.0)), dict(good, cam=(458.0, np.inf, 367.0, 248.0)), dict(good, cam=(458.0, 457.0, np.nan, 248.0)),
           dict(good, huber_delta=np.nan), dict(good, pose2=[0, 0, 0, 0, 1, 0, 0]), dict(good, pose2=[0, 0, 0, 1, np.inf, 0, 0])]
    for p in bad:
        rc, r, keep = _refused(solver, p)
        assert rc == capi.ERR_ARG and r.status == capi.ERR_ARG and r.median_depth == 7.0 and r.n_used == 7
        assert (keep["points"] == 7.0).all() and (keep["chi2"] == 7.0).all()
    for null in ("obs1", "obs2", "points", "rpoints"):
        rc, r, keep = _refused(solver, good, null=null)
        assert rc == capi.ERR_ARG and r.status == capi.ERR_ARG and (keep["points"] == 7.0).all()
    L, h = solver._L, solver._h
    d, r, keep = capi.init_map_desc(good)
    descs = (capi.InitMapDesc * 1)(d); res = (capi.InitMapResult * 1)(r)
    assert L.movba_init_map(None, descs, res, 1, None) == capi.ERR_ARG and L.movba_init_map(h, descs, res, -1, None) == capi.ERR_ARG
    assert L.movba_init_map(h, descs, res, capi.MAX_TWO_VIEW_BATCH + 1, None) == capi.ERR_ARG
    assert L.movba_init_map(h, None, res, 1, None) == capi.ERR_ARG and L.movba_init_map(h, descs, None, 1, None) == capi.ERR_ARG
    assert L.movba_init_map(h, None, None, 0, None) == capi.OK and not keep["points"].any()
    d.n_matches = capi.MAX_TWO_VIEW_MATCHES + 1
    descs[0] = d
    assert L.movba_init_map(h, descs, res, 1, None) == capi.ERR_ARG and not keep["points"].any()
    # one invalid descriptor among valid ones: nothing is solved
    two = solver.init_map([good, good])
    d2, r2, k2 = capi.init_map_desc(dict(good, max_iters=-1))
    d1, r1, k1 = capi.init_map_desc(good)
    descs = (capi.InitMapDesc * 2)(d1, d2); res = (capi.InitMapResult * 2)(r1, r2)
    assert L.movba_init_map(h, descs, res, 2, None) == capi.ERR_ARG and res[0].status == res[1].status == capi.ERR_ARG
    assert not k1["points"].any() and two[0]["points"].any()


def test_an_uploaded_window_is_left_as_it_was(built_lib):
    w = synth.cfg("small")
    pairs = [call_args(p) for p in M.PAIRS()[3:8]]
    outs = []
    for between in (False, True):
        s = built_lib.Solver()
        s.upload(w)
        if between:
            s.init_map(pairs)
        assert s.run() == 0
        a = s.download()
        if between:
            s.init_map(pairs)
        b = s.download()
        s.close()
        outs.append((a, b))
    for key in ("poses", "points", "chi2", "outlier"):
        ref = bits(outs[0][0][key])
        assert all(np.array_equal(bits(o[key]), ref) for pair in outs for o in pair), key
    assert outs[0][0]["n_solves"] == outs[1][0]["n_solves"] == outs[1][1]["n_solves"]
