"""movba_init_map without a GPU: the restatement the GPU tests compare against (ref_init_map: the oracle's bundle adjustment on
the two-keyframe window of include/movba.h's stage 1, stages 3 and 4 in numpy), the committed cases (PAIRS), properties of the
restatement itself, and the host side of the call - checks, packing, copy-out, handle sharing - under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer (tests/init_map: a stand-alone driver against the stand-in runtime of
tests/hipstub and a fake device of its own)."""
import copy
import os
import subprocess

import numpy as np
import pytest

import order_noise

from conftest import ROOT, quat_angle
from movba import synth

IM_OK, IM_NEG_DEPTH, IM_FEW_TRACKED = 0, 1, 2
HUBER = float(np.sqrt(np.float32(5.0)))
IM_DIR = os.path.join(ROOT, "tests", "init_map")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")


# ---- the committed cases -------------------------------------------------------------------------------------------------

NOISE_PX = 0.05


def make_pair(n_used, scene="general", seed=0, mismatch=0.0, mask=False, negate=False, min_tracked=50, max_iters=20, huber=HUBER,
              sigmas=False):
    """One case: synth.make_two_view's scene with n_used matches, and a start disturbed the way a minimal-sample pose and a
    linear triangulation are: rotation by ~2e-3 rad, translation direction by ~5e-3, depths by ~2 %.  mismatch: that share of the
    matches keeps a second observation anywhere in the image (Huber acts, trials get rejected).  mask: the used matches are
    spread out under a `use` mask, with NaN in every slot that is not used.  negate: every start point mirrored through camera
    1 (all depths negative).  sigmas: per-match information of a few octaves instead of 1.  Observation noise: NOISE_PX - at the
    scenes' depths of 4 - 40 baselines a point 40 baselines away has 11 px of parallax, so its depth is known to 2 % only when
    the observations are good to ~0.1 px: with less noise than that the observations say more about the map than the
    disturbed start does, and the truth tests below have something to show.
    -> dict for Solver.init_map, with truth_R, truth_t, truth_X (used matches) and spec beside it."""
    tv = synth.make_two_view(n_used, inlier_frac=1.0 - mismatch, noise_px=NOISE_PX, seed=seed, scene=scene)
    rng = np.random.default_rng(1000 + seed)
    w = rng.normal(0, 2e-3 / np.sqrt(3), 3)
    R0 = synth._rodrigues(w) @ tv["R"]
    t0 = tv["t"] + rng.normal(0, 5e-3 / np.sqrt(3), 3)
    t0 /= np.linalg.norm(t0)
    X0 = tv["X"] * (1.0 + rng.normal(0, 0.02, (n_used, 1)))
    if negate:
        X0 = -X0
    pair = dict(obs1=tv["obs1"], obs2=tv["obs2"], points=X0, pose2=np.concatenate([synth.quat_from_R(R0), t0]), cam=tv["cam"],
                min_tracked=min_tracked, max_iters=max_iters, huber_delta=huber)
    if sigmas:
        lv = synth.level_scale_factors(4, 1.2, np.float64)[rng.integers(0, 4, (2, n_used))]
        pair["inv_sigma2_1"], pair["inv_sigma2_2"] = 1.0 / lv[0] ** 2, 1.0 / lv[1] ** 2
    if mask:
        pair = spread_out(pair, seed)
    pair.update(truth_R=tv["R"], truth_t=tv["t"], truth_X=tv["X"], truth_inlier=tv["is_inlier"],
                spec=f"{scene}-{n_used}" + ("-mm" if mismatch else "") + ("-mask" if mask else "") + ("-neg" if negate else ""))
    return pair


def spread_out(pair, seed=0, fill=np.nan):
    """The same pair under a `use` mask: its matches keep their order in a longer list whose other slots hold `fill`."""
    n = len(pair["obs1"])
    rng = np.random.default_rng(77 + seed)
    m = n + max(3, n // 3)
    use = np.zeros(m, np.uint8)
    use[np.sort(rng.choice(m, n, replace=False))] = 1
    out = dict(pair)
    for key, width in (("obs1", 2), ("obs2", 2), ("points", 3), ("inv_sigma2_1", 0), ("inv_sigma2_2", 0)):
        if pair.get(key) is None:
            continue
        a = np.full((m, width) if width else (m,), fill)
        a[use == 1] = pair[key]
        out[key] = a
    out["use"] = use
    return out


def used(pair):
    u = pair.get("use")
    return np.ones(len(pair["obs1"]), bool) if u is None else np.asarray(u) != 0


# (the gross mismatches sit on planar and forward scenes: the general ones carry the comparison with the generating truth)
_SPECS = [dict(n_used=1, scene="general", seed=1), dict(n_used=5, scene="planar", seed=2), dict(n_used=6, scene="forward", seed=3),
          dict(n_used=12, scene="general", seed=4),                                           # (below min_tracked)
          dict(n_used=63, scene="planar", seed=5, mismatch=0.03), dict(n_used=64, scene="general", seed=6),
          dict(n_used=65, scene="forward", seed=7, sigmas=True), dict(n_used=255, scene="general", seed=8),
          dict(n_used=256, scene="planar", seed=9, mismatch=0.02), dict(n_used=257, scene="forward", seed=10, mismatch=0.03),
          dict(n_used=300, scene="general", seed=11, mask=True),
          dict(n_used=300, scene="general", seed=12, negate=True),
          dict(n_used=1200, scene="general", seed=13), dict(n_used=1200, scene="forward", seed=14, mismatch=0.02)]
_pairs = None


def PAIRS():
    global _pairs
    if _pairs is None:
        _pairs = [make_pair(**s) for s in _SPECS]
    return _pairs


# ---- the restatement -----------------------------------------------------------------------------------------------------

def window_of(pair):
    """Stage 1 of include/movba.h as a synth.Window: keyframe 1 fixed at the identity, keyframe 2 free at pose2, one point per
    used match in match order, each with the edge in keyframe 1 first."""
    u = used(pair)
    n = int(u.sum())
    q = np.asarray(pair["pose2"], np.float64).copy()
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], q], np.float64)
    obs = np.stack([np.asarray(pair["obs1"], np.float64)[u], np.asarray(pair["obs2"], np.float64)[u]], 1).reshape(-1, 2)
    s1 = np.ones(len(u)) if pair.get("inv_sigma2_1") is None else np.asarray(pair["inv_sigma2_1"], np.float64)
    s2 = np.ones(len(u)) if pair.get("inv_sigma2_2") is None else np.asarray(pair["inv_sigma2_2"], np.float64)
    return synth.Window(poses=poses, pose_fixed=np.array([1, 0], np.uint8), points=np.asarray(pair["points"], np.float64)[u].copy(),
                        edge_pose=np.tile(np.array([0, 1], np.int32), n), edge_point=np.repeat(np.arange(n, dtype=np.int32), 2),
                        obs=obs, inv_sigma2=np.stack([s1[u], s2[u]], 1).reshape(-1), cam=tuple(pair["cam"]),
                        huber_delta=pair.get("huber_delta", HUBER), max_iters=pair.get("max_iters", 20))


def finish(pair, poses, points, chi2):
    """Stages 3 and 4 on a bundle adjustment's result (poses (2, 7), points and chi2 of the used matches) -> the fields of
    Solver.init_map's dict that follow from them, per-match arrays in the pair's own layout."""
    u = used(pair)
    n = int(u.sum())
    z = points[:, 2]
    med = float(np.sort(z)[(n - 1) // 2])
    outcome = IM_NEG_DEPTH if med < 0 else IM_FEW_TRACKED if n < pair.get("min_tracked", 50) else IM_OK
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / med if outcome == IM_OK else 1.0
        pose = poses[1].copy()
        pose[4:] = pose[4:] * inv
        P = np.full((len(u), 3), np.nan)
        P[u] = points * inv
    c2 = np.full((len(u), 2), np.nan)
    c2[u] = chi2.reshape(-1, 2)
    return dict(pose=pose, points=P, chi2=c2, median_depth=med, outcome=outcome, n_used=n)


def ref_init_map(oracle_mod, pair):
    w = window_of(pair)
    o = oracle_mod.solve(w, stale_error_quirk=False, max_iters=w.max_iters, max_trials=pair.get("max_trials", 0))
    r = finish(pair, o["poses"], o["points"], o["chi2"])
    r.update(status=0, oracle=o, window=w, cost0=o["cost0"], cost=o["cost"], iters_done=o["iters_done"], n_solves=o["n_solves"],
             lam=o["lam"], trace=o["trace"])
    return r


def normalised(pair, res):
    """pose and points of a result with the scale taken out whatever the outcome (what is compared when a bound is given for
    normalised quantities): translation and points over the median depth."""
    m = res["median_depth"]
    s = 1.0 if res["outcome"] == IM_OK else 1.0 / m
    return res["pose"][4:] * s, res["points"][used(pair)] * s


def truth_error(pair, pose, points):
    """(rotation [rad], translation direction [rad], points: rms distance over the matches that are no mismatches, after both
    sides are scaled to median depth 1) of an estimate (pose (7,), points of the used matches) to the generating truth, up to
    scale."""
    rot = float(quat_angle(pose[None, :4], synth.quat_from_R(pair["truth_R"])[None])[0])
    t = pose[4:] / np.linalg.norm(pose[4:])
    ang = float(np.arccos(np.clip(t @ pair["truth_t"], -1, 1)))
    X, Xt = points, pair["truth_X"]
    g = pair["truth_inlier"]
    pt = float(np.sqrt((np.linalg.norm(X / np.median(X[:, 2]) - Xt / np.median(Xt[:, 2]), axis=1)[g] ** 2).mean()))
    return rot, ang, pt


def cost_floor(w, rtol):
    """The robust cost below which two correct fp64 evaluations need not agree to the relative tolerance rtol.  A residual is
    obs - (f x / z + c): a difference of two numbers of the size of the observation, so however it is computed it carries an
    absolute rounding error of a few ulp of |obs| - 8 eps max|obs| bounds the four operations of the projection and the
    subtraction, 1.3e-12 px for a 752-pixel image - and chi2 = e^2 then carries 2 |e| delta.  Two evaluations agree to rtol only
    while the rms residual stays above 2 delta / rtol, i.e. the cost above n_edges (2 delta / rtol)^2.  The under-determined cases
    (1, 5, 6 matches) fit their observations exactly and reach costs of 1e-24: their last trials lie below this floor, where
    order_noise.noise_floor_trial's own clause for the rounding floor (1e-18 of the first cost) does not reach."""
    delta = 8 * np.finfo(float).eps * float(np.abs(w.obs).max())
    return w.n_edges * (2 * delta / rtol) ** 2


def raw(pair, res):
    """the bundle adjustment's own estimate behind a result: the rescaling of an accepted map undone"""
    s = res["median_depth"] if res["outcome"] == IM_OK else 1.0
    return res["pose"][4:] * s, res["points"][used(pair)] * s


def check(pair, g, ref, w, tol, trace_ref):
    """g (Solver.init_map, or anything with its fields) against ref (fields of ref_init_map / finish) on window w with
    order_noise.tolerances tol; trace_ref: the solve whose trace, n_solves and iters_done g's are held to, up to its noise floor:
    order_noise.noise_floor_trial, or the first trial whose F1 lies under cost_floor, whichever comes first."""
    u = used(pair)
    assert g["status"] == 0 and g["outcome"] == ref["outcome"] and g["n_used"] == ref["n_used"] == int(u.sum())
    assert np.isnan(g["points"][~u]).all() and np.isnan(g["chi2"][~u]).all()
    rot = float(quat_angle(g["pose"][None, :4], ref["pose"][None, :4])[0])
    (tg, Xg), (tr, Xr) = raw(pair, g), raw(pair, ref)
    (tgn, Xgn), (trn, Xrn) = normalised(pair, g), normalised(pair, ref)
    d = dict(rot=rot, trans=float(np.abs(tg - tr).max()), point=float(np.abs(Xg - Xr).max()),
             trans_n=float(np.abs(tgn - trn).max()), point_n=float(np.abs(Xgn - Xrn).max()),
             median=abs(g["median_depth"] - ref["median_depth"]), chi2=order_noise.chi2_mixed(g["chi2"][u], ref["chi2"][u]))
    print(pair.get("spec", ""), "distances", d, "tolerances", tol)
    assert d["rot"] < tol["rot"] and d["trans"] < tol["trans"] and d["point"] < tol["point"]
    assert d["trans_n"] < tol["trans"] and d["point_n"] < tol["point"] and d["median"] < tol["point"]
    np.testing.assert_allclose(g["chi2"][u], ref["chi2"][u], rtol=tol["chi2_tol"][0], atol=tol["chi2_tol"][1])
    floor = cost_floor(w, tol["f1_rtol"])
    np.testing.assert_allclose([g["cost0"], g["cost"]], [ref["cost0"], ref["cost"]], rtol=tol["f1_rtol"], atol=tol["f1_rtol"] * floor)
    o = trace_ref
    below = np.flatnonzero(o["trace"]["f1"] < floor)
    k0 = min(order_noise.noise_floor_trial(o), int(below[0]) if len(below) else len(o["trace"]["f1"]))
    if k0 == len(o["trace"]["accept"]):
        assert g["n_solves"] == o["n_solves"] and g["iters_done"] == o["iters_done"]
    assert len(g["trace"]["accept"]) >= k0 and np.array_equal(g["trace"]["accept"][:k0], o["trace"]["accept"][:k0])
    np.testing.assert_allclose(g["trace"]["lam"][:k0], o["trace"]["lam"][:k0], rtol=tol["lam_rtol"])
    np.testing.assert_allclose(g["trace"]["f1"][:k0], o["trace"]["f1"][:k0], rtol=tol["f1_rtol"])
    assert g["n_chol_fail"] == 0 and g["last_rejected"] == int(g["trace"]["accept"][-1] == 0)


_refs = {}


def ref_of(oracle_mod, k):
    """ref_init_map of PAIRS()[k], computed once per session and shared (callers must not change it)."""
    if k not in _refs:
        _refs[k] = ref_init_map(oracle_mod, PAIRS()[k])
    return _refs[k]


# ---- tests of the restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(_SPECS)), ids=[f"{s['scene']}-{s['n_used']}" for s in _SPECS])
def test_restatement_normalises_and_never_raises_the_cost(oracle_mod, k):
    pair, r = PAIRS()[k], ref_of(oracle_mod, k)
    o = r["oracle"]
    assert o["status"] == 0 and r["n_used"] == _SPECS[k]["n_used"] and r["cost"] <= r["cost0"]
    want = IM_NEG_DEPTH if _SPECS[k].get("negate") else IM_FEW_TRACKED if r["n_used"] < 50 else IM_OK
    assert r["outcome"] == want
    u = used(pair)
    assert np.isnan(r["points"][~u]).all() and np.isnan(r["chi2"][~u]).all() and np.isfinite(r["points"][u]).all()
    if r["outcome"] == IM_OK:
        z = np.sort(r["points"][u][:, 2])
        assert abs(z[(r["n_used"] - 1) // 2] - 1.0) <= 4 * np.finfo(float).eps
        assert abs(np.linalg.norm(r["pose"][4:]) * r["median_depth"] - np.linalg.norm(o["poses"][1, 4:])) < 1e-14
    else:
        assert np.array_equal(r["pose"], o["poses"][1]) and np.array_equal(r["points"][u], o["points"])


def test_restatement_spends_rejected_trials_and_huber_acts(oracle_mod):
    """The cases are not easy ones: somewhere trials are rejected, and the mismatched observations sit beyond the kernel."""
    rejected = huber = 0
    for k, s in enumerate(_SPECS):
        r = ref_of(oracle_mod, k)
        rejected += int((r["trace"]["accept"] == 0).sum())
        if s.get("mismatch"):
            huber += int((r["oracle"]["chi2"] > HUBER ** 2).sum())
    assert rejected > 0 and huber > 0


def pose_sigmas(oracle_mod, ref):
    """Standard deviations the observations themselves leave in the estimate, from the Gauss-Newton covariance at the oracle's
    result: NOISE_PX^2 times the inverse of the reduced 6 x 6 matrix S (points eliminated, information 1 per pixel^2), over the
    left tangent [omega; upsilon] of T21, with the scale gauge (upsilon along t: S's null vector) projected out.
    -> (rotation [rad], translation direction [rad]): root of the trace of the rotation block, and of D C D^T with
    D = (I - t t^T / |t|^2) [-[t]x | I] / |t|, the change of direction a tangent step makes."""
    w = copy.copy(ref["window"])
    o = ref["oracle"]
    w.poses, w.points = o["poses"].copy(), o["points"].copy()
    S = oracle_mod.linearize(w, 0.0)["S"]
    t = o["poses"][1, 4:]
    th = t / np.linalg.norm(t)
    g = np.concatenate([np.zeros(3), th])
    P = np.eye(6) - np.outer(g, g)
    cov = NOISE_PX ** 2 * np.linalg.pinv(P @ S @ P, rcond=1e-10, hermitian=True)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    D = (np.eye(3) - np.outer(th, th)) @ np.hstack([-tx, np.eye(3)]) / np.linalg.norm(t)
    return float(np.sqrt(np.trace(cov[:3, :3]))), float(np.sqrt(np.trace(D @ cov @ D.T)))


@pytest.mark.parametrize("k", [k for k, s in enumerate(_SPECS) if s["scene"] == "general" and s["n_used"] >= 5 and not s.get("negate")],
                         ids=lambda k: f"general-{_SPECS[k]['n_used']}")
def test_restatement_does_not_move_away_from_the_truth(oracle_mod, k):
    """Every general scene whose matches determine a pose (five or more; the mirrored start of the negated case has no truth to
    return to): compared up to scale, the bundle adjustment's estimate is no further from the generating truth than the
    disturbed start in rotation, translation direction and map.  Where the observations themselves determine a component less
    well than the start was disturbed - the translation direction from 12 matches: 7e-3 rad against the 5e-3 of the
    disturbance - "no further" cannot hold for a correct estimator, and the bound is three of the estimate's own standard
    deviations (pose_sigmas) instead: max(start, 3 sigma)."""
    pair, r = PAIRS()[k], ref_of(oracle_mod, k)
    u = used(pair)
    e0 = truth_error(pair, np.asarray(pair["pose2"]), np.asarray(pair["points"])[u])
    e1 = truth_error(pair, r["pose"], r["points"][u])
    s_rot, s_dir = pose_sigmas(oracle_mod, r)
    print("rotation, translation direction, map: start", e0, "result", e1, "sigma", (s_rot, s_dir))
    assert e1[0] <= max(e0[0], 3 * s_rot) and e1[1] <= max(e0[1], 3 * s_dir) and e1[2] <= e0[2], (e0, e1, s_rot, s_dir)


def test_mask_layout_is_the_compacted_pair(oracle_mod):
    pair = make_pair(40, "general", seed=21)
    sp = spread_out(pair, 5)
    a, b = ref_init_map(oracle_mod, pair), ref_init_map(oracle_mod, sp)
    assert np.array_equal(a["points"], b["points"][used(sp)]) and np.array_equal(a["pose"], b["pose"])


# ---- the library's own arithmetic on the CPU ---------------------------------------------------------------------------------

def run_im_main(exe, pair, tmp_path):
    """tests/init_map/im_main.cpp on the used matches of `pair` -> the fields of Solver.init_map's dict (stages 3 and 4 by
    finish())"""
    u = used(pair)
    n = int(u.sum())
    w = window_of(pair)
    path = os.path.join(str(tmp_path), "pair.bin")
    with open(path, "wb") as f:
        f.write(np.array([n, w.max_iters, pair.get("max_trials", 0), 0], np.int32).tobytes())
        f.write(np.array(list(w.cam) + [w.huber_delta], np.float64).tobytes())
        f.write(np.asarray(pair["pose2"], np.float64).tobytes())
        for a in (w.obs[0::2], w.obs[1::2], w.points, w.inv_sigma2[0::2], w.inv_sigma2[1::2]):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    r = subprocess.run([exe, path], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = {}
    trials = []
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        if key == "trial":
            trials.append([float(v) for v in vals])
        else:
            got[key] = np.array([float(v) for v in vals])
    tr = np.array(trials).reshape(-1, 5)
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], got["pose"]], np.float64)
    g = finish(pair, poses, got["points"].reshape(-1, 3), got["chi2"])
    g.update(status=0, cost0=float(got["cost0"][0]), cost=float(got["cost"][0]), lam=float(got["lambda"][0]), n_chol_fail=int(got["cholfail"][0]),
             iters_done=int(got["iters"][0]), n_solves=int(got["solves"][0]), last_rejected=int(len(tr) and tr[-1, 4] == 0),
             trace=dict(lam=tr[:, 0], f0=tr[:, 1], f1=tr[:, 2], rho=tr[:, 3], accept=tr[:, 4].astype(int)))
    return g


@pytest.fixture(scope="module")
def im_main():
    subprocess.check_call(["make", "-C", IM_DIR, "-s", "im_main_asan"])
    return os.path.join(IM_DIR, "im_main_asan")


@pytest.mark.parametrize("k", range(len(_SPECS)), ids=[f"{s['scene']}-{s['n_used']}" for s in _SPECS])
def test_the_librarys_arithmetic_against_the_restatement_on_the_cpu(oracle_mod, im_main, tmp_path, k):
    """init_map.h's per-point arithmetic - what k_init_map inlines - summed serially (tests/init_map/im_main.cpp, under
    AddressSanitizer + UndefinedBehaviorSanitizer), held to the oracle as the GPU tests hold the kernel."""
    pair, ref = PAIRS()[k], ref_of(oracle_mod, k)
    w = ref["window"]
    tol = order_noise.tolerances(w, order_noise.spread(oracle_mod, w))
    check(pair, run_im_main(im_main, pair, tmp_path), ref, w, tol, ref["oracle"])


def test_a_failed_factorisation_is_a_rejected_trial_as_in_the_oracle(oracle_mod, im_main, tmp_path):
    """Negative information on the keyframe-2 edges makes the reduced matrix indefinite until lambda has grown past it: the first
    factorisations fail.  The oracle books each as a rejected trial with F1 = DBL_MAX, the estimate untouched, lambda raised;
    the library's loop (the one k_init_map runs) must fail on the same trials, count them and go on as the oracle does."""
    pair = make_pair(20, "general", seed=31)
    pair["inv_sigma2_1"], pair["inv_sigma2_2"] = np.ones(20), -np.ones(20)
    o = ref_init_map(oracle_mod, pair)["oracle"]
    g = run_im_main(im_main, pair, tmp_path)
    big = np.finfo(float).max
    failed = o["trace"]["f1"] == big
    # (order_noise.noise_floor_trial is built for positive costs; here the comparison runs up to the first accepted trial)
    k0 = int(np.flatnonzero(o["trace"]["accept"])[0]) + 1 if o["trace"]["accept"].any() else len(failed)
    print("trials", o["n_solves"], "failed", int(failed.sum()), "compared", k0, "failed among them", int(failed[:k0].sum()))
    assert o["status"] == 0 and failed[0] and failed[:k0].sum() >= 3 and not o["trace"]["accept"][failed].any()
    assert np.array_equal(g["trace"]["f1"][:k0] == big, failed[:k0]) and g["n_chol_fail"] >= failed[:k0].sum()
    assert np.array_equal(g["trace"]["accept"][:k0], o["trace"]["accept"][:k0])
    np.testing.assert_allclose(g["trace"]["lam"][:k0], o["trace"]["lam"][:k0], rtol=order_noise.USUAL_LAM)
    ok = ~failed[:k0]
    np.testing.assert_allclose(g["trace"]["f1"][:k0][ok], o["trace"]["f1"][:k0][ok], rtol=order_noise.USUAL_F1)
    if k0 == len(failed):
        assert g["n_chol_fail"] == failed.sum() and g["n_solves"] == o["n_solves"] and g["iters_done"] == o["iters_done"]
        assert np.array_equal(g["points"][used(pair)], np.asarray(pair["points"]))       # every trial rejected: the estimate is the start


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["init_map_asan", "init_map_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/init_map/init_map_driver.cpp: every refusal of the header with nothing written, n == 0, empty pairs between solved
    ones, the mask layout against the compacted one, pinned against ordinary result memory, and a call between two solves of an
    uploaded window - with the library's host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of
    tests/init_map linked into one program."""
    subprocess.check_call(["make", "-C", IM_DIR, "-s", target])
    r = subprocess.run([os.path.join(IM_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "init_map driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
