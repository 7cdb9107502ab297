"""The HIP path at monocular map scale and far from the world origin.

Every synthetic window and frame of the suite lives within a few metres of the origin, 4 - 30 units deep, on baselines of 0.3
units.  The windows and frames here are the same problems in the world X' = s X + c (movba.synth.similarity,
tests/test_map_scale_cpu.py): s = 0.05 and 1 / 9.5516 (what a map rescaled to median depth 1 looks like), s = 20,
c = (2000, -300, 1500), and s = 0.05 with c = (100, -15, 75).  What that reaches that no other test does:

  a different LM path: at s = 0.05 and 1 / 9.5516 the 30-keyframe window rejects six / seven trials and takes 16 / 17 reduced
  solves where the suite's windows accept ten of ten; lambda_0 comes from the translation / point blocks at s = 0.05;
  H, S and the 6 x 6 pivot blocks whose translation and rotation parts are 1 / s^2 = 400 times further apart: k_band's pivot
  blocks, the PCG's block preconditioner, its fp32 coarse inverse and its 200-iteration hand-over rule, the dense solvers'
  column scaling, the depth reciprocal at depths of 0.2 and of 600;
  R X + t that cancels three to four digits on every projection (FAR, S05FAR).

Every bound is order_noise.tolerances(window, the oracle's spread over 16 edge orders THERE, length_unit=s): the usual 1e-8 rad,
s x 1e-8, s x 1e-6 (a tolerance on a length is a statement about a map of that size), or three times the oracle's own spread
where that is larger - it is not on any window here (test_map_scale_cpu asserts it).  Decisions - accept trace up to the noise
floor, n_solves, outlier flags outside the guard band - are compared exactly; the oracle takes the same ones under all 16
orders (asserted there too).  Each compared quantity is printed as a fraction of its bound.  Measured on the MI355X: local BA
at most 0.015 of a bound on every solver, no PCG hand-over at any scale (22.5 iterations per solve at most).

PoseOptimization keeps the tolerances of the general-position tests with the translation's multiplied by s, except on nine
frames whose translation the ORACLE does not reproduce to them under another order of the matches (far from the origin
t = -R c multiplies the rotation's last digits by 2 500; test_map_scale_cpu.POSE_RECLASSIFIED asserts it frame by frame):
max(usual, 3 x the oracle's spread) there, and the device lands on the oracle's own alternative outcomes (0.333 of the bound
= the spread itself in five of the nine)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, quat_angle

sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth  # noqa: E402

import order_noise  # noqa: E402
import test_map_scale_cpu as M  # noqa: E402
from test_gpu_general_position import SOLVERS, assert_solver_that_ran  # noqa: E402
from test_gpu_marginals import _check as check_marginals  # noqa: E402
from test_gpu_parity import GUARD, _shared_stream_solvers, check_against  # noqa: E402
from test_gpu_pose_batch import KEYS as POSE_KEYS  # noqa: E402
from test_marginals_cpu import rel_block_err  # noqa: E402

pytestmark = pytest.mark.gpu

T_IDS = M.T_IDS
# marginals in the generators' units against the numpy reference: max(1e-7, 10 x the reference's own agreement) = 1e-7.
# Measured on the MI355X: 4.0e-10 at most (`small` at s = 0.05, undamped, point blocks); pose blocks 3.6e-11 at most.
MARG_BOUND = max(1e-7, 10 * M.MARG_REFERENCE_AGREEMENT)
# the base of the metamorphic comparison: a shift alone is the same LM as the unshifted window at the same scale
UNSHIFTED = {"FAR": None, "S05FAR": "S05"}


@pytest.fixture(scope="module")
def solvers(built_lib):
    """SOLVERS' handles.  Its "banded" is the default choice, which gives the 30-keyframe window to the PCG (a band of 9 over 30
    keyframes is estimated slower): that window goes through a handle that forces k_band, so that its pivot blocks see the
    rejecting LM path too."""
    s = {k: built_lib.Solver(**kw) for k, kw in SOLVERS.items()}
    s["banded", "kf30"] = built_lib.Solver(solver=2)
    yield s
    for v in s.values():
        v.close()


def handle(solvers, which, name):
    return solvers.get((which, name), solvers[which])


def fractions(r, o, w, tol):
    """each quantity check_against bounds, as a fraction of its bound"""
    d = order_noise.distances(r, o, w)
    return {k: d[k] / (tol[k][0] if k == "chi2_tol" else tol[k]) for k in d}


def report(label, r, o, w, tol):
    fr = fractions(r, o, w, tol)
    print(f"{label}: {r['n_solves']} solves (band {r['n_band']}, direct {r['n_direct']}, PCG give-ups {r['n_pcg_giveups']}, PCG iterations "
          f"{r['pcg_iters']}); fractions of the bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in fr.items()))
    return fr


def check_against_unshifted(rt, r0, o, w, c, tol, label):
    """metamorphic, as test_gpu_general_position.check_against_ungauged: the solve of the shifted window against the same
    solver's unshifted solve mapped forward; decisions equal, distances within the bounds of the shifted window"""
    assert np.array_equal(rt["trace"]["accept"], r0["trace"]["accept"]) and rt["n_solves"] == r0["n_solves"], label
    mism = rt["outlier"] != r0["outlier"]
    assert (np.abs(r0["chi2"][mism] - w.chi2_gate) <= GUARD).all(), label
    pf, xf = synth.similarity_poses(r0["poses"], 1.0, c), synth.similarity_points(r0["points"], 1.0, c)
    rot = float(quat_angle(rt["poses"][:, :4], pf[:, :4]).max())
    trans = float(np.abs(rt["poses"][:, 4:] - pf[:, 4:]).max())
    point = float(np.abs(rt["points"] - xf).max())
    print(f"{label}: against the unshifted solve mapped forward: rotation {rot / tol['rot']:.3g}, translation {trans / tol['trans']:.3g}, "
          f"points {point / tol['point']:.3g} of the bounds")
    assert rot < tol["rot"] and trans < tol["trans"] and point < tol["point"], label


# ---- local BA on every reduced solver ----------------------------------------------------------------------------------------
# PCG hand-overs to the direct solver (k_pcg_rows would need more than 200 iterations), as measured on the MI355X: none.
PCG_GIVEUPS = {}


def assert_ran(r, which, name, t):
    n = PCG_GIVEUPS.get((name, t), 0) if which == "pcg" else 0
    if n == 0:
        assert_solver_that_ran(r, which)
    else:
        assert r["n_chol_fail"] == 0 and r["n_sync_timeouts"] == 0 and r["n_band"] == 0 and r["n_pcg_giveups"] == n


_unshifted = {}


@pytest.mark.parametrize("which", list(SOLVERS))
@pytest.mark.parametrize("t", T_IDS)
@pytest.mark.parametrize("name", ["stereo", "kf30"])
def test_every_reduced_solver_under_the_five_transforms(solvers, oracle_mod, name, t, which):
    s = handle(solvers, which, name)
    w, o = M.window(name, t), M.oracle_solve(oracle_mod, name, t)
    tol = M.bounds(oracle_mod, name, t)
    r = s.solve(w)
    label = f"{name} under {t} on {which}"
    report(label, r, o, w, tol)
    assert_ran(r, which, name, t)
    check_against(r, o, w, noise_guard=True, **tol)
    if t in UNSHIFTED:
        key = (which, name, UNSHIFTED[t])
        if key not in _unshifted:
            _unshifted[key] = s.solve(M.window(name, UNSHIFTED[t]))
        check_against_unshifted(r, _unshifted[key], o, w, M.TRANSFORMS[t][1], tol, label)


@pytest.mark.parametrize("t", [None] + T_IDS, ids=["none"] + T_IDS)
def test_small_on_the_default_solver_choice(solver, oracle_mod, t):
    w, o = M.window("small", t), M.oracle_solve(oracle_mod, "small", t)
    tol = M.bounds(oracle_mod, "small", t)
    r = solver.solve(w)
    report(f"small under {t}", r, o, w, tol)
    assert r["n_chol_fail"] == 0 and r["n_sync_timeouts"] == 0
    check_against(r, o, w, noise_guard=True, **tol)
    if t in UNSHIFTED:
        check_against_unshifted(r, solver.solve(M.window("small", UNSHIFTED[t])), o, w, M.TRANSFORMS[t][1], tol, f"small under {t}")


@pytest.mark.parametrize("which", list(SOLVERS))
def test_the_rejecting_window_after_one_and_two_iterations(solvers, oracle_mod, which):
    """The pattern of test_large_steps_on_every_reduced_solver on the 30-keyframe window at s = 0.05: compared after one and two
    iterations as well, so that later iterations cannot average an early error away.  Bounds from the oracle's spread of the
    solve cut to as many iterations."""
    s = handle(solvers, which, "kf30")
    w = M.window("kf30", "S05")
    for iters in (1, 2, None):
        r = s.solve(w, max_iters=iters)
        o = M.oracle_solve(oracle_mod, "kf30", "S05", max_iters=iters)
        tol = M.bounds(oracle_mod, "kf30", "S05", max_iters=iters)
        report(f"kf30 under S05 on {which}, max_iters {iters}", r, o, w, tol)
        assert_ran(r, which, "kf30", "S05")
        check_against(r, o, w, noise_guard=True, **tol)
    assert M.rejected_before_the_noise_floor(r) >= 5 and r["n_solves"] >= 15          # the device took the rejecting path itself


# ---- the batched run ------------------------------------------------------------------------------------------------------------
def test_batched_run_gives_the_four_scales_their_solo_bits(built_lib, oracle_mod):
    """as test_gpu_parity.test_batched_run_is_bit_identical_to_solo_runs: ONE movba_lba_run_batch over the 30-keyframe window at
    s = 1, 0.05, 20 and far from the origin - windows that take 10, 16, 10 and 10 reduced solves and leave the batch at
    different trials"""
    ts = [None, "S05", "S20", "FAR"]
    ws = [M.window("kf30", t) for t in ts]
    st, solvers = _shared_stream_solvers(built_lib, len(ws))
    try:
        solo = [s.solve(w) for s, w in zip(solvers, ws)]
        assert len({a["n_solves"] for a in solo}) >= 2
        for s, w in zip(solvers, ws):
            s.upload(w)
        assert built_lib.run_batch(solvers) == 0
        for s, w, a, t in zip(solvers, ws, solo, ts):
            b = s.download()
            for k in ("poses", "points", "chi2", "outlier"):
                assert np.array_equal(a[k], b[k]), (t, k)
            assert np.array_equal(a["trace"]["pcg"], b["trace"]["pcg"]) and np.array_equal(a["trace"]["accept"], b["trace"]["accept"]), t
            assert a["n_solves"] == b["n_solves"] and a["lam"] == b["lam"], t
            check_against(b, M.oracle_solve(oracle_mod, "kf30", t), w, noise_guard=True, **M.bounds(oracle_mod, "kf30", t))
    finally:
        for s in solvers:
            s.close()


# ---- marginals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", M.MARG_TRANSFORMS)
@pytest.mark.parametrize("name", ["small", "stereo"])
def test_marginals_under_scale_and_shift(solver, name, t):
    """test_gpu_marginals' check as it stands (1e-7 per block against the numpy reference at the downloaded estimate), and the
    same after the unit change of test_map_scale_cpu.in_generator_units: the translation part of a pose block is 400 times
    smaller than its rotation part at s = 0.05 and would hide behind it in a relative Frobenius error."""
    s, _ = M.TRANSFORMS[t]
    w = M.window(name, t)
    r = solver.solve(w)
    assert r["status"] == 0
    for d in M.MARG_DAMPINGS:
        mc = solver.marginals(d)
        label = f"{name} under {t}"
        ref = check_marginals(w, r, mc, d, label)
        got_u, ref_u = M.in_generator_units(mc["pose_cov"], mc["point_cov"], s), M.in_generator_units(ref["pose_cov"], ref["point_cov"], s)
        ep, eq = rel_block_err(got_u[0], ref_u[0]), rel_block_err(got_u[1], ref_u[1])
        # the translation part alone: the 3 x 3 upsilon-upsilon corner of every pose block
        et = rel_block_err(np.ascontiguousarray(mc["pose_cov"][:, 3:, 3:]), np.ascontiguousarray(ref["pose_cov"][:, 3:, 3:]))
        print(f"{label}: damping {d:g}: in generator units pose blocks {ep / MARG_BOUND:.3g}, point blocks {eq / MARG_BOUND:.3g}, "
              f"translation corners {et / MARG_BOUND:.3g} of the bound {MARG_BOUND:g}")
        assert ep <= MARG_BOUND and eq <= MARG_BOUND and et <= MARG_BOUND, label




# ---- pose optimisation ------------------------------------------------------------------------------------------------------------
def pose_distance(a, b, s):
    """(largest quaternion component difference, largest translation difference / s)"""
    return float(np.abs(a[:4] - b[:4]).max()), float(np.abs(a[4:] - b[4:]).max()) / s


@pytest.mark.parametrize("t", T_IDS)
def test_pose_optimisation_under_the_five_transforms(solver, oracle_mod, built_lib, t):
    """Tolerances of test_gpu_general_position.test_pose_optimisation_in_the_four_frames (1e-9 on the pose), the translation's
    multiplied by s - except the frames of test_map_scale_cpu.POSE_RECLASSIFIED, whose translation the oracle itself does not
    reproduce to it under another order of the matches: max(usual, 3 x the oracle's spread) there."""
    s, _ = M.TRANSFORMS[t]
    for i, (label, kw, f) in enumerate(M.pose_cases(t)[:3]):
        r = solver.pose_opt(**kw)
        _, o = M.pose_oracle(oracle_mod, built_lib, t, i)
        bq, bt, bc = M.pose_bounds(oracle_mod, built_lib, t, i)
        dq, dt = pose_distance(r["pose"], o["pose"], s)
        print(f"{label} under {t}: quaternion {dq / bq:.3g}, translation {dt / bt:.3g}, chi2 {order_noise.chi2_mixed(r['chi2'], o['chi2']) / bc[0]:.3g} "
              f"of the bounds {bq:.3g} / s x {bt:.3g} / {bc[0]:.3g}; inliers {r['n_inliers']} / {o['n_inliers']}")
        assert r["status"] == 0 and r["n_inliers"] == o["n_inliers"]
        assert dq < bq and dt < bt
        mism = r["outlier"] != o["outlier"]
        assert (np.abs(o["chi2"][mism] - kw["chi2_gate"]) <= GUARD).all()
        np.testing.assert_allclose(r["chi2"], o["chi2"], rtol=bc[0], atol=bc[1])


@pytest.mark.parametrize("t", T_IDS)
def test_pose_hypothesis_stage_under_the_five_transforms(solver, oracle_mod, built_lib, t):
    """test_gpu_general_position.test_pose_hypothesis_stage_in_the_four_frames (55 % outliers, 50 samples, seed 7, start pose 150
    degrees off): P3P on points 0.2 - 1.5 units deep, 80 - 600 units deep, and 2 500 units from the origin.  The winner to 1e-7 /
    s x 1e-7, the final pose to 1e-8 / s x 1e-8 (or by test_map_scale_cpu.POSE_RECLASSIFIED)."""
    s, c = M.TRANSFORMS[t]
    label, kw, f = M.pose_cases(t)[3]
    o_r, o = M.pose_oracle(oracle_mod, built_lib, t, 3)
    bq, bt, _ = M.pose_bounds(oracle_mod, built_lib, t, 3)
    r = solver.pose_opt(**kw)
    wq, wt = pose_distance(r["ransac_pose"], o_r["pose"], s)
    dq, dt = pose_distance(r["pose"], o["pose"], s)
    print(f"hypothesis stage under {t}: winner quaternion {wq / 1e-7:.3g}, translation {wt / 1e-7:.3g} of 1e-7 / s x 1e-7; final pose "
          f"quaternion {dq / bq:.3g}, translation {dt / bt:.3g} of {bq:.3g} / s x {bt:.3g}")
    assert r["status"] == 0 and r["ransac_inliers"] == o_r["n_inliers"] >= 0.9 * (~f["is_outlier"]).sum()
    assert wq < 1e-7 and wt < 1e-7
    assert r["n_inliers"] == o["n_inliers"] and dq < bq and dt < bt
    mism = r["outlier"] != o["outlier"]
    assert (np.abs(o["chi2"][mism] - kw["chi2_gate"]) <= GUARD).all()
    assert ((r["outlier"] == 1) == f["is_outlier"]).mean() > 0.99
    pb = synth.unsimilarity_poses(r["pose"][None], s, c)               # (the generating truth, in the generator's world)
    assert np.abs(pb[0, 4:] - f["truth0"][4:]).max() < 0.03 and quat_angle(pb[:, :4], f["truth0"][None, :4]).max() < 2e-3


def test_pose_batch_gives_the_transformed_frames_their_solo_bits(solver):
    cases = [kw for t in T_IDS for _, kw, _ in M.pose_cases(t)]
    solo = [solver.pose_opt(**kw) for kw in cases]
    out = solver.pose_opt_batch(cases)
    assert len(out) == len(cases) == 20
    for b, s in zip(out, solo):
        assert b["status"] == 0
        for key in POSE_KEYS:
            np.testing.assert_array_equal(b[key], s[key], err_msg=key)
