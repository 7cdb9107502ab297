"""How far the ORACLE moves under the edge orders the reference itself produces, in every quantity the parity suite compares,
and the tolerances that follow from it.  A helper module (tests and tests/dev/fuzz_parity.py import it; pytest collects nothing
here).

The reference adds a map point's edges in the iteration order of a std::map keyed by KeyFrame POINTERS
(MapPoint::GetObservations(), src/Optimizer.cc:629-700), which differs from run to run: every within-point order is the
reference's arithmetic, and no solver can be held closer to ONE of those orders than they are to each other.
conftest.oracle_order_noise measures that for the poses and points; spread() measures it for the lambda trace, the cost trace
and the per-edge chi2 as well, over the SAME seeded permutations, and tolerances() turns the record into check_against's
keyword arguments: max(usual, factor * spread) per quantity, nothing picked."""
import copy
import hashlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import quat_angle

GUARD = 1e-6                                              # |chi2 - gate| inside which an outlier flag may differ
MODULE_TOL = dict(rot=1e-8, trans=1e-8, point=1e-6)       # test_gpu_parity's ROT_TOL / TRANS_TOL / POINT_TOL
WEAK_TOL = dict(rot=1e-6, trans=1e-6, point=1e-4)         # SURVEY 8(d)'s float32-map tolerance: see test_weakly_constrained_windows
DEGENERATE_TOL = dict(rot=1e-3, trans=1e-3, point=1e-2)   # a free keyframe with fewer than three observations has no unique pose
USUAL_LAM = 1e-7
USUAL_F1 = 1e-6                                           # check_against's value under noise_guard
USUAL_CHI2 = (1e-6, 1e-7)                                 # (rtol, atol): atol = rtol / 10
WORKERS = 8

Spread = namedtuple("Spread", "rot trans point lam f1 chi2 same_decisions first4 n")


def noise_floor_trial(o):
    """First trial whose accept / reject decision the oracle takes on rounding noise: |F0 - F1| <= 1e-9 F0 (the robust cost
    is a sum over all edges; a solve that has converged to machine precision keeps running, g2o has no convergence test, and
    the sign of F0 - F1 is then arbitrary).  Decisions from there on are a guard band, like |chi2 - 5| <= 1e-6 for the flags."""
    f0, f1 = o["trace"]["f0"], o["trace"]["f1"]
    k = np.flatnonzero((np.abs(f0 - f1) <= 1e-9 * np.abs(f0)) | (f0 <= 1e-18 * f0[0]))     # (or a cost at the absolute rounding floor)
    return int(k[0]) if len(k) else len(f0)


def within_point_permutation(w, t):
    """conftest.oracle_order_noise's t-th edge order: still grouped by point, shuffled inside a group."""
    pm = np.random.default_rng(7919 + t).permutation(w.n_edges)
    return pm[np.argsort(w.edge_point[pm], kind="stable")]


def permuted(w, pm):
    """The window with edge i := w's edge pm[i]."""
    w2 = copy.copy(w)
    w2.edge_pose, w2.edge_point, w2.obs, w2.inv_sigma2 = w.edge_pose[pm], w.edge_point[pm], w.obs[pm], w.inv_sigma2[pm]
    if getattr(w, "obs_right", None) is not None: w2.obs_right = w.obs_right[pm]
    return w2


def unpermute(a, pm):
    """Per-edge output of a solve of permuted(w, pm) (it comes back in THAT window's edge order) -> w's edge order."""
    inv = np.empty_like(pm)
    inv[pm] = np.arange(len(pm))
    return a[inv]


def chi2_mixed(c, ref):
    """max over edges of |c - ref| / (0.1 + |ref|), edges with a non-finite chi2 on either side left out: the smallest s
    with which np.testing.assert_allclose(c, ref, rtol=s, atol=s / 10) holds - the suite's usual (1e-6, 1e-7) has that ratio."""
    fin = np.isfinite(c) & np.isfinite(ref)
    return float((np.abs(c[fin] - ref[fin]) / (0.1 + np.abs(ref[fin]))).max()) if fin.any() else 0.0


def _compare(o, o2, pm, gate):
    """One permuted solve against the caller-order solve -> (rot, trans, point, lam, f1, chi2, same decisions)."""
    rot = float(quat_angle(o2["poses"][:, :4], o["poses"][:, :4]).max())
    trans = float(np.abs(o2["poses"][:, 4:] - o["poses"][:, 4:]).max())
    point = float(np.abs(o2["points"] - o["points"]).max()) if len(o["points"]) else 0.0
    k = min(noise_floor_trial(o), noise_floor_trial(o2), len(o["trace"]["lam"]), len(o2["trace"]["lam"]))
    tr, tr2 = o["trace"], o2["trace"]
    rel = lambda a, ref: float((np.abs(a[:k] - ref[:k]) / np.abs(ref[:k])).max()) if k else 0.0
    lam, f1 = rel(tr2["lam"], tr["lam"]), rel(tr2["f1"], tr["f1"])
    chi2 = chi2_mixed(unpermute(o2["chi2"], pm), o["chi2"])
    mism = unpermute(o2["outlier"], pm) != o["outlier"]
    same = bool(np.array_equal(tr2["accept"][:k], tr["accept"][:k]) and o2["n_solves"] == o["n_solves"]
                and (np.abs(o["chi2"][mism] - gate) <= GUARD).all())
    return rot, trans, point, lam, f1, chi2, same


def _digest(w):
    """The window's content (everything oracle.solve reads): the cache key, so that a window built twice from the same
    make_window arguments - once per solver variant of a parametrised test - pays for its permuted solves once."""
    h = hashlib.sha1()
    for name in ("poses", "pose_fixed", "points", "edge_pose", "edge_point", "obs", "inv_sigma2", "obs_right", "cam_kf", "bf_kf"):
        a = getattr(w, name, None)
        h.update(name.encode() + (b"-" if a is None else np.ascontiguousarray(a).tobytes()))
    h.update(repr((tuple(w.cam), w.huber_delta, w.chi2_gate, w.max_iters, getattr(w, "bf", None))).encode())
    return h.hexdigest()


def distances(r, o, w):
    """How far solve r is from the oracle's o in the quantities check_against bounds (traces up to o's noise floor):
    -> dict(rot, trans, point, lam_rtol, f1_rtol, chi2_tol), keyed like tolerances()' result."""
    k = min(noise_floor_trial(o), len(r["trace"]["lam"]))
    rel = lambda a, ref: float((np.abs(a[:k] - ref[:k]) / np.abs(ref[:k])).max()) if k else 0.0
    return dict(rot=float(quat_angle(r["poses"][:, :4], o["poses"][:, :4]).max()), trans=float(np.abs(r["poses"][:, 4:] - o["poses"][:, 4:]).max()),
                point=float(np.abs(r["points"] - o["points"]).max()) if len(o["points"]) else 0.0,
                lam_rtol=rel(r["trace"]["lam"], o["trace"]["lam"]), f1_rtol=rel(r["trace"]["f1"], o["trace"]["f1"]),
                chi2_tol=chi2_mixed(r["chi2"], o["chi2"]))


_cache = {}


def spread(oracle_mod, w, n=16, workers=WORKERS, cache=True):
    """The oracle's own movement under n within-point edge permutations (those of conftest.oracle_order_noise), each permuted
    solve against the caller-order solve -> Spread:
      rot [rad], trans [m], point [m]   as conftest.oracle_order_noise computes them
      lam, f1                           largest relative difference of the lambda / F1 trace over the trials before the earlier
                                        of the two solves' noise floors
      chi2                              chi2_mixed of the un-permuted per-edge chi2
      same_decisions                    in EVERY permutation: accept trace equal up to the noise floor, n_solves equal, every
                                        outlier flag that differs inside |chi2 - gate| <= 1e-6
      first4                            (rot, trans, point) over the first four permutations only: conftest.oracle_order_noise(n=4)
    The permuted solves run on a thread pool: the serial oracle releases the GIL through ctypes and keeps no file-scope state,
    so the bits are those of a serial run (tests/test_order_noise_cpu.py holds that)."""
    key = (_digest(w), n)
    if cache and key in _cache:
        return _cache[key]
    o = oracle_mod.solve(w)                                 # (also loads the library before any thread asks for it)
    pms = [within_point_permutation(w, t) for t in range(n)]
    ws = [permuted(w, pm) for pm in pms]
    if workers > 1:
        with ThreadPoolExecutor(workers) as ex:
            sols = list(ex.map(oracle_mod.solve, ws))
    else:
        sols = [oracle_mod.solve(x) for x in ws]
    rows = [_compare(o, o2, pm, w.chi2_gate) for o2, pm in zip(sols, pms)]
    mx = lambda rs, j: max([r[j] for r in rs], default=0.0)
    sp = Spread(*(mx(rows, j) for j in range(6)), same_decisions=all(r[6] for r in rows),
                first4=tuple(mx(rows[:4], j) for j in range(3)), n=n)
    if cache:
        _cache[key] = sp
    return sp


def usual(w):
    """The suite's pose / point tolerances by the sweep's classes: the minimum observation count of a free keyframe."""
    per_kf = np.bincount(w.edge_pose, minlength=w.n_poses)[w.pose_fixed == 0]
    least = per_kf.min() if len(per_kf) else 0
    return dict(DEGENERATE_TOL if least < 3 else WEAK_TOL if least < 12 else MODULE_TOL)


def tolerances(w, sp, factor=3, length_unit=1.0):
    """check_against's keyword arguments for window w with measured spread sp: max(usual, factor * spread) per quantity.
    A factor at all, because a maximum over a finite sample underestimates the reach of the distribution and because the GPU
    differs from the oracle by more than within-point order (other reduction trees in the Schur pass, another reduced solver);
    3 is the factor the pose bounds have had since they were first measured.  It is not a knob for making a case pass.
    length_unit: the size of w's map in units of the generators' (synth.similarity's s).  The usual translation and point
    tolerances are statements about a map of the generators' size and are multiplied by it; rotation, lambda, F1 and chi2 have
    no length in them and stay."""
    u = usual(w)
    s = factor * sp.chi2
    return dict(rot=max(u["rot"], factor * sp.rot), trans=max(length_unit * u["trans"], factor * sp.trans),
                point=max(length_unit * u["point"], factor * sp.point),
                lam_rtol=max(USUAL_LAM, factor * sp.lam), f1_rtol=max(USUAL_F1, factor * sp.f1),
                chi2_tol=USUAL_CHI2 if s <= USUAL_CHI2[0] else (s, s / 10))
