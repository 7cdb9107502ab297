"""movba_point_normals restated from the rules of include/movba.h (what the CPU and GPU tests compare against) - numpy fp64 for
the centres, a plain Python loop over every list for the sequential sum - and the committed cases: the parity call, the exact
case, the windows' caller-order lists.  Helper module: no tests here (tests/test_point_normals_cpu.py,
tests/test_gpu_point_normals.py)."""
import math

import numpy as np

from movba import synth

N_LEVELS = 8
SCALE_12 = synth.level_scale_factors(N_LEVELS, 1.2, np.float64)      # mvScaleFactors: 1, 1.2, 1.2 * 1.2, ... (in double here)
SCALE_POW2 = 2.0 ** np.arange(N_LEVELS)
PARITY_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 300)
PARITY_VIEWS = 300


def rotation(pose):
    q = np.asarray(pose[:4], np.float64)
    x, y, z, w = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def centre(pose):
    """Ow = -Rcw^T tcw, term by term as the header writes it"""
    R, t = rotation(pose), np.asarray(pose[4:], np.float64)
    return np.array([-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)])


def ref_point_normals(points, views, lists, ref_view, ref_level, scale_factors):
    """-> dict(normals (N, 3), max_distance, min_distance (N,), terms: per point the list of |d / len| of its observers)"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    Ow = np.array([centre(v) for v in np.asarray(views, np.float64).reshape(-1, 7)]).reshape(-1, 3)
    scale = [float(s) for s in scale_factors]
    n_pts = len(points)
    out = dict(normals=np.full((n_pts, 3), np.nan), max_distance=np.full(n_pts, np.nan), min_distance=np.full(n_pts, np.nan), terms=[])
    with np.errstate(all="ignore"):
        for p in range(n_pts):
            P = [float(c) for c in points[p]]
            acc, n, terms = [0.0, 0.0, 0.0], 0, []
            for v in lists[p]:
                O = Ow[int(v)]
                d = [P[0] - float(O[0]), P[1] - float(O[1]), P[2] - float(O[2])]
                length = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                u = [float(np.float64(c) / np.float64(length)) for c in d]      # (numpy's division: 0 / 0 is NaN, not an exception)
                acc = [acc[0] + u[0], acc[1] + u[1], acc[2] + u[2]]
                terms.append(math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) if length > 0 else float("nan"))
                n += 1
            out["terms"].append(terms)
            if n == 0:
                continue
            out["normals"][p] = [c / float(n) for c in acc]
            O = Ow[int(ref_view[p])]
            d = [P[0] - float(O[0]), P[1] - float(O[1]), P[2] - float(O[2])]
            dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            out["max_distance"][p] = dist * scale[int(ref_level[p])]
            out["min_distance"][p] = out["max_distance"][p] / scale[-1]
    return out


KEYS = ("normals", "max_distance", "min_distance")


def same_bits(a, b):
    """equal bit for bit; a NaN equals any NaN (IEEE 754 leaves the sign and payload of a generated NaN to the implementation)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def compare(got, ref, label, rtol=1e-12):
    """values within rtol relative to max(1, |value|); NaN exactly where the restatement has it; every figure printed first"""
    for key in KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape, (label, key)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key, "NaN pattern")
        ok = ~np.isnan(r)
        err = float((np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))).max()) if ok.any() else 0.0
        print(label, key, "max relative error", err)
        assert err <= rtol, (label, key, err)


# ---- the parity call ------------------------------------------------------------------------------------------------------

_parity = {}


def parity_case():
    """300 views at general-position poses with |t| <= 10 (quaternions not normalised), 1000 points, every one at least 0.5 from
    every centre; lists of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 300 observers in turn, drawn without repetition in random
    order; ref_level cycling through 0 .. 7; ref_view anywhere among the views (in the list or not), -1 for every second point
    with an empty list.  -> dict(points, views, lists, ref_view, ref_level, scale_factors); computed once, not to be changed."""
    if "case" not in _parity:
        rng = np.random.default_rng(20250611)
        q = rng.normal(size=(PARITY_VIEWS, 4)) * rng.uniform(0.5, 2.0, size=(PARITY_VIEWS, 1))
        t = rng.normal(size=(PARITY_VIEWS, 3))
        t *= (rng.uniform(0.5, 10.0, size=PARITY_VIEWS) / np.linalg.norm(t, axis=1))[:, None]
        views = np.concatenate([q, t], 1)
        Ow = np.array([centre(v) for v in views])
        cand = rng.uniform(-12.0, 12.0, size=(3000, 3))
        far = np.linalg.norm(cand[:, None, :] - Ow[None, :, :], axis=2).min(axis=1) >= 0.5
        points = cand[far][:1000]
        assert len(points) == 1000
        lists, ref_view = [], np.zeros(1000, np.int32)
        for p in range(1000):
            n = PARITY_LENGTHS[p % len(PARITY_LENGTHS)]
            lists.append(rng.permutation(PARITY_VIEWS)[:n].astype(np.int32))
            ref_view[p] = rng.integers(PARITY_VIEWS)
            if n == 0 and (p // len(PARITY_LENGTHS)) % 2:
                ref_view[p] = -1
        ref_level = ((np.arange(1000) // 3) % N_LEVELS).astype(np.int32)
        _parity["case"] = dict(points=points, views=views, lists=lists, ref_view=ref_view, ref_level=ref_level, scale_factors=SCALE_12)
    return _parity["case"]


def parity_ref():
    if "ref" not in _parity:
        _parity["ref"] = ref_point_normals(**parity_case())
    return _parity["ref"]


def subset(case, idx):
    """the call over the points idx of a case, in that order"""
    idx = [int(i) for i in idx]
    return dict(case, points=case["points"][idx], lists=[case["lists"][i] for i in idx], ref_view=case["ref_view"][idx],
                ref_level=case["ref_level"][idx])


# ---- the exact case -------------------------------------------------------------------------------------------------------

TRIPLES = ((1, 2, 2), (2, 3, 6), (4, 4, 7), (2, 6, 9))      # lengths 3, 7, 9, 11


def exact_case(scale_factors=SCALE_12, n_points=40):
    """Identity rotations (one quaternion in four not normalised: (0, 0, 0, 2)), integer translations and integer points whose
    differences to their observers' centres are signed permutations of the 3-D Pythagorean triples, times 1, 2 or 4: squares,
    sums, square roots and the centre itself are exact, every division, every add of the sum, the division by n and the two
    scalings are one correctly rounded IEEE operation each, so numpy and the device have no freedom.  Every point has views of
    its own, lists of 1 .. 9 observers, and a reference view that is in its list or (every third point) a further one.  Point 5
    lies in the centre of its third observer and is seen from there by its reference; point 6 lies in an observer's centre and
    has another reference."""
    rng = np.random.default_rng(77)
    views, points, lists, ref_view = [], [], [], []
    for p in range(n_points):
        P = rng.integers(-50, 51, size=3).astype(np.float64)
        n = 1 + p % 9
        mine = []
        for k in range(n + 1):          # (the last one is the further reference view)
            tri = np.array(TRIPLES[rng.integers(len(TRIPLES))], np.float64)[rng.permutation(3)]
            d = tri * rng.choice([-1.0, 1.0], size=3) * float(2 ** rng.integers(3))
            if p in (5, 6) and k == 2:
                d = np.zeros(3)
            Ow = P - d
            mine.append(len(views))
            views.append([0.0, 0.0, 0.0, 2.0 if len(views) % 4 == 1 else 1.0] + list(-Ow))     # (Rcw = I: tcw = -Ow)
        points.append(P)
        lists.append(np.array(mine[:n], np.int32))
        ref_view.append(mine[n] if p % 3 == 2 else mine[int(rng.integers(n))])
    ref_view[5] = lists[5][2]
    ref_view[6] = lists[6][0]
    n_levels = len(scale_factors)
    ref_level = (np.arange(n_points) % n_levels).astype(np.int32)
    return dict(points=np.array(points), views=np.array(views), lists=lists, ref_view=np.array(ref_view, np.int32), ref_level=ref_level,
                scale_factors=np.asarray(scale_factors, np.float64))


# ---- a window's lists -----------------------------------------------------------------------------------------------------

def window_lists(w, outlier=None):
    """the observers of every map point of a window: its edges' keyframes in caller order, without the flagged edges"""
    lists = [[] for _ in range(w.n_points)]
    for e in range(w.n_edges):
        if outlier is None or not outlier[e]:
            lists[int(w.edge_point[e])].append(int(w.edge_pose[e]))
    return lists


def window_refs(w, seed=5):
    """a reference keyframe (the first observer in caller order; any keyframe for a point without edges) and an octave per
    map point"""
    rng = np.random.default_rng(seed)
    lists = window_lists(w)
    ref_pose = np.array([l[0] if l else int(rng.integers(w.n_poses)) for l in lists], np.int32)
    return ref_pose, rng.integers(0, N_LEVELS, size=w.n_points).astype(np.int32)
