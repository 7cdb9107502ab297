"""movba_view_points restated in numpy fp64 from the rules of include/movba.h (what the CPU and GPU tests compare against), and
the committed cases: the nine-view parity call, the hand-made items on the gates, the median lists.  Helper module: no tests
here (tests/test_view_points_cpu.py, tests/test_gpu_view_points.py)."""
import numpy as np

FRUSTUM, FUSE, DEPTH = 0, 1, 2
VISIBLE, FUSE_CANDIDATE, DEPTH_ITEM = 1, 2, 3
REJ_BEHIND, REJ_U, REJ_V, REJ_IMAGE, REJ_DIST, REJ_ANGLE = range(16, 22)
DEFAULTS = dict(bf=0.0, bounds=(0.0, 0.0, 0.0, 0.0), log_scale_factor=float(np.log(1.2)), n_levels=8, cos_limit=0.5, q=2)
VALUE_KEYS = ("z", "uv", "dist", "view_cos", "ur", "track_depth")
NEAR = 1e-9         # an item closer than this (relative) to a gate it reaches is not compared by code


def order_key(v):
    """the total order of doubles by bit pattern (csrc/init_map.h: im_order_key) as uint64"""
    u = np.ascontiguousarray(v, np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def key_value(k):
    k = np.asarray(k, np.uint64)
    u = np.where((k >> np.uint64(63)) != 0, k & np.uint64((1 << 63) - 1), ~k)
    return u.view(np.float64)


def median_of(z, q):
    """element (n - 1) // q of the ascending order of z under order_key; -1.0 for an empty list"""
    if len(z) == 0:
        return -1.0
    return float(key_value(np.sort(order_key(z))[(len(z) - 1) // q:][:1])[0])


def rotation(pose):
    q = np.asarray(pose[:4], np.float64)
    x, y, z, w = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _near(a, b):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) <= NEAR * np.maximum(1.0, np.abs(b))


def ref_view(points, view):
    """One view -> dict of per-item arrays (code, z, uv, dist, view_cos, level, ur, track_depth, near), n_accepted, median_depth.
    near: the item lies within NEAR of a gate it reaches (or of a level boundary): its decision is not held to the bit."""
    g = lambda key: view.get(key, DEFAULTS[key])
    idx = np.asarray(view["items"], np.int64).reshape(-1)
    n = len(idx)
    mode = view["mode"]
    P = np.asarray(points["points"], np.float64).reshape(-1, 3)[idx]
    R = rotation(view["pose"])
    t = np.asarray(view["pose"][4:], np.float64)
    nan = np.full(n, np.nan)
    out = dict(code=np.zeros(n, np.uint8), z=nan.copy(), uv=np.full((n, 2), np.nan), dist=nan.copy(), view_cos=nan.copy(),
               level=np.full(n, -1, np.int32), ur=nan.copy(), track_depth=nan.copy(), near=np.zeros(n, bool))
    with np.errstate(all="ignore"):
        z = R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2]
        out["z"] = z
        if mode == DEPTH:
            out["code"][:] = DEPTH_ITEM
            out.update(n_accepted=n, median_depth=median_of(z, g("q")))
            return out
        Pn = np.asarray(points["normals"], np.float64).reshape(-1, 3)[idx]
        dmax = np.asarray(points["max_distance"], np.float64)[idx]
        dmin = np.asarray(points["min_distance"], np.float64)[idx]
        fx, fy, cx, cy = view["cam"]
        x0, x1, y0, y1 = g("bounds")
        code = np.zeros(n, np.uint8)
        near = np.zeros(n, bool)
        live = np.ones(n, bool)

        def gate(reject, rej_code, close):
            nonlocal live
            near[live & close] = True
            code[live & reject] = rej_code
            live = live & ~reject

        gate(z < 0.0, REJ_BEHIND, np.abs(z) <= NEAR)
        x = R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1] + R[0, 2] * P[:, 2] + t[0]
        y = R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1] + R[1, 2] * P[:, 2] + t[1]
        u = fx * x / z + cx
        v = fy * y / z + cy
        out["uv"][live] = np.stack([u, v], 1)[live]
        if mode == FRUSTUM:
            gate((u < x0) | (u > x1), REJ_U, _near(u, x0) | _near(u, x1))
            gate((v < y0) | (v > y1), REJ_V, _near(v, y0) | _near(v, y1))
        else:
            gate(~((u >= x0) & (u < x1) & (v >= y0) & (v < y1)), REJ_IMAGE, _near(u, x0) | _near(u, x1) | _near(v, y0) | _near(v, y1))
        Ow = np.array([-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)])
        po = P - Ow
        dist = np.sqrt(po[:, 0] * po[:, 0] + po[:, 1] * po[:, 1] + po[:, 2] * po[:, 2])
        out["dist"][live] = dist[live]
        gate((dist < 0.8 * dmin) | (dist > 1.2 * dmax), REJ_DIST, _near(dist, 0.8 * dmin) | _near(dist, 1.2 * dmax))
        dot = po[:, 0] * Pn[:, 0] + po[:, 1] * Pn[:, 1] + po[:, 2] * Pn[:, 2]
        if mode == FUSE:
            gate(dot < 0.5 * dist, REJ_ANGLE, _near(dot, 0.5 * dist))
            code[live] = FUSE_CANDIDATE
        else:
            vc = dot / dist
            out["view_cos"][live] = vc[live]
            gate(vc < g("cos_limit"), REJ_ANGLE, _near(vc, g("cos_limit")))
            code[live] = VISIBLE
            s = np.log(dmax / dist) / g("log_scale_factor")
            near[live & (np.abs(s - np.round(s)) <= NEAR)] = True
            s = np.ceil(s)
            nl = g("n_levels")
            lvl = np.where(~(s >= 0.0), 0.0, np.where(s >= nl, nl - 1.0, s))
            out["level"][live] = lvl[live].astype(np.int32)
            out["ur"][live] = (u - g("bf") / z)[live]
            out["track_depth"][live] = np.sqrt(x * x + y * y + z * z)[live]
    out.update(code=code, near=near, n_accepted=int(live.sum()), median_depth=float("nan"))
    return out


def ref_view_points(points, views):
    """The whole call -> the dict Solver.view_points gives, plus `near`."""
    per = [ref_view(points, v) for v in views]
    out = {}
    for key in ("code", "z", "uv", "dist", "view_cos", "level", "ur", "track_depth", "near"):
        shape = (0, 2) if key == "uv" else (0,)
        out[key] = np.concatenate([p[key] for p in per]) if per else np.zeros(shape)
    out["n_accepted"] = np.array([p["n_accepted"] for p in per], np.int32)
    out["median_depth"] = np.array([p["median_depth"] for p in per], np.float64)
    out["view_ptr"] = np.concatenate([[0], np.cumsum([len(p["code"]) for p in per])]).astype(np.int32)
    out["status"] = 0
    return out


def same_bits(a, b):
    """two values equal to the bit (NaN payloads included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(got, ref, label="", median_bits=False):
    """got (Solver.view_points, or anything with its fields) against ref_view_points: codes and levels equal on every item the
    restatement keeps, at most 1 % of the items dropped, values within 1e-12 relative to max(1, |value|) and NaN where the
    restatement has NaN, counts exact (a view with a dropped item: within the number dropped), medians as the values (they
    are selected among z) or, with median_bits - lists whose z is exact - to the bit."""
    keep = ~ref["near"]
    n = len(keep)
    assert got["status"] == 0 and len(got["code"]) == n, label
    dropped = int((~keep).sum())
    print(label, "items", n, "dropped", dropped)
    assert dropped <= 0.01 * n, label
    assert np.array_equal(got["code"][keep], ref["code"][keep]), label
    assert np.array_equal(got["level"][keep], ref["level"][keep]), label
    for key in VALUE_KEYS:
        if key not in got:
            continue
        g, r = got[key][keep], ref[key][keep]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        with np.errstate(invalid="ignore"):
            err = np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))
        err = err[~(g[ok] == r[ok])]            # (equal infinities)
        print(label, key, "max relative error", float(err.max()) if len(err) else 0.0)
        assert (err <= 1e-12).all(), (label, key)
    ptr = ref["view_ptr"]
    for v in range(len(ptr) - 1):
        slack = int((~keep[ptr[v]:ptr[v + 1]]).sum())
        assert abs(int(got["n_accepted"][v]) - int(ref["n_accepted"][v])) <= slack, (label, v)
    gm, rm = np.asarray(got["median_depth"], np.float64), ref["median_depth"]
    if median_bits:
        assert same_bits(gm, rm), label
    else:
        assert np.array_equal(np.isnan(gm), np.isnan(rm)), label
        ok = ~np.isnan(rm)
        assert (np.abs(gm[ok] - rm[ok]) <= 1e-12 * np.maximum(1.0, np.abs(rm[ok]))).all(), label


# ---- the committed cases -------------------------------------------------------------------------------------------------

PARITY_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
PARITY_MODES = (DEPTH, FUSE, FRUSTUM) * 3
_parity = None


def _look_at(centre, target, roll, rng):
    """Tcw (7,) of a camera at `centre` looking at `target`, rolled about its axis, the quaternion not normalised"""
    f = target - centre
    f /= np.linalg.norm(f)
    a = np.cross(f, rng.normal(size=3))
    a /= np.linalg.norm(a)
    b = np.cross(f, a)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * a + s * b, -s * a + c * b, f])            # rows: camera axes in the world
    tr = np.trace(R)
    # (trace > -1 for the rolls used here)
    w = np.sqrt(max(1.0 + tr, 1e-12)) / 2
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return np.concatenate([q * rng.uniform(0.5, 2.0), -R @ centre])


def parity_case():
    """One call of nine views - three of each mode, lists of PARITY_LENGTHS - over a shared table of 1200 points: cameras in
    general position 3 - 6 units from the middle of a cloud 12 units wide, so that points lie behind every camera and outside
    every image; normals that point away from a reference centre near the cameras with enough scatter for the angle gate;
    distance ranges around the distance to that centre, so that the distance gate rejects at both ends and the predicted level
    clamps at both ends.  Points with |z| < 0.1 in any view are not in the table.  -> (points, views), computed once."""
    global _parity
    if _parity is not None:
        return _parity
    rng = np.random.default_rng(20240607)
    views = []
    for k in range(9):
        centre = rng.normal(size=3)
        centre *= rng.uniform(3.0, 6.0) / np.linalg.norm(centre)
        pose = _look_at(centre, rng.uniform(-1.0, 1.0, 3), rng.uniform(-0.6, 0.6), rng)
        views.append(dict(mode=PARITY_MODES[k], pose=pose, cam=(rng.uniform(380, 460), rng.uniform(380, 460), rng.uniform(300, 340), rng.uniform(220, 260)),
                          bf=float(rng.uniform(30, 50)), bounds=(-5.5, 645.25, -4.75, 485.5), log_scale_factor=float(np.log(1.2)), n_levels=8,
                          cos_limit=0.5, q=(1, 2, 3)[k // 3]))
    X = rng.uniform(-6.0, 6.0, (4000, 3))
    ok = np.ones(len(X), bool)
    for v in views:
        z = X @ rotation(v["pose"])[2] + v["pose"][6]
        ok &= np.abs(z) >= 0.1
    X = X[ok][:1200]
    assert len(X) == 1200
    ref_centre = rng.normal(size=3) * 2.0
    d_ref = np.linalg.norm(X - ref_centre, axis=1)
    normals = (X - ref_centre) / d_ref[:, None] + rng.normal(0, 0.6, X.shape)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    points = dict(points=X, normals=normals, max_distance=d_ref * rng.uniform(0.7, 5.0, len(X)), min_distance=d_ref * rng.uniform(0.3, 1.2, len(X)))
    for v, n in zip(views, PARITY_LENGTHS):
        v["items"] = rng.integers(0, len(X), n).astype(np.int32)
    _parity = (points, views)
    return _parity


_parity_ref = None


def parity_ref():
    """ref_view_points of parity_case(), computed once and shared (callers must not change it)"""
    global _parity_ref
    if _parity_ref is None:
        _parity_ref = ref_view_points(*parity_case())
    return _parity_ref


def gate_case():
    """Items exactly on each gate: identity pose, fx = fy = 1, cx = cy = 0, integer-valued coordinates, so that every quantity
    is exact.  Four views over the same table: FRUSTUM and FUSE with log_scale_factor = log 2 and four levels, FRUSTUM with log
    1.05 (the level clamps at both ends far from a boundary), and FRUSTUM at cos_limit 0.25.  bounds [-2, 2] x [-3, 3].
    -> (points, views, want): want[label] = (code in FRUSTUM, code in FUSE, level in FRUSTUM or None)."""
    nan, inf = float("nan"), float("inf")
    rows = [
        # label                          P               Pn              max   min   FRUSTUM          FUSE             level
        ("inside",                       (0, 0, 2),      (0, 0, 1),      2,    1,    VISIBLE,         FUSE_CANDIDATE,  0),
        ("u == maxX",                    (4, 0, 2),      (1, 0, 0),      8,    1,    VISIBLE,         REJ_IMAGE,       None),
        ("u == minX",                    (-4, 0, 2),     (-1, 0, 0),     8,    1,    VISIBLE,         FUSE_CANDIDATE,  None),
        ("v == maxY",                    (0, 6, 2),      (0, 1, 0),      8,    1,    VISIBLE,         REJ_IMAGE,       None),
        ("v == minY",                    (0, -6, 2),     (0, -1, 0),     8,    1,    VISIBLE,         FUSE_CANDIDATE,  None),
        ("u past maxX",                  (5, 0, 2),      (1, 0, 0),      8,    1,    REJ_U,           REJ_IMAGE,       None),
        ("v past minY",                  (0, -7, 2),     (0, -1, 0),     8,    1,    REJ_V,           REJ_IMAGE,       None),
        ("z == 0, u = +inf",             (1, 0, 0),      (1, 0, 0),      8,    0,    REJ_U,           REJ_IMAGE,       None),
        ("z == 0, u = -inf",             (-1, 0, 0),     (1, 0, 0),      8,    0,    REJ_U,           REJ_IMAGE,       None),
        ("z == 0, v = +inf",             (0, 1, 0),      (0, 1, 0),      8,    0,    REJ_V,           REJ_IMAGE,       None),
        ("the camera centre: 0 / 0",     (0, 0, 0),      (0, 0, 1),      8,    0,    VISIBLE,         REJ_IMAGE,       3),
        ("z == -1",                      (0, 0, -1),     (0, 0, -1),     8,    0,    REJ_BEHIND,      REJ_BEHIND,      None),
        ("dist == 0.8 min",              (0, 0, 4),      (0, 0, 1),      5,    5,    VISIBLE,         FUSE_CANDIDATE,  1),
        ("dist below 0.8 min",           (0, 0, 3),      (0, 0, 1),      8,    5,    REJ_DIST,        REJ_DIST,        None),
        ("dist == 1.2 max",              (0, 0, 6),      (0, 0, 1),      5,    1,    VISIBLE,         FUSE_CANDIDATE,  0),
        ("dist above 1.2 max",           (0, 0, 7),      (0, 0, 1),      5,    1,    REJ_DIST,        REJ_DIST,        None),
        ("viewCos == cos_limit",         (0, 0, 2),      (0, 0, 0.5),    2,    1,    VISIBLE,         FUSE_CANDIDATE,  0),
        ("viewCos below cos_limit",      (0, 0, 2),      (0, 0, 0.25),   2,    1,    REJ_ANGLE,       REJ_ANGLE,       None),
        ("ratio 1: level 0",             (0, 0, 4),      (0, 0, 1),      4,    1,    VISIBLE,         FUSE_CANDIDATE,  0),
        ("ratio 8: level 3 of 4",        (0, 0, 1),      (0, 0, 1),      8,    1,    VISIBLE,         FUSE_CANDIDATE,  3),
        ("ratio 64: clamped to 3",       (0, 0, 1),      (0, 0, 1),      64,   1,    VISIBLE,         FUSE_CANDIDATE,  3),
        ("NaN in the point",             (nan, 0, 2),    (0, 0, 1),      8,    1,    VISIBLE,         REJ_IMAGE,       0),
        ("NaN in the normal",            (0, 0, 2),      (nan, 0, 1),    2,    1,    VISIBLE,         FUSE_CANDIDATE,  0),
        ("NaN max_distance",             (0, 0, 2),      (0, 0, 1),      nan,  1,    VISIBLE,         FUSE_CANDIDATE,  0),
        ("NaN min_distance",             (0, 0, 2),      (0, 0, 1),      2,    nan,  VISIBLE,         FUSE_CANDIDATE,  0),
        ("infinite max_distance",        (0, 0, 2),      (0, 0, 1),      inf,  1,    VISIBLE,         FUSE_CANDIDATE,  3),
    ]
    pts = dict(points=np.array([r[1] for r in rows], np.float64), normals=np.array([r[2] for r in rows], np.float64),
               max_distance=np.array([r[3] for r in rows], np.float64), min_distance=np.array([r[4] for r in rows], np.float64))
    base = dict(pose=(0, 0, 0, 1, 0, 0, 0), cam=(1.0, 1.0, 0.0, 0.0), bf=2.0, bounds=(-2.0, 2.0, -3.0, 3.0), n_levels=4, cos_limit=0.5,
                items=np.arange(len(rows), dtype=np.int32))
    views = [dict(base, mode=FRUSTUM, log_scale_factor=float(np.log(2.0))), dict(base, mode=FUSE, log_scale_factor=float(np.log(2.0))),
             dict(base, mode=FRUSTUM, log_scale_factor=float(np.log(1.05))), dict(base, mode=FRUSTUM, log_scale_factor=float(np.log(2.0)), cos_limit=0.25)]
    want = {r[0]: (r[5], r[6], r[7]) for r in rows}
    return pts, views, [r[0] for r in rows], want


MEDIAN_SIZES = (1, 2, 3, 255, 256, 257, 4097)
_median = None


def _depth_view(first, n, q):
    # (t_z = -0 and x = y = -0 in the table: z is the third coordinate to the bit, -0 included)
    return dict(mode=DEPTH, pose=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, -0.0), cam=(1.0, 1.0, 0.0, 0.0), q=q, items=np.arange(first, first + n, dtype=np.int32))


def median_case(big=40000):
    """DEPTH views over a table whose third coordinates are the lists themselves (identity pose): MEDIAN_SIZES x q in (1, 2, 3)
    of mixed-sign depths with duplicates, then the special lists - all equal; duplicates across the wanted rank; +-0 only;
    +-inf among numbers; a NaN among numbers; an empty list - and one list of `big` items.  -> (points, views, lists)."""
    global _median
    if _median is not None and _median[3] == big:
        return _median[:3]
    rng = np.random.default_rng(977)
    inf, nan = float("inf"), float("nan")
    lists, qs = [], []
    for n in MEDIAN_SIZES:
        for q in (1, 2, 3):
            z = np.round(rng.normal(0.0, 20.0, n), 1)            # (one decimal: many duplicates at 4097)
            z[rng.random(n) < 0.05] = 0.0
            z[rng.random(n) < 0.05] = -0.0
            lists.append(z); qs.append(q)
    special = [np.full(300, 7.25), np.concatenate([np.full(100, 1.0), np.full(200, 3.5), np.full(100, 9.0)])[rng.permutation(400)],
               np.array([0.0, -0.0, -0.0, 0.0, -0.0, 0.0, 0.0]), np.array([3.0, -inf, inf, 1.0, inf, -2.0, -inf, -inf]),
               np.array([5.0, nan, 1.0, 2.0]), np.array([nan]), np.array([-4.0, 2.0, inf, nan, 0.5]), np.zeros(0)]
    for z in special:
        for q in (1, 2, 3):
            lists.append(z); qs.append(q)
    lists.append(np.round(rng.uniform(-5.0, 60.0, big), 2)); qs.append(2)
    zs = np.concatenate(lists)
    P = np.full((len(zs), 3), -0.0)
    P[:, 2] = zs
    views, at = [], 0
    for z, q in zip(lists, qs):
        views.append(_depth_view(at, len(z), q))
        at += len(z)
    _median = (dict(points=P), views, lists, big)
    return _median[:3]
