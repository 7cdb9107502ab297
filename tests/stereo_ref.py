"""movba_stereo_points restated in numpy, independently of mov-slam_amd/csrc/stereo_points.h, and the cases the CPU and GPU tests
share.  The restatement follows the reference's text: Frame::ComputeStereoMatches behind its LK call (Frame.cc:306-353) - the
gates point by point in np.float32, every operation one numpy operation on float32 operands and so one rounding, the pairs (int
distance, index) SORTED, the median read at size / 2, the sorted pairs walked from the back -, Frame::UnprojectStereo (:836-851)
and the walks of Tracking::StereoInitialization (Tracking.cc:532-547) and CreateNewKeyFrame / UpdateLastFrame (:1022-1098,
:828-887) with their own nPoints counter and break.  The library selects the median by radix and computes the list's length in
closed form; nothing of that is used here.  sel_point is numpy's own matrix product in float64: it is compared within a derived
bound, everything else exactly."""
import functools
import json
import os
import subprocess

import numpy as np

F = np.float32
NONE, ALL, CLOSE = 0, 1, 2
OK, REJ_STATUS, REJ_ROW, REJ_DISPARITY, REJ_FAR = 1, 16, 17, 18, 19
POINT_KEYS = ("u_right", "depth", "code")
FRAME_KEYS = ("n_stereo", "median_dist", "th_dist")
EXACT_KEYS = POINT_KEYS + FRAME_KEYS + ("sel_ptr", "sel_src", "sel_new", "sel_cam")
KEYS = EXACT_KEYS + ("sel_point",)
CAM = (F(420.5), F(418.25), F(31.5), F(23.75))


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def rotation(q):
    """Rcw of a quaternion (x y z w), normalised first"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def centre(pose):
    """(Rwc, Ow) of Tcw = (qx qy qz qw tx ty tz); None: the identity"""
    if pose is None:
        return np.eye(3), np.zeros(3)
    R = rotation(pose[:4])
    return R.T, -R.T @ np.asarray(pose[4:], np.float64)


def gates(fr, max_row_diff, min_disparity):
    """Frame.cc:306-338 -> (u_right, depth, code, [(int dist, i)])"""
    pt, nxt, status = np.asarray(fr["pt"], F).reshape(-1, 2), np.asarray(fr["next_pt"], F).reshape(-1, 2), np.asarray(fr["pt_status"]).reshape(-1)
    n = len(pt)
    ur, depth, code, pairs = np.full(n, -1, F), np.full(n, -1, F), np.zeros(n, np.uint8), []
    cols, rows, bf, minD, maxD = F(fr["cols"]), F(fr["rows"]), F(fr["bf"]), F(min_disparity), F(fr["max_disparity"])
    with np.errstate(all="ignore"):
        for i in range(n):
            lx, ly, rx, ry = pt[i, 0], pt[i, 1], nxt[i, 0], nxt[i, 1]
            if status[i] == 0 or rx < 0 or ry < 0 or rx >= cols or ry >= rows:
                code[i] = REJ_STATUS
                continue
            if np.abs(ry - ly) > F(max_row_diff):
                code[i] = REJ_ROW
                continue
            best = rx
            disparity = lx - best
            if not (disparity >= minD and disparity < maxD):
                code[i] = REJ_DISPARITY
                continue
            if disparity <= 0:
                disparity = F(0.01)
                best = F(np.float64(lx) - 0.01)
            depth[i] = bf / disparity
            ur[i] = best
            dx, dy = lx - rx, ly - ry
            dist = F(np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)))
            pairs.append((int(dist), i))
            code[i] = OK
    return ur, depth, code, pairs


def ref_frame(fr, max_row_diff=4.0, min_disparity=0.0, max_point=100):
    ur, depth, code, pairs = gates(fr, max_row_diff, min_disparity)
    median, th = -1, F(0)
    if pairs:
        pairs.sort()
        median = pairs[len(pairs) // 2][0]
        th = F(1.5) * F(1.4) * F(median)
        for dist, i in reversed(pairs):
            if F(dist) < th:
                break
            ur[i] = depth[i] = -1
            code[i] = REJ_FAR
    n = len(ur)
    has = np.asarray(fr["has_point"]).reshape(-1) if fr.get("has_point") is not None else np.zeros(n, np.uint8)
    select = fr.get("select", NONE)
    src, new = [], []
    if select == ALL:
        for i in range(n):
            if depth[i] > 0:
                src.append(i)
                new.append(0 if has[i] else 1)
    elif select == CLOSE:
        order = sorted((depth[i], i) for i in range(n) if depth[i] > 0)
        n_points = 0
        for z, i in order:
            src.append(i)
            new.append(0 if has[i] else 1)
            n_points += 1
            if z > F(fr["th_depth"]) and n_points > max_point:
                break
    un = np.asarray(fr["pt_un"] if fr.get("pt_un") is not None else fr["pt"], F).reshape(-1, 2)
    fx, fy, cx, cy = (F(v) for v in fr["cam"])
    invfx, invfy = F(1) / fx, F(1) / fy
    cam = np.zeros((len(src), 3), F)
    for k, i in enumerate(src):
        z = depth[i]
        cam[k] = ((un[i, 0] - cx) * z * invfx, (un[i, 1] - cy) * z * invfy, z)
    Rwc, Ow = centre(fr.get("pose"))
    point = cam.astype(np.float64) @ Rwc.T + Ow if len(src) else np.zeros((0, 3))
    # the derived bound of sel_point per component k: 16 x 2^-53 x (|x| + |y| + |z| + |Ow_k|) - three products, three additions and
    # the rounding of R's entries
    bound = 16 * 2.0 ** -53 * (np.abs(cam.astype(np.float64)).sum(axis=1, keepdims=True) + np.abs(Ow)) if len(src) else np.zeros((0, 3))
    return dict(sel_bound=bound, u_right=ur, depth=depth, code=code, n_stereo=int((depth > 0).sum()), median_dist=median, th_dist=th,
                sel_src=np.array(src, np.int32), sel_new=np.array(new, np.uint8), sel_cam=cam, sel_point=point)


def ref_stereo(frames, max_row_diff=4.0, min_disparity=0.0, max_point=100):
    """-> the dict of Solver.stereo_points (without status)"""
    parts = [ref_frame(fr, max_row_diff, min_disparity, max_point) for fr in frames]
    n = [len(p["code"]) for p in parts]
    n_pt, nf = sum(n), len(frames)
    out = dict(pt_ptr=np.concatenate([[0], np.cumsum(n)]).astype(np.int32),
               sel_ptr=np.concatenate([[0], np.cumsum([len(p["sel_src"]) for p in parts])]).astype(np.int32),
               sel_src=np.full(n_pt, -1, np.int32), sel_new=np.zeros(n_pt, np.uint8), sel_cam=np.full((n_pt, 3), np.nan, F),
               sel_point=np.full((n_pt, 3), np.nan), sel_bound=np.zeros((n_pt, 3)))
    for key, dtype in (("u_right", F), ("depth", F), ("code", np.uint8)):
        out[key] = np.concatenate([p[key] for p in parts]).astype(dtype) if parts else np.zeros(0, dtype)
    for key, dtype in (("n_stereo", np.int32), ("median_dist", np.int32), ("th_dist", F)):
        out[key] = np.array([p[key] for p in parts], dtype).reshape(nf)
    total = int(out["sel_ptr"][-1])
    for key in ("sel_src", "sel_new", "sel_cam", "sel_point", "sel_bound"):
        if total:
            out[key][:total] = np.concatenate([p[key] for p in parts])
    return out


def _same(a, b):
    if a.dtype == F:
        return a.view(np.uint32) == b.view(np.uint32)
    return a == b


def compare(got, want, label="", point="bound"):
    """exact, bit for bit (NaN padding included), but sel_point: "bound" - within the restatement's sel_bound; "exact" - equal; None -
    left out"""
    for key in EXACT_KEYS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, key, a.shape, b.shape, a.dtype, b.dtype)
        same = _same(a, b)
        assert same.all(), (label, key, np.argwhere(~same)[:5].tolist(), a[~same][:5], b[~same][:5])
    if point is None:
        return
    a, b = np.asarray(got["sel_point"]), np.asarray(want["sel_point"])
    total = int(want["sel_ptr"][-1])
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.isnan(a[total:]).all(), (label, "sel_point")
    if point == "exact":
        assert (a[:total] == b[:total]).all(), (label, "sel_point, exact", np.argwhere(a[:total] != b[:total])[:5].tolist())
    else:
        with np.errstate(invalid="ignore"):
            ok = (np.abs(a[:total] - b[:total]) <= want["sel_bound"][:total]) | ((a[:total] == b[:total]) & np.isinf(b[:total]))
        assert ok.all(), (label, "sel_point", np.argwhere(~ok)[:5].tolist(), a[:total][~ok][:5], b[:total][~ok][:5])


def frame_part(res, f):
    """frame f of a result as the result of a call with that frame alone"""
    a, b = int(res["pt_ptr"][f]), int(res["pt_ptr"][f + 1])
    s0, s1 = int(res["sel_ptr"][f]), int(res["sel_ptr"][f + 1])
    out = {key: res[key][a:b] for key in POINT_KEYS}
    out.update({key: res[key][f:f + 1] for key in FRAME_KEYS})
    out.update(pt_ptr=np.array([0, b - a], np.int32), sel_ptr=np.array([0, s1 - s0], np.int32))
    for key, fill in (("sel_src", -1), ("sel_new", 0), ("sel_cam", np.nan), ("sel_point", np.nan), ("sel_bound", 0)):
        if key not in res:
            continue
        full = np.full((b - a,) + res[key].shape[1:], fill, res[key].dtype)
        full[:s1 - s0] = res[key][s0:s1]
        out[key] = full
    return out


def digest(res):
    """a few integers that pin a result"""
    total = int(res["sel_ptr"][-1])
    return dict(u_right=int((np.ascontiguousarray(res["u_right"]).view(np.uint32).astype(np.int64) >> 8).sum()),
                depth=int((np.ascontiguousarray(res["depth"]).view(np.uint32).astype(np.int64) >> 8).sum()),
                codes=tuple(int((res["code"] == c).sum()) for c in (OK, REJ_STATUS, REJ_ROW, REJ_DISPARITY, REJ_FAR)),
                n_stereo=int(res["n_stereo"].sum()), median=int(res["median_dist"].sum()), selected=total,
                sel_src=int(res["sel_src"][:total].astype(np.int64).sum()), sel_new=int(res["sel_new"].sum()),
                sel_cam=int((np.ascontiguousarray(res["sel_cam"][:total]).view(np.uint32).astype(np.int64) >> 8).sum()))


# ---- the library's own walk on the CPU -----------------------------------------------------------------------------------------

def run_stereo_main(exe, frames, tmp_path, max_row_diff=4.0, min_disparity=0.0, max_point=100, env=None, reps=None):
    """tests/stereo_points/stereo_main.cpp (a build of it: exe) on one call, written to tmp_path in the program's format -> the fields
    of Solver.stereo_points' dict; env: variables added to the program's (a sanitizer's options); reps: the walk is timed that often
    and the dict carries host_walk = dict(median_ms, min_ms)"""
    from movba import capi
    d, keep = capi.stereo_desc(frames, max_row_diff, min_disparity, max_point)
    nf, n = len(frames), len(keep["pt"])
    flags = (1 if keep["pt_un"] is not None else 0) | (2 if keep["poses"] is not None else 0) | (4 if keep["has_point"] is not None else 0)
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([nf, n, max_point, flags], np.int32).tobytes())
        f.write(np.array([max_row_diff, min_disparity], np.float32).tobytes())
        for key in ("rows", "cols", "select", "pt_ptr", "bf", "max_disparity", "th_depth", "cam", "pt", "next_pt", "pt_status", "pt_un", "poses", "has_point"):
            if keep[key] is not None:
                f.write(keep[key].tobytes())
    r = subprocess.run([exe, src, dst] + ([str(reps)] if reps else []), env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stereo_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    at = 0

    def take(count, dtype, width=1):
        nonlocal at
        a = np.frombuffer(blob, dtype, count * width, at)
        at += a.nbytes
        return a.reshape(count, width) if width > 1 else a

    out = dict(u_right=take(n, np.float32), depth=take(n, np.float32), code=take(n, np.uint8), n_stereo=take(nf, np.int32), median_dist=take(nf, np.int32),
               th_dist=take(nf, np.float32), sel_ptr=take(nf + 1, np.int32), sel_src=take(n, np.int32), sel_new=take(n, np.uint8),
               sel_cam=take(n, np.float32, 3), sel_point=take(n, np.float64, 3), pt_ptr=keep["pt_ptr"])
    assert at == len(blob)
    if reps:
        out["host_walk"] = json.loads(r.stdout.splitlines()[-1])
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def make_frame(pt, next_pt, status=None, rows=48, cols=64, bf=40.0, max_disparity=32.0, th_depth=6.0, select=NONE, cam=CAM, **more):
    pt, next_pt = np.asarray(pt, F).reshape(-1, 2), np.asarray(next_pt, F).reshape(-1, 2)
    status = np.ones(len(pt), np.uint8) if status is None else np.asarray(status, np.uint8).reshape(-1)
    return dict(pt=pt, next_pt=next_pt, pt_status=status, rows=rows, cols=cols, bf=F(bf), max_disparity=F(max_disparity), th_depth=F(th_depth),
                select=select, cam=np.asarray(cam, F), **more)


def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


# gates_case: (label, L, R, status, the code the gates give); rows 48, cols 64, max_disparity 32
GATE_POINTS = (
    ("next.x -0.0 passes", (20.0, 10.0), (-0.0, 10.0), 1, OK),
    ("next.x just below 0", (20.0, 10.0), (down(0.0), 10.0), 1, REJ_STATUS),
    ("next.y just below 0", (20.0, 1.0), (15.0, down(0.0)), 1, REJ_STATUS),
    ("next.x cols - 1", (63.5, 10.0), (63.0, 10.0), 1, OK),
    ("next.x cols", (64.0, 10.0), (64.0, 10.0), 1, REJ_STATUS),
    ("next.x just below cols", (64.0, 10.0), (down(64.0), 10.0), 1, OK),
    ("next.y rows", (30.0, 46.0), (25.0, 48.0), 1, REJ_STATUS),
    ("next.y just below rows", (30.0, 46.0), (25.0, down(48.0)), 1, OK),
    ("pt_status 0", (30.0, 20.0), (25.0, 20.0), 0, REJ_STATUS),
    ("pt_status 0 with a NaN", (30.0, 20.0), (np.nan, np.inf), 0, REJ_STATUS),
    ("pt_status 255", (30.0, 20.0), (25.0, 20.0), 255, OK),
    ("row difference 4.0", (30.0, 10.0), (25.0, 14.0), 1, OK),
    ("row difference -4.0", (30.0, 14.0), (25.0, 10.0), 1, OK),
    ("row difference just above 4.0", (30.0, 0.0), (25.0, up(4.0)), 1, REJ_ROW),
    ("row difference just below -4.0", (30.0, up(4.0)), (25.0, 0.0), 1, REJ_ROW),
    ("disparity 0: the 0.01 branch", (10.3, 12.0), (10.3, 12.0), 1, OK),
    ("disparity 0 at a large x", (63.7, 12.0), (63.7, 13.0), 1, OK),
    ("disparity just below 0", (10.0, 12.0), (up(10.0), 12.0), 1, REJ_DISPARITY),
    ("disparity just above 0", (10.0, 12.0), (down(10.0), 12.0), 1, OK),
    ("disparity max_disparity", (40.0, 12.0), (8.0, 12.0), 1, REJ_DISPARITY),
    ("disparity just below max_disparity", (40.0, 12.0), (8.0 + 2.0 ** -19, 12.0), 1, OK),
    ("distance 0.99999994", (down(1.0), 30.0), (0.0, 30.0), 1, OK),
    ("distance 1.0", (21.0, 30.0), (20.0, 30.0), 1, OK),
    ("distance just below 2.0", (down(2.0), 30.0), (0.0, 30.0), 1, OK),
    ("distance 2.0", (22.0, 30.0), (20.0, 30.0), 1, OK),
    ("distance 5 from 3 and 4", (23.0, 30.0), (20.0, 34.0), 1, OK),
)


@functools.lru_cache(None)
def gates_case():
    """every gate at its boundary in one frame, and the same points in a second frame behind 40 points at distance 1 that hold
    the median down, so that the far ones are pruned there"""
    pt, nxt, st = [p[1] for p in GATE_POINTS], [p[2] for p in GATE_POINTS], [p[3] for p in GATE_POINTS]
    more = [(30.0 + 0.25 * k, 20.0) for k in range(40)]
    return [make_frame(pt, nxt, st, select=ALL),
            make_frame(pt + more, nxt + [(x - 1.5, y) for x, y in more], st + [1] * 40, select=CLOSE, has_point=np.arange(len(pt) + 40) % 3 == 0)]


def _line(dists, x0=40.0):
    """points whose int distances are `dists` (disparity dist + 0.5), all accepted"""
    pt = [(x0 + 0.01 * k, 5.0 + (k % 30)) for k in range(len(dists))]
    return pt, [(x - (dv + 0.5), y) for (x, y), dv in zip(pt, dists)]


def exact_threshold():
    """the smallest median m > 1 whose thDist is an integer in fp32 -> (m, thDist)"""
    for m in range(2, 4000):
        th = F(1.5) * F(1.4) * F(m)
        if float(th) == int(th) and int(th) + 0.5 < 31:
            return m, int(th)
    raise AssertionError("no such median")


@functools.lru_cache(None)
def median_case():
    """1 candidate; 2 (the upper median); an odd and an even count; median 0; (float)dist == thDist; points but no candidate; no
    points.  MEDIAN_WANT: the frames' (median_dist, n_stereo)"""
    m, th = exact_threshold()
    frames = []
    for dists in ([3], [1, 3], [2, 9, 4, 1, 3], [2, 9, 4, 1, 3, 5], [0, 0, 0, 7, 2], [m] * 5 + [th, th - 1, 1, 1]):
        frames.append(make_frame(*_line(dists), select=ALL))
    pt, nxt = _line([1, 2, 3])
    frames.append(make_frame(pt, nxt, [0, 0, 0], select=ALL))
    frames.append(make_frame(np.zeros((0, 2)), np.zeros((0, 2)), select=CLOSE))
    return frames


def walk_frame(n_cand, n_close, seed, select=CLOSE, has=None, extra=7, **more):
    """n_cand candidates at int distances 5 .. 9 - none pruned: thDist >= 10.5 -, depths ascending against a shuffled index,
    n_close of them at or below th_depth; `extra` points the gates refuse in between"""
    rng = np.random.default_rng(seed)
    disparity = (F(9.9) - F(0.004) * np.arange(n_cand, dtype=F)).astype(F)          # descending: depth ascending
    assert n_cand == 0 or disparity[-1] > 5
    depth = F(40.0) / disparity
    n = n_cand + extra
    slot = rng.permutation(n)
    pt = np.stack([rng.uniform(30, 60, n), rng.uniform(2, 45, n)], axis=1).astype(F)
    nxt = pt.copy()
    status = np.ones(n, np.uint8)
    for k in range(n_cand):
        nxt[slot[k], 0] = pt[slot[k], 0] - disparity[k]
    for k in range(n_cand, n):
        nxt[slot[k]] = (pt[slot[k], 0] - 3, pt[slot[k], 1] + 9) if k % 2 else pt[slot[k]]
        status[slot[k]] = k % 2
    th_depth = 1.0 if n_close == 0 or n_cand == 0 else (float(depth[n_close - 1]) + float(depth[min(n_close, n_cand - 1)])) / 2 if n_close < n_cand else 100.0
    if has is not None:
        more["has_point"] = (rng.uniform(size=n) < has).astype(np.uint8)
    return make_frame(pt, nxt, status, th_depth=th_depth, select=select, **more)


WALK = ((99, 0), (100, 0), (101, 0), (102, 0), (200, 0), (200, 100), (200, 101), (200, 150), (150, 150))
WALK_LENGTHS = (99, 100, 101, 101, 101, 101, 102, 151, 150)


@functools.lru_cache(None)
def walk_case():
    """the walk's lengths (max_point 100), equal depths, has_point mixed and absent, ALL, CLOSE and NONE in one call"""
    frames = [walk_frame(n, c, 100 + k, has=0.4 if k % 2 else None) for k, (n, c) in enumerate(WALK)]
    # equal depths: 12 points at one disparity, in two groups
    pt = np.array([(50.0, 3.0 + k) for k in range(12)], F)
    nxt = pt - np.array([[6.0 if k % 2 else 8.0, 0.0] for k in range(12)], F)
    frames.append(make_frame(pt, nxt, th_depth=100.0, select=CLOSE, has_point=np.arange(12) % 4 == 1))
    frames.append(walk_frame(130, 20, 300, select=ALL, has=0.5))
    frames.append(walk_frame(130, 20, 301, select=NONE))
    return frames


def random_frame(n, seed, select, pose=None, has=0.3, un=False):
    """n points of a plausible stereo frame: disparities of 0.4 .. 30 pixels, a row noise that sometimes passes 4, lost tracks,
    tracks that left the image; about a tenth far off in distance"""
    rng = np.random.default_rng(seed)
    pt = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1).astype(F)
    disparity = np.where(rng.uniform(size=n) < 0.1, rng.uniform(30, 70, n), rng.uniform(0.4, 30, n))
    nxt = (pt - np.stack([disparity, rng.normal(0, 1.6, n)], axis=1)).astype(F)
    status = (rng.uniform(size=n) < 0.9).astype(np.uint8)
    more = dict(has_point=(rng.uniform(size=n) < has).astype(np.uint8)) if has is not None else {}
    if un:
        more["pt_un"] = (pt + rng.normal(0, 0.5, (n, 2))).astype(F)
    if pose is not None:
        more["pose"] = np.asarray(pose, np.float64)
    return make_frame(pt, nxt, status, rows=480, cols=640, bf=F(38.7), max_disparity=F(80.0), th_depth=F(3.2), select=select,
                      cam=(F(458.6), F(457.3), F(367.2), F(248.4)), **more)


POSE_NEAR = (0.1, -0.2, 0.05, 0.97, 0.3, -0.1, 0.2)
POSE_FAR = (0.31, 0.42, -0.17, 0.83, 41234.5, -8765.25, 1203.125)
COUNTS = (0, 1, 63, 64, 65, 1025, 4097, 16384)


@functools.lru_cache(None)
def counts_case():
    """0 .. 16 384 points per frame, each count as CLOSE and the large ones as ALL too; poses near and far and none"""
    frames = [random_frame(n, 500 + k, CLOSE, pose=(POSE_NEAR, POSE_FAR, None)[k % 3]) for k, n in enumerate(COUNTS)]
    frames += [random_frame(n, 600 + k, ALL, pose=POSE_FAR, un=True) for k, n in enumerate((65, 1025, 4097))]
    return frames


@functools.lru_cache(None)
def counts_nopose_case():
    """no frame has a pose: poses is NULL, sel_point == (double)sel_cam"""
    return [random_frame(n, 700 + k, (CLOSE, ALL)[k % 2], has=None) for k, n in enumerate((65, 1025, 300))]


N_FRAMES = 1024
FRAMES_ALONE = (0, 63, 64, 65, 511, 1023)


@functools.lru_cache(None)
def frames_case():
    """1 024 tiny frames, 0 .. 3 points, with runs of empty ones"""
    rng = np.random.default_rng(77)
    frames = []
    for f in range(N_FRAMES):
        n = int(rng.integers(0, 4))
        if f < 3 or 66 <= f < 76 or 126 <= f < 131 or f == N_FRAMES - 1:
            n = 0
        if f in FRAMES_ALONE[1:5]:
            n = 2
        fr = random_frame(n, 1000 + f, (NONE, ALL, CLOSE)[f % 3], pose=POSE_NEAR if f % 2 else None, has=0.3)
        fr["max_disparity"] = F(31.0)
        frames.append(fr)
    return frames


def _cached(case, **params):
    @functools.lru_cache(None)
    def ref():
        return ref_stereo(case(), **params)
    return ref


gates_ref, median_ref, walk_ref, counts_ref, counts_nopose_ref, frames_ref = (_cached(c) for c in (gates_case, median_case, walk_case, counts_case,
                                                                                                 counts_nopose_case, frames_case))
CASES = dict(gates=(gates_case, gates_ref), median=(median_case, median_ref), walk=(walk_case, walk_ref), counts=(counts_case, counts_ref),
             counts_nopose=(counts_nopose_case, counts_nopose_ref), frames=(frames_case, frames_ref))

# what the restatement gave when the cases were written: digest(counts_ref()) and digest(walk_ref())
PINNED = dict(counts={'u_right': 164896554784, 'depth': 160649682509, 'codes': (21212, 3437, 297, 0, 1940), 'n_stereo': 21212, 'median': 182, 'selected': 14343, 'sel_src': 74462504, 'sel_new': 10034, 'sel_cam': 307799838603},
              walk={'u_right': 7993121203, 'depth': 7833627522, 'codes': (1624, 47, 30, 0, 0), 'n_stereo': 1624, 'median': 107, 'selected': 1148, 'sel_src': 91016, 'sel_new': 888, 'sel_cam': 19504122345})
