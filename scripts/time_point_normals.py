"""Developer timer of movba_lba_point_normals and movba_point_normals (not collected by pytest) on the headline window (50 + 10
keyframes x 20 000 map points, synth.cfg("cfg3")): median wall time per call, warm, host clock around the whole call (checks,
packing, copy in, two launches, synchronisation: every call ends in one) on descriptors and result buffers built once.

    lba_point_normals   the solved window resident on the device, the downloaded outlier flags, results in movba_host_alloc memory
    point_normals       the same estimate and the same lists as arrays, results in movba_host_alloc memory and in ordinary memory
    host loops          the same arithmetic on the host, for scale: a plain interpreter loop over the observation lists (what a
                        caller without this call does per point; interpreter speed, not the C++ adapter's), and the same sums
                        vectorised in numpy (np.add.at over the edges)

The traffic the calls imply is counted from the shapes and printed beside the times, with the time that traffic would take at
the device's 8 TB/s peak.

    python scripts/time_point_normals.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_point_normals.py --reps 20
        k_pn_centres' and k_pn_points' own times in DIR's kernel_stats: a run of its own

The clocks are whatever the device runs at under the load (not pinned)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import capi, synth  # noqa: E402

PEAK_BYTES_PER_S = 8e12
SCALE = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)]))


def centres(poses):
    q = poses[:, :4] / np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    return -np.einsum("vji,vj->vi", R, poses[:, 4:])


def python_loop(points, Ow, lists, ref_pose, ref_level):
    """the normal update as a caller without the call writes it: per point, a walk over its observers"""
    P, O = points.tolist(), Ow.tolist()
    scale, top = SCALE.tolist(), float(SCALE[-1])
    out = []
    for p, obs in enumerate(lists):
        if not obs:
            out.append(None)
            continue
        X = P[p]
        ax = ay = az = 0.0
        for v in obs:
            c = O[v]
            dx, dy, dz = X[0] - c[0], X[1] - c[1], X[2] - c[2]
            ln = math.sqrt(dx * dx + dy * dy + dz * dz)
            ax += dx / ln; ay += dy / ln; az += dz / ln
        n = float(len(obs))
        c = O[ref_pose[p]]
        dx, dy, dz = X[0] - c[0], X[1] - c[1], X[2] - c[2]
        mx = math.sqrt(dx * dx + dy * dy + dz * dz) * scale[ref_level[p]]
        out.append((ax / n, ay / n, az / n, mx, mx / top))
    return out


def numpy_host(points, Ow, edge_point, edge_pose, keep, ref_pose, ref_level):
    d = points[edge_point[keep]] - Ow[edge_pose[keep]]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    acc = np.zeros_like(points)
    np.add.at(acc, edge_point[keep], d)
    n = np.bincount(edge_point[keep], minlength=len(points)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = acc / n[:, None]
    mx = np.linalg.norm(points - Ow[ref_pose], axis=1) * SCALE[ref_level]
    return normals, mx, mx / SCALE[-1]


def timed(fn, warmup, reps):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t[warmup:])
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p90_ms=float(np.percentile(t, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--window", default="cfg3", help="a synth.cfg name (rehearsals: small)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    w = synth.cfg(a.window)
    NP, P, E = w.n_poses, w.n_points, w.n_edges
    s = capi.Solver()
    res = s.solve(w)
    assert res["status"] == 0
    outlier = np.ascontiguousarray(res["outlier"], np.uint8)
    keep = outlier == 0
    lists = [[] for _ in range(P)]
    for e in np.flatnonzero(keep):
        lists[int(w.edge_point[e])].append(int(w.edge_pose[e]))
    rng = np.random.default_rng(1)
    ref_pose = np.array([l[0] if l else 0 for l in lists], np.int32)
    ref_level = rng.integers(0, 8, P).astype(np.int32)
    n_obs = int(keep.sum())
    out = dict(window=a.window, n_poses=NP, n_points=P, n_edges=E, n_obs=n_obs, reps=a.reps)

    # bytes each call moves: across the bus (inputs in; results out, written into pinned memory by the kernel) and on the device
    # (what the kernels read there: the estimate, the lists - edges already grouped, so no permutation - the flags, the per-point
    # entries; the centres are written once and re-read from cache)
    out["lba_bytes"] = dict(bus_in=8 * P + 8 * 8 + E, bus_out=40 * P, device=56 * NP + 24 * NP + 24 * P + 4 * (P + 1) + 4 * E + E + 8 * P)
    out["array_bytes"] = dict(bus_in=56 * NP + 24 * P + 4 * (P + 1) + 4 * n_obs + 8 * P + 64, bus_out=40 * P,
                              device=56 * NP + 24 * NP + 24 * P + 4 * (P + 1) + 4 * n_obs + 8 * P)
    for key in ("lba_bytes", "array_bytes"):
        b = out[key]
        b["total"] = b["bus_in"] + b["bus_out"] + b["device"]
        b["at_peak_us"] = b["total"] / PEAK_BYTES_PER_S * 1e6

    _i, _d, _u = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    r, buf = capi.normals_result(P, s._pinned)

    def lba():
        rc = s._L.movba_lba_point_normals(s._h, ref_pose.ctypes.data_as(_i), ref_level.ctypes.data_as(_i), SCALE.ctypes.data_as(_d), 8,
                                          outlier.ctypes.data_as(_u), r.normals, r.max_distance, r.min_distance)
        assert rc == 0
    out["lba_point_normals_pinned"] = timed(lba, a.warmup, a.reps)
    first = {k: v.copy() for k, v in buf.items()}

    d, kept = capi.normals_desc(res["points"], res["poses"], lists, ref_pose, ref_level, SCALE)
    for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
        r2, buf2 = capi.normals_result(P, alloc)

        def arr():
            assert s._L.movba_point_normals(s._h, C.byref(d), C.byref(r2)) == 0
        out[f"point_normals_{where}"] = timed(arr, a.warmup, a.reps)
        for k in first:         # (the resident call gives the array call's bits)
            assert np.array_equal(first[k], buf2[k], equal_nan=True), k
    s.close()

    Ow = centres(res["poses"])
    ref_list, lvl_list = ref_pose.tolist(), ref_level.tolist()
    out["host_python_loop"] = timed(lambda: python_loop(res["points"], Ow, lists, ref_list, lvl_list), 1, a.host_reps)
    out["host_numpy"] = timed(lambda: numpy_host(res["points"], Ow, w.edge_point, w.edge_pose, keep, ref_pose, ref_level), 1, max(a.host_reps, 5))
    hn = numpy_host(res["points"], Ow, w.edge_point, w.edge_pose, keep, ref_pose, ref_level)
    ok = ~np.isnan(first["max_distance"])
    assert np.abs(hn[0][ok] - first["normals"][ok]).max() < 1e-9 and np.abs(hn[1][ok] - first["max_distance"][ok]).max() < 1e-9
    for k, v in out.items():
        print(k, v)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
