"""Developer timer of movba_view_points (not collected by pytest): median wall time per call, warm, host clock around the whole
call (checks, chunk table, packing, copy in, two launches, synchronisation, copy out) on descriptors and result buffers built
once, for the three shapes DESIGN.md quotes: one FRUSTUM view of 20 000 items (one session's frame over its local map), 64
such views (64 sessions in one call), and 30 DEPTH views of 2 000 items (the median depths in front of one keyframe's
triangulation).  Each shape twice: every per-item array asked for in ordinary memory (staged and copied out), and in
movba_host_alloc memory (written by the kernels themselves).

    python scripts/time_view_points.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_view_points.py --reps 20 --shape depth_30x2000
        k_vp_items' and k_vp_views' own times for one shape in DIR's kernel_stats: a run of its own

The clocks are whatever the device runs at under the load (not pinned)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import capi  # noqa: E402


def make_call(n_views, n_items, mode, n_points, seed):
    """a cloud 4 - 30 units ahead of cameras near the origin, normals towards the origin, every list drawn from the table"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-12, 12, n_points), rng.uniform(-9, 9, n_points), rng.uniform(4, 30, n_points)], 1)
    d = np.linalg.norm(X, axis=1)
    normals = X / d[:, None] + rng.normal(0, 0.4, X.shape)
    points = dict(points=X, normals=normals / np.linalg.norm(normals, axis=1, keepdims=True), max_distance=d * rng.uniform(0.8, 4.0, n_points),
                  min_distance=d * rng.uniform(0.2, 1.1, n_points))
    views = []
    for _ in range(n_views):
        q = np.concatenate([rng.normal(0, 0.05, 3), [1.0]])
        views.append(dict(mode=mode, pose=np.concatenate([q, rng.normal(0, 0.3, 3)]), cam=(458.0, 457.0, 367.0, 248.0), bf=47.9,
                          bounds=(0.0, 752.0, 0.0, 480.0), items=rng.integers(0, n_points, n_items).astype(np.int32)))
    return points, views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default=None, help="one of the shapes only (the profiler's runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = capi.Solver()
    shapes = (("frustum_1x20000", 1, 20000, capi.VIEW_FRUSTUM, 20000), ("frustum_64x20000", 64, 20000, capi.VIEW_FRUSTUM, 20000),
              ("depth_30x2000", 30, 2000, capi.VIEW_DEPTH, 20000))
    out = dict(reps=a.reps)
    for name, nv, ni, mode, npnt in shapes:
        if a.shape not in (None, name):
            continue
        points, views = make_call(nv, ni, mode, npnt, 5100 + nv)
        d, keep = capi.view_desc(points, views)
        for where, alloc in (("ordinary", np.zeros), ("pinned", s._pinned)):
            r, res = capi.view_result(nv * ni, nv, alloc)
            t = []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                rc = s._L.movba_view_points(s._h, C.byref(d), C.byref(r))
                t.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            t = np.array(t[a.warmup:])
            out[f"{name}_{where}"] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p90_ms=float(np.percentile(t, 90)),
                                          accepted=int(res["n_accepted"].sum()), items=nv * ni)
            print(name, where, out[f"{name}_{where}"])
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
