#!/usr/bin/env python3
"""Whole-call time of movba_lba_marginals (host clock around the synchronised call) on cfg2 and cfg3: poses only and poses +
points, next to the same window's movba_lba_solve, plus the numpy reference (tests/test_marginals_cpu.py) on the same window.

    python scripts/marginals_time.py [--reps 50] [--out profiles/marginals_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from movba import capi, synth  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from test_marginals_cpu import marginals_schur
    res = {}
    for name in args.configs.split(","):
        w = synth.cfg(name)
        s = capi.Solver()
        s.prepare(w, pinned=True)
        assert s.solve_prepared(pack=False) == 0
        d = s._prep[0]
        pc = np.zeros((d.n_poses, 6, 6)); qc = np.zeros((d.n_points, 3, 3))
        pp, qp = pc.ctypes.data_as(C.POINTER(C.c_double)), qc.ctypes.data_as(C.POINTER(C.c_double))
        L, h = s._L, s._h
        for _ in range(5):
            assert L.movba_lba_marginals(h, 0.0, pp, qp) == 0
        solve = median_ms(lambda: s.solve_prepared(pack=False), args.reps)
        poses = median_ms(lambda: L.movba_lba_marginals(h, 0.0, pp, None), args.reps)
        both = median_ms(lambda: L.movba_lba_marginals(h, 0.0, pp, qp), args.reps)
        nf = int((np.asarray(w.pose_fixed) == 0).sum())
        row = dict(n_free=nf, n_points=w.n_points, n_edges=w.n_edges, ntile=(6 * nf + 47) // 48,
                   solve_ms=solve[0], marginals_poses_ms=poses[0], marginals_poses_points_ms=both[0],
                   p10_p90=dict(solve=solve[1:], poses=poses[1:], poses_points=both[1:]),
                   ratio_poses_points_to_solve=both[0] / solve[0])
        if not args.no_numpy:
            r = s.download_prepared(pack=True)
            t0 = time.perf_counter()
            marginals_schur(w, r["poses"], r["points"], 0.0)
            row["numpy_reference_ms"] = (time.perf_counter() - t0) * 1e3
        s.close()
        res[name] = row
        print(name, json.dumps(row), flush=True)
    out = dict(reps=args.reps, timing="median of whole calls, host clock around each synchronised call (pinned solve buffers)",
               configs=res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
