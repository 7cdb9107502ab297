#!/usr/bin/env python3
"""Whole-call time of movba_triangulate (host clock around the synchronised call, warm, median) for 30 x 2 000 monocular,
30 x 2 000 stereo and 8 sessions x 30 x 2 000 matches, with ordinary and with pinned (movba_host_alloc) result arrays, plus the
same scenes through the single-thread numpy restatement of tests/test_triangulate_cpu.py (context only: it is not the
reference's cv::triangulatePoints loop).

    python scripts/triangulate_time.py [--reps 30] [--out profiles/triangulate_time.json]
    rocprofv3 --kernel-trace --stats ... -- python scripts/triangulate_time.py --reps 20 --no-numpy     # the kernel alone
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


def bytes_of(sc):
    """what the call moves: the packed copy to the device, and the results back"""
    m = sc["matches"]; n = len(m["obs1"])
    h2d = sum(np.asarray(a).nbytes for a in list(sc["views"].values()) + list(m.values())) + \
        np.asarray(sc["pairs"]["pair_view"], np.int32).nbytes + np.asarray(sc["pairs"]["pair_ptr"], np.int32).nbytes
    return int(h2d), 25 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    scenes = {
        "mono_30x2000": synth.make_triangulation(30, 2000, 7101),
        "stereo_30x2000": synth.make_triangulation(30, 2000, 7102, stereo=True),
        "mono_8x30x2000": synth.concat_triangulations([synth.make_triangulation(30, 2000, 7200 + k) for k in range(8)]),
    }
    s = capi.Solver()
    res = {}
    for name, sc in scenes.items():
        row = {}
        for pinned in (False, True):
            d, keep = capi.tri_desc(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
            n = int(keep["pair_ptr"][-1])
            pts = s._pinned((n, 3)) if pinned else np.zeros((n, 3))
            code = s._pinned((n,), np.uint8) if pinned else np.zeros(n, np.uint8)
            r = capi.TriResult()
            r.points = pts.ctypes.data_as(C.POINTER(C.c_double)); r.code = code.ctypes.data_as(C.POINTER(C.c_uint8))
            call = lambda: s._L.movba_triangulate(s._h, C.byref(d), C.byref(r))
            for _ in range(5):
                assert call() == 0
            med, p10, p90 = median_ms(call, args.reps)
            row["pinned_ms" if pinned else "ordinary_ms"] = med
            row["pinned_p10_p90" if pinned else "ordinary_p10_p90"] = (p10, p90)
            row["n_accepted"] = r.n_accepted
        h2d, d2h = bytes_of(sc)
        row.update(n_matches=n, n_pairs=int(len(keep["pair_view"])), h2d_bytes=h2d, result_bytes=d2h)
        if not args.no_numpy:
            from test_triangulate_cpu import triangulate_ref
            t0 = time.perf_counter()
            triangulate_ref(sc["views"], sc["pairs"], sc["matches"], sc["reproj_gate"], sc["far_threshold"])
            row["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        res[name] = row
        print(name, json.dumps(row), flush=True)
    s.close()
    out = dict(reps=args.reps, timing="median of whole calls, host clock around each synchronised call, 5 warm-up calls", scenes=res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
