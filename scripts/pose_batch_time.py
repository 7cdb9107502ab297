"""Frames per second of movba_pose_opt_batch against the same frames as sequential movba_pose_opt calls on one handle.

cfg1 frames (synth.make_frame: 500 matches, one seed per frame) in batches of N in {1, 8, 64, 256}, for the LM alone and for
the full pipeline (50 samples, confidence 0.95, LO 10).  Host clock around calls that end in the library's own
synchronisation, after warm-up; the median of the repeats.  One JSON line per (pipeline, N) on stdout and in --out.

  python scripts/pose_batch_time.py [--out profiles/x.json] [--reps 15]
  python scripts/pose_batch_time.py --trace       # a few calls of each kind only, for rocprofv3 --kernel-trace --stats
  python scripts/pose_batch_time.py --solo-only   # solo cfg1 calls only (A/B of libraries through MOVBA_LIB)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import capi, synth  # noqa: E402

FULL = dict(ransac_iters=50, confidence=0.95, lo_iters=10)


def frames(n, full):
    out = []
    for k in range(n):
        f = synth.make_frame(n=500, seed=9000 + k)
        kw = dict(Xw=f["Xw"], obs=f["obs"], pose0=f["pose0"], cam=f["cam"], huber_delta=5.0, chi2_gate=25.0)
        if full:
            kw.update(FULL, ransac_seed=1 + k)
        out.append(kw)
    return out


def median_s(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--solo-only", action="store_true")
    a = ap.parse_args()
    s = capi.Solver(device=0)
    rows = []
    if a.solo_only or a.trace:
        f = frames(1, False)[0]
        for _ in range(3):
            s.pose_opt(**f)
        t = median_s(lambda: s.pose_opt(**f), 200)
        rows.append(dict(what="solo cfg1 LM", ms_per_call=round(t * 1e3, 4)))
        if a.trace:
            for full in (False, True):
                fr = frames(64, full)
                for _ in range(5):
                    s.pose_opt_batch(fr)
                for f in fr[:8]:
                    s.pose_opt(**f)
    else:
        for full in (False, True):
            for n in (1, 8, 64, 256):
                fr = frames(n, full)
                reps = a.reps if n <= 64 else max(5, a.reps // 3)
                tb = median_s(lambda: s.pose_opt_batch(fr), reps)
                ts = median_s(lambda: [s.pose_opt(**f) for f in fr], reps)
                rows.append(dict(pipeline="full (50 samples, conf 0.95, LO 10)" if full else "LM only (4 x 10)", n=n,
                                 batch_ms=round(tb * 1e3, 4), batch_frames_per_s=round(n / tb, 1),
                                 sequential_ms=round(ts * 1e3, 4), sequential_frames_per_s=round(n / ts, 1),
                                 speedup=round(ts / tb, 2)))
    s.close()
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
