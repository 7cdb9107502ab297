"""Developer timer of movba_two_view_lo against movba_two_view on the same input (not collected by pytest): median wall time per
call, warm, host clock around the whole call (copy in, launches, synchronisation, copy out), the two calls ALTERNATING so that
both see the same clocks and the same neighbours - for one pair and for 64 pairs of `--matches` matches and `--samples` samples.

    python scripts/time_two_view_lo.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_two_view_lo.py --reps 20
        per-kernel times (k_tv_hyp, k_tv_lo, k_tv_recover, k_tv_check) in DIR's kernel_stats: a run of its own

The clocks are whatever the device runs at under the load (not pinned)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--matches", type=int, default=500)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--lo-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = capi.Solver()
    scenes = ("general", "planar", "forward", "general")
    pairs = [dict(synth.make_two_view(a.matches, 0.7, 0.5, 9000 + k, scene=scenes[k % 4]), ransac_iters=a.samples, ransac_seed=1 + k)
             for k in range(64)]
    out = dict(matches=a.matches, samples=a.samples, reps=a.reps, lo_iters=a.lo_iters)
    for label, batch in (("1_pair", pairs[:1]), ("64_pairs", pairs)):
        n = len(batch)
        descs = (capi.TwoViewDesc * n)(); res = (capi.TwoViewResult * n)(); info = (capi.TwoViewLoInfo * n)()
        keeps = []
        for k, p in enumerate(batch):
            d, r, keep = capi.two_view_desc(p)
            descs[k] = d; res[k] = r; keeps.append(keep)
        ts = dict(plain=[], lo=[])
        for it in range(a.warmup + a.reps):
            for which in ("plain", "lo"):
                t0 = time.perf_counter()
                if which == "plain":
                    rc = s._L.movba_two_view(s._h, descs, res, n)
                else:
                    rc = s._L.movba_two_view_lo(s._h, descs, res, n, a.lo_iters, info)
                t1 = time.perf_counter()
                assert rc == 0
                if it >= a.warmup:
                    ts[which].append((t1 - t0) * 1e3)
        for which in ts:
            out[f"{label}_{which}_ms"] = dict(median=float(np.median(ts[which])), min=float(np.min(ts[which])), p90=float(np.percentile(ts[which], 90)))
        out[f"{label}_ratio"] = out[f"{label}_lo_ms"]["median"] / out[f"{label}_plain_ms"]["median"]
        out[f"{label}_kept"] = [int(info[k].kept) for k in range(min(n, 8))]
        out[f"{label}_steps"] = [int(info[k].steps) for k in range(min(n, 8))]
    s.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
