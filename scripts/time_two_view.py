"""Developer timer of movba_two_view (not collected by pytest): median wall time per call of 1 pair x 500 matches x 256 samples
and of 64 such pairs, warm, host clock around the whole call (copy in, three launches, synchronisation, copy out).

    python scripts/time_two_view.py                      -> profiles/two_view_time.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_two_view.py --reps 20 --no-json
        per-kernel times (k_tv_hyp, k_tv_recover, k_tv_check) in DIR's kernel_stats: a run of its own, no counters with it

The clocks are whatever the device runs at under the load (not pinned); the figure is the median after `--warmup` calls."""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--matches", type=int, default=500)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    s = capi.Solver()
    scenes = ("general", "planar", "forward", "general")
    pairs = [dict(synth.make_two_view(a.matches, 0.7, 0.5, 9000 + k, scene=scenes[k % 4]), ransac_iters=a.samples, ransac_seed=1 + k)
             for k in range(64)]
    out = dict(matches=a.matches, samples=a.samples, reps=a.reps)
    for label, batch in (("1_pair", pairs[:1]), ("64_pairs", pairs)):
        for pinned in (False, True):
            descs = (capi.TwoViewDesc * len(batch))(); res = (capi.TwoViewResult * len(batch))()
            keeps = []
            for k, p in enumerate(batch):
                d, r, keep = capi.two_view_desc(p, s._pinned if pinned else np.zeros)
                descs[k] = d; res[k] = r; keeps.append(keep)
            ts = []
            for it in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                rc = s._L.movba_two_view(s._h, descs, res, len(batch))
                t1 = time.perf_counter()
                assert rc == 0
                if it >= a.warmup:
                    ts.append((t1 - t0) * 1e3)
            key = label + ("_pinned" if pinned else "")
            out[key + "_ms"] = dict(median=float(np.median(ts)), min=float(np.min(ts)), p90=float(np.percentile(ts, 90)))
            out[key + "_samples_used"] = [int(res[k].samples_used) for k in range(min(len(batch), 8))]
            out[key + "_outcomes"] = [int(res[k].outcome) for k in range(min(len(batch), 8))]
    s.close()
    print(json.dumps(out))
    if not a.no_json:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "two_view_time.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
