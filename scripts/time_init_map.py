"""Developer timer of movba_init_map (not collected by pytest): median wall time per call, warm, host clock around the whole call
(copy in, launch, synchronisation, copy out) for one pair and for 64 pairs of `--matches` used matches - and beside it the same
64 maps through what a caller had before the call existed: 64 handles on one stream, each with the two-keyframe window uploaded
(movba_lba_upload), movba_lba_run_batch, 64 downloads and the median depth and rescaling on the host.  The two routes ALTERNATE,
so that both see the same clocks and the same neighbours.

    python scripts/time_init_map.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_init_map.py --reps 20 --no-handles
        k_init_map's own time in DIR's kernel_stats: a run of its own

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


def make_pair(n, seed):
    """a general scene with a start disturbed as a minimal-sample pose and a linear triangulation are (the cases of
    tests/test_init_map_cpu.py), 2 % gross mismatches"""
    tv = synth.make_two_view(n, inlier_frac=0.98, noise_px=0.05, seed=seed, scene="general")
    rng = np.random.default_rng(1000 + seed)
    R0 = synth._rodrigues(rng.normal(0, 2e-3 / np.sqrt(3), 3)) @ tv["R"]
    t0 = tv["t"] + rng.normal(0, 5e-3 / np.sqrt(3), 3)
    return dict(obs1=tv["obs1"], obs2=tv["obs2"], points=tv["X"] * (1.0 + rng.normal(0, 0.02, (n, 1))),
                pose2=np.concatenate([synth.quat_from_R(R0), t0 / np.linalg.norm(t0)]), cam=tv["cam"])


def window_of(p):
    n = len(p["obs1"])
    return synth.Window(poses=np.array([[0, 0, 0, 1, 0, 0, 0], p["pose2"]], np.float64), pose_fixed=np.array([1, 0], np.uint8),
                        points=np.array(p["points"]), edge_pose=np.tile(np.array([0, 1], np.int32), n),
                        edge_point=np.repeat(np.arange(n, dtype=np.int32), 2), obs=np.stack([p["obs1"], p["obs2"]], 1).reshape(-1, 2),
                        inv_sigma2=np.ones(2 * n), cam=tuple(p["cam"]), max_iters=20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--no-handles", action="store_true", help="movba_init_map alone (the profiler's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pairs = [make_pair(a.matches, 9100 + k) for k in range(64)]
    s = capi.Solver()

    def prepared(batch):
        n = len(batch)
        descs = (capi.InitMapDesc * n)(); res = (capi.InitMapResult * n)()
        keeps = []
        for k, p in enumerate(batch):
            d, r, keep = capi.init_map_desc(p)
            descs[k] = d; res[k] = r
            keeps.append(keep)
        return lambda: s._L.movba_init_map(s._h, descs, res, n, None), res, keeps

    call1, res1, keep1 = prepared(pairs[:1])
    call64, res64, keep64 = prepared(pairs)
    routes = {"init_map_1_pair": call1, "init_map_64_pairs": call64}
    solves = {}
    if not a.no_handles:
        import torch
        st = torch.cuda.Stream(device=0)
        hs = [capi.Solver(device=0, stream=st.cuda_stream) for _ in pairs]
        ws = [window_of(p) for p in pairs]
        for h, w in zip(hs, ws):
            h.prepare(w, flags=0, max_iters=20)

        def through_handles():
            for h in hs:
                h.upload_prepared()
            rc = capi.run_batch(hs)
            for k, h in enumerate(hs):
                h.download_prepared()
                r, o = h._prep[2], h._prep[3]
                z = np.sort(o["points"][:, 2])
                med = z[(len(z) - 1) // 2]
                if not med < 0 and len(z) >= 50:
                    o["points"] *= 1.0 / med; o["poses"][1, 4:] *= 1.0 / med
                solves[k] = r.n_solves
            return rc
        routes["64_handles_run_batch"] = through_handles
    for f in routes.values():
        for _ in range(a.warmup):
            assert f() == 0
    times = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, f in routes.items():
            t0 = time.perf_counter()
            rc = f()
            times[k].append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, (k, rc)
    out = dict(matches=a.matches, reps=a.reps, lm_trials_64=int(sum(r.n_solves for r in res64)), lm_trials_1=int(res1[0].n_solves),
               outcomes_ok=int(sum(r.outcome == capi.IM_OK for r in res64)))
    if solves:
        out["lm_trials_64_handles"] = int(sum(solves.values()))
    for k, t in times.items():
        out[k] = dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), p90_ms=float(np.percentile(t, 90)))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
