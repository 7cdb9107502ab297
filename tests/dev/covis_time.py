"""Developer timer of movba_covisibility (not collected by pytest) at the workload's own shape: a map of 500 keyframes on a path
whose points are each seen by a run of consecutive keyframes, about 5.5 observers per point, and queries of 2 000 points each - a
keyframe's own points, so most of a query's observations fall on the same handful of neighbours, which is what the kernel's LDS
atomics contend on.

    one query            one keyframe's UpdateConnections
    64 queries           64 keyframes in one call
    whole_map            obs_ptr / obs_view hold the lists of every point of the map, as a caller passes them that keeps one
                         flattened copy for all its calls
    own_points           they hold the lists of the points the call's queries name and nothing else, renumbered

Per shape: median wall time per call, warm, host clock around the whole call (checks, packing, copy in, one launch,
synchronisation) on descriptors and result buffers built once, results in movba_host_alloc memory and in ordinary memory, 30
entries handed out per query; and the same loop as a single-thread C++ std::map restatement (tests/dev/covis_map_loop.cpp, built
here with g++ -O2), whose results are compared with the device's through a checksum.  The traffic the call implies is counted
from the shapes and printed beside the times, with the time that traffic would take at the device's 8 TB/s peak.

    python tests/dev/covis_time.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/dev/covis_time.py --reps 20 --no-host --only 64
        k_covis' own time in DIR's kernel_stats: a run of its own (--only 1 or --only 64: one launch shape per trace; the two
        layouts launch the same work)

The clocks are whatever the device runs at under the load (not pinned)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import capi  # noqa: E402

PEAK_BYTES_PER_S = 8e12
N_VIEWS, ITEMS, HAND_OUT = 500, 2000, 30


def make_map(seed=1):
    """-> (lists, per keyframe the points it sees): runs of 2 + Poisson(3.5) consecutive keyframes, enough points that every
    keyframe sees 2 000 of them"""
    rng = np.random.default_rng(seed)
    n_points = int(N_VIEWS * ITEMS / 5.5 * 1.15)
    length = np.minimum(2 + rng.poisson(3.5, n_points), N_VIEWS)
    start = rng.integers(0, N_VIEWS - length + 1)
    lists = [np.arange(s, s + n, dtype=np.int32) for s, n in zip(start, length)]
    seen = [[] for _ in range(N_VIEWS)]
    for p, l in enumerate(lists):
        for v in l:
            seen[v].append(p)
    return lists, seen


def make_queries(seen, n_queries, seed=2):
    rng = np.random.default_rng(seed)
    frames = np.linspace(20, N_VIEWS - 21, n_queries).astype(np.int32)
    queries = []
    for k in frames:
        assert len(seen[k]) >= ITEMS, (k, len(seen[k]))
        queries.append(rng.choice(seen[k], size=ITEMS, replace=False).astype(np.int32))
    return queries, frames


def timed(fn, warmup, reps):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t[warmup:])
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p90_ms=float(np.percentile(t, 90)))


def checksum(res):
    """what tests/dev/covis_map_loop.cpp adds up, from the device's arrays (max_out = n_views)"""
    total = 0
    for q in range(len(res["n_counted"])):
        nc, nk = int(res["n_counted"][q]), int(res["n_connected"][q])
        total += nc + 3 * nk + 5 * (int(res["best_view"][q]) + 1) + 7 * int(res["best_weight"][q])
        if nc and res["best_weight"][q] < 15:
            total += int(res["best_view"][q]) + 1
        else:
            total += int(((np.arange(nk) + 1) * (res["out_view"][q, :nk].astype(np.int64) + 1)).sum())
    return total


def write_call(path, d, keep):
    with open(path, "wb") as f:
        f.write(np.array([d.n_views, d.n_points, d.n_queries, d.min_weight, d.max_out, len(keep["obs_view"]), len(keep["query_point"]),
                          int("query_self" in keep), int("eligible" in keep)], np.int32).tobytes())
        for key in ("obs_ptr", "obs_view", "query_ptr", "query_point", "query_self", "eligible"):
            if key in keep:
                f.write(keep[key].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the std::map loop (profiler runs)")
    ap.add_argument("--only", type=int, default=0, help="1 or 64: time that shape alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    lists, seen = make_map()
    n_obs = int(sum(len(l) for l in lists))
    out = dict(n_views=N_VIEWS, n_points=len(lists), n_obs=n_obs, observers_per_point=n_obs / len(lists), items_per_query=ITEMS, hand_out=HAND_OUT, reps=a.reps)
    tmp = tempfile.mkdtemp(prefix="covis_time_")
    exe = None
    if not a.no_host:
        exe = os.path.join(tmp, "covis_map_loop")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(os.path.dirname(os.path.abspath(__file__)), "covis_map_loop.cpp"), "-o", exe])
    s = capi.Solver()
    for nq in (1, 64):
        if a.only and a.only != nq:
            continue
        all_queries, frames = make_queries(seen, nq)
        # the whole order once, for the checksum and the shape of the result
        full = s.covisibility(N_VIEWS, lists, all_queries, query_self=frames)
        entries = int(sum(len(lists[p]) for q in all_queries for p in q))
        for layout in ("whole_map", "own_points"):
            # own_points: the caller hands over the lists of the points its queries name and nothing else, renumbered
            if layout == "own_points":
                used = np.unique(np.concatenate(all_queries))
                new_index = np.full(len(lists), -1, np.int32)
                new_index[used] = np.arange(len(used), dtype=np.int32)
                call_lists, queries = [lists[p] for p in used], [new_index[q] for q in all_queries]
            else:
                call_lists, queries = lists, all_queries
            row = dict(n_queries=nq, n_points=len(call_lists), n_obs=int(sum(len(l) for l in call_lists)))
            row["n_counted"] = [int(full["n_counted"].min()), int(full["n_counted"].max())]
            row["n_connected"] = [int(full["n_connected"].min()), int(full["n_connected"].max())]
            row["best_weight"] = [int(full["best_weight"].min()), int(full["best_weight"].max())]
            d, keep = capi.covis_desc(N_VIEWS, call_lists, queries, query_self=frames, max_out=HAND_OUT)
            b = dict(bus_in=int(sum(v.nbytes for v in keep.values())), bus_out=16 * nq + 8 * nq * HAND_OUT,
                     device=8 * nq + 4 * nq + 12 * nq * ITEMS + 4 * entries)      # per query: its prefix pair and self, per item its index and list bounds, per observation its view
            b["total"] = b["bus_in"] + b["bus_out"] + b["device"]
            b["at_peak_us"] = b["total"] / PEAK_BYTES_PER_S * 1e6
            row["bytes"], row["observations_counted"] = b, entries
            for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
                r, buf = capi.covis_result(nq, HAND_OUT, alloc)

                def call():
                    assert s._L.movba_covisibility(s._h, C.byref(d), C.byref(r)) == 0
                row[f"call_{where}"] = timed(call, a.warmup, a.reps)
                assert np.array_equal(buf["out_view"], full["out_view"][:, :HAND_OUT]) and np.array_equal(buf["n_connected"], full["n_connected"])
            if exe:
                src = os.path.join(tmp, f"call_{nq}_{layout}.bin")
                write_call(src, d, keep)
                host = json.loads(subprocess.check_output([exe, src, str(a.host_reps)], text=True))
                assert host["checksum"] == checksum(full), (host["checksum"], checksum(full))
                row["host_std_map"] = dict(median_ms=host["median_ms"], min_ms=host["min_ms"])
            out[f"queries_{nq}_{layout}"] = row
    s.close()
    for k, v in out.items():
        print(k, v)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
