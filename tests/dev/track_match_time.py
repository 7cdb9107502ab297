"""Developer timer of movba_track_match (not collected by pytest) at the workload's own shape: keyframes of 2 000 features, 40 % of
the slots already holding a map point, a neighbour carrying 60 % of the current keyframe's track ids in its own order.

    tri_1          one TRIANGULATION query of 2 000 x 2 000 slots
    tri_30         30 such queries in one call: one keyframe against its neighbours (CreateNewMapPoints)
    lookup_2000    one LOOKUP query of 2 000 items in a view of 2 000 slots (SearchByVideoFeature)

Per shape: wall time per call, warm, host clock around the whole call (checks, packing, copy in, two launches, synchronisation)
on descriptors and result buffers built once, results in movba_host_alloc memory and in ordinary memory, the payload (obs, ur,
depth) gathered; two passes over the shapes, so that the spread between them shows beside the medians; and the same joins on one
host thread (tests/dev/track_match_loop.cpp, built here with g++ -O2): the double loop as the reference writes it and a
std::unordered_map join, both with the gather, their results compared with the device's through a checksum.

    python tests/dev/track_match_time.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/dev/track_match_time.py --reps 20 --no-host --only tri_30
        k_tm_match's and k_tm_pack's own times in DIR's kernel_stats: a run of its own, one launch shape per trace

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

SLOTS, NEIGHBOURS, TAKEN, SHARED = 2000, 30, 0.4, 0.6
PAYLOAD = ("obs1", "obs2", "ur1", "ur2", "depth1", "depth2")


def make_views(seed=1):
    """the current keyframe (view 0) and its neighbours: a neighbour keeps SHARED of the current keyframe's ids, in its own order,
    and fills up with ids of its own"""
    rng = np.random.default_rng(seed)

    def view(track):
        n = len(track)
        return dict(track=track.astype(np.int32), taken=(rng.random(n) < TAKEN).astype(np.uint8), obs=rng.uniform(0, 640, (n, 2)),
                    ur=np.where(rng.random(n) < 0.5, rng.uniform(0, 640, n), -1.0), depth=rng.uniform(1, 30, n))

    current = rng.permutation(1 << 20)[:SLOTS]
    views = [view(current)]
    for k in range(NEIGHBOURS):
        kept = rng.choice(current, int(SHARED * SLOTS), replace=False)
        own = (1 << 21) + k * SLOTS + np.arange(SLOTS - len(kept))
        views.append(view(rng.permutation(np.concatenate([kept, own]))))
    return views


def timed(fn, warmup, reps):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t[warmup:])
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p90_ms=float(np.percentile(t, 90)))


def checksum(res):
    """what tests/dev/track_match_loop.cpp adds up, from the device's arrays"""
    n = int(res["n_matches"])
    total = n + int((res["match_slot1"][:n].astype(np.int64) + 1).sum()) + 3 * int((res["match_slot2"][:n].astype(np.int64) + 1).sum())
    if "obs2" in res["matches"]:
        total += int((np.ascontiguousarray(res["matches"]["obs2"][:n, 0]).view(np.uint64) >> np.uint64(40)).sum())
    return total + 5 * int((res["item_slot"].astype(np.int64) + 2).sum())


def write_call(path, d, keep):
    """the format of tests/track_match/tm_main.cpp"""
    have = [int(k in keep) for k in ("slot_taken", "slot_obs", "slot_ur", "slot_depth")]
    with open(path, "wb") as f:
        f.write(np.array([d.n_views, d.n_queries, len(keep["slot_track"]), len(keep["item_track"])] + have, np.int32).tobytes())
        for key in ("view_ptr", "slot_track", "query_mode", "query_view", "query_ptr", "item_track", "slot_taken", "slot_obs", "slot_ur", "slot_depth"):
            if key in keep:
                f.write(keep[key].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host joins (profiler runs)")
    ap.add_argument("--only", default=None, help="tri_1, tri_30 or lookup_2000: time that shape alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    views = make_views()
    rng = np.random.default_rng(3)
    ids = np.where(rng.random(SLOTS) < SHARED, rng.choice(views[1]["track"], SLOTS), (1 << 22) + np.arange(SLOTS)).astype(np.int32)
    T, L = capi.TM_TRIANGULATION, capi.TM_LOOKUP
    shapes = dict(tri_1=(views[:2], [(T, 0, 1)]), tri_30=(views, [(T, 0, k + 1) for k in range(NEIGHBOURS)]), lookup_2000=(views[:2], [(L, 1, ids)]))
    out = dict(slots=SLOTS, neighbours=NEIGHBOURS, taken=TAKEN, shared=SHARED, reps=a.reps, warmup=a.warmup, passes=2)
    tmp = tempfile.mkdtemp(prefix="track_match_time_")
    exe = None
    if not a.no_host:
        exe = os.path.join(tmp, "track_match_loop")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(os.path.dirname(os.path.abspath(__file__)), "track_match_loop.cpp"), "-o", exe])
    s = capi.Solver()
    calls = {}
    for name, (vw, queries) in shapes.items():
        if a.only and a.only != name:
            continue
        full = s.track_match(vw, queries)
        d, keep = capi.track_desc(vw, queries)
        row = dict(n_queries=d.n_queries, n_slots=len(keep["slot_track"]), n_items=len(keep["item_track"]), match_cap=keep["match_cap"],
                   n_matches=int(full["n_matches"]), n_found=int(full["n_found"].sum()),
                   bus_in_bytes=int(sum(v.nbytes for v in keep.values() if isinstance(v, np.ndarray))))
        bufs = {}
        for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
            bufs[where] = capi.track_result(d.n_queries, len(keep["item_track"]), keep["match_cap"], PAYLOAD, alloc)
            row[f"call_{where}"] = []
        calls[name] = (d, keep, bufs, full)
        out[name] = row
    for _ in range(2):
        for name, (d, keep, bufs, full) in calls.items():
            for where, (r, buf) in bufs.items():
                def call():
                    assert s._L.movba_track_match(s._h, C.byref(d), C.byref(r)) == 0
                out[name][f"call_{where}"].append(timed(call, a.warmup, a.reps))
                assert np.array_equal(buf["match_slot2"], full["match_slot2"]) and np.array_equal(buf["item_slot"], full["item_slot"])
    for name, (d, keep, bufs, full) in calls.items():
        if exe:
            src = os.path.join(tmp, f"call_{name}.bin")
            write_call(src, d, keep)
            host = json.loads(subprocess.check_output([exe, src, str(a.host_reps)], text=True))
            for method in ("double_loop", "unordered_map"):
                assert host[method]["checksum"] == checksum(full), (name, method, host[method]["checksum"], checksum(full))
                out[name]["host_" + method] = dict(median_ms=host[method]["median_ms"], min_ms=host[method]["min_ms"])
    s.close()
    for k, v in out.items():
        print(k, v)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
