"""Developer timer of movba_lk_track (not collected by pytest) at the workload's own shapes: one frame pair with 1 200 points, the
reference's parameters (3 levels above the image, 20 iterations, eps 0.01, threshold 1e-4).

    vga31, vga21       480 x 640, window 31 (the extractor's calls) and 21 (the stereo call)
    hd31, hd21         1080 x 1920
    vga31_8            8 frame pairs of vga31's kind in one call (8 streams)
    n<k>               vga31 with k points: where the call breaks even with the host loop
    floor              one 40 x 36 frame, one point, window 5: what a call costs whatever it holds

The images are a texture of tests/lk_ref.py moved by (2.5, -1.25) pixels with light noise; the points are uniform over the frame.
Per shape: wall time per call, warm, host clock around the whole call (checks, packing of both images, copy in, the launches,
synchronisation, copy-out) on descriptors and result buffers built once, results in movba_host_alloc memory and in ordinary
memory, each timed twice (the spread between the two is the noise of the box); and the same work on one host thread
(tests/dev/lk_loop.cpp, built here with g++ -O2: lk.h's own statements, both pyramids and every point - not OpenCV's SIMD code),
its results compared with the device's through a checksum.

    python tests/dev/lk_time.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/dev/lk_time.py --reps 20 --no-host --only vga31
        the kernels' own times in DIR's stats: a run of its own

The clocks are whatever the device runs at under the load (not pinned)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from movba import capi  # noqa: E402
import lk_ref as K  # noqa: E402
from express_time import timed  # noqa: E402

N_PT = 1200


def make_frame(rng, rows, cols, win, n_pt, seed):
    pts = np.stack([rng.uniform(0, cols, n_pt), rng.uniform(0, rows, n_pt)], axis=1)
    return K.frame(rows, cols, win, pts, seed=seed, shift8=(20, -10), noise=2)


def checksum(res):
    """what tests/dev/lk_loop.cpp adds up, from the device's arrays"""
    bits = np.ascontiguousarray(res["next_pt"]).view(np.uint32).astype(np.int64) >> 8
    return int(bits.sum()) + 7 * int(res["exit_code"].astype(np.int64).sum()) + 13 * int(res["keep"].sum()) + 1000003 * int(res["kept_ptr"][-1])


def write_call(path, frames, keep, p):
    """the format of tests/lk/lk_main.cpp"""
    with open(path, "wb") as f:
        f.write(np.array([len(frames), len(keep["pt"]), p["max_level"], p["max_iter"]], np.int32).tobytes())
        f.write(np.array([p["eps"], p["min_eig_threshold"]], np.float64).tobytes())
        for key in ("rows", "cols", "win", "pt_ptr", "pt"):
            f.write(keep[key].tobytes())
        for fr in frames:
            if len(fr["pt"]):
                f.write(np.ascontiguousarray(fr["prev"]).tobytes())
                f.write(np.ascontiguousarray(fr["next"]).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host loop (profiler runs)")
    ap.add_argument("--only", default=None, help="shape names, comma-separated: time those shapes alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    vga31 = make_frame(rng, 480, 640, 31, N_PT, 1)
    shapes = dict(vga31=[vga31], vga21=[dict(vga31, win=21)], hd31=[make_frame(rng, 1080, 1920, 31, N_PT, 2)])
    shapes["hd21"] = [dict(shapes["hd31"][0], win=21)]
    shapes["vga31_8"] = [vga31] + [make_frame(rng, 480, 640, 31, N_PT, 10 + k) for k in range(7)]
    for k in (10, 50, 200):
        shapes[f"n{k}"] = [dict(vga31, pt=vga31["pt"][:k])]
    shapes["floor"] = [K.frame(40, 36, 5, [(20.0, 18.0)], seed=3)]
    out = dict(n_pt=N_PT, reps=a.reps, warmup=a.warmup)
    tmp = tempfile.mkdtemp(prefix="lk_time_")
    exe = None
    if not a.no_host:
        exe = os.path.join(tmp, "lk_loop")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "hipstub"),
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mov-slam_amd", "csrc"),
                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "lk_loop.cpp"), "-o", exe])
    s = capi.Solver()
    for name, frames in shapes.items():
        if a.only and name not in a.only.split(","):
            continue
        full = s.lk_track(frames)
        d, keep = capi.lk_desc(frames)
        n = len(keep["pt"])
        row = dict(n_frames=len(frames), n_pt=n, kept=int(full["kept_ptr"][-1]), exits=K.digest(full)["exits"],
                   levels=[len(K.level_sizes(fr["prev"].shape[0], fr["prev"].shape[1], fr["win"], 3)) - 1 for fr in frames][:2])
        for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
            r, buf = capi.lk_result(d.n_frames, n, alloc)

            def call():
                assert s._L.movba_lk_track(s._h, C.byref(d), C.byref(r)) == 0
            row[f"call_{where}"] = [timed(call, a.warmup, a.reps) for _ in range(2)]
            K.compare(dict(buf), full, name)
        if exe:
            path = os.path.join(tmp, f"call_{name}.bin")
            write_call(path, frames, keep, K.PARAMS)
            host = json.loads(subprocess.check_output([exe, path, str(a.host_reps)], text=True))
            os.remove(path)
            assert host["host_loop"]["checksum"] == checksum(full), (name, host["host_loop"]["checksum"], checksum(full))
            row["host_loop"] = dict(median_ms=host["host_loop"]["median_ms"], min_ms=host["host_loop"]["min_ms"])
        out[name] = row
        print(name, row, flush=True)
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
