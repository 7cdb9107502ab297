"""Developer timer of movba_stereo_points (not collected by pytest) at the workload's own shapes:

    f1200        one stereo frame with 1 200 keypoints, MOVBA_STEREO_SELECT_CLOSE (a keyframe insertion)
    f1200_all    the same frame with MOVBA_STEREO_SELECT_ALL (the initialisation)
    f1200_8      8 such frames in one call (8 streams)
    f16384       one frame at the bound, 16 384 keypoints, CLOSE: the sort at 128 KiB of LDS
    floor        one frame, one point: what a call costs whatever it holds

The frames are tests/stereo_ref.py's random_frame: disparities of 0.4 .. 30 pixels, a tenth far off, a tenth lost, a pose.
Per shape: wall time per call, warm, host clock around the whole call (checks, packing, copy in, the two launches, synchronisation,
copy-out) on descriptors and result buffers built once, results in movba_host_alloc memory and in ordinary memory, each timed
twice (the spread between the two is the noise of the box); and the same work on one host thread (tests/stereo_points/
stereo_main.cpp, built here with g++ -O2 and no sanitizer: stereo_points.h's own walk), its results compared with the device's bit
for bit.

    python tests/dev/stereo_time.py [--out FILE]

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
import stereo_ref as S  # noqa: E402
from express_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host walk (profiler runs)")
    ap.add_argument("--only", default=None, help="shape names, comma-separated: time those shapes alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    one = S.random_frame(1200, 1, S.CLOSE, pose=S.POSE_NEAR)
    shapes = dict(f1200=[one], f1200_all=[dict(one, select=S.ALL)],
                  f1200_8=[one] + [S.random_frame(1200, 10 + k, S.CLOSE, pose=S.POSE_FAR) for k in range(7)],
                  f16384=[S.random_frame(16384, 2, S.CLOSE, pose=S.POSE_NEAR)], floor=[S.random_frame(1, 3, S.CLOSE)])
    out = dict(reps=a.reps, warmup=a.warmup)
    tmp = tempfile.mkdtemp(prefix="stereo_time_")
    exe = None
    if not a.no_host:
        exe = os.path.join(tmp, "stereo_main")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "hipstub"),
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mov-slam_amd", "csrc"),
                               os.path.join(ROOT, "tests", "stereo_points", "stereo_main.cpp"), "-o", exe])
    s = capi.Solver()
    for name, frames in shapes.items():
        if a.only and name not in a.only.split(","):
            continue
        full = s.stereo_points(frames)
        d, keep = capi.stereo_desc(frames)
        n = len(keep["pt"])
        h2d = sum(keep[k].nbytes for k in ("pt_ptr", "pt", "next_pt", "pt_status", "pt_un", "has_point") if keep[k] is not None) + 144 * len(frames)
        row = dict(n_frames=len(frames), n_pt=n, n_stereo=int(full["n_stereo"].sum()), selected=int(full["sel_ptr"][-1]), bytes_in=int(h2d),
                   bytes_out=int(sum(v.nbytes for k, v in full.items() if k in S.KEYS)))
        for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
            r, buf = capi.stereo_result(d.n_frames, n, alloc)

            def call():
                assert s._L.movba_stereo_points(s._h, C.byref(d), C.byref(r)) == 0
            row[f"call_{where}"] = [timed(call, a.warmup, a.reps) for _ in range(2)]
            S.compare(dict(buf), full, name, point="exact")
        if exe:
            host = S.run_stereo_main(exe, frames, tmp, reps=a.host_reps)
            S.compare(host, full, name + ", the host walk", point="exact")
            row["host_walk"] = host["host_walk"]
        out[name] = row
        print(name, row, flush=True)
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
