"""Developer timer of movba_advance (not collected by pytest) at the workload's own shape: a 1080 x 1920 frame of tiled noisy step
edges, threshold 25, about 3 000 previous features with 1 - 4 candidates among 1 500 motion vectors, about 4 000 macroblocks of
the four shapes and the 7 973 rects of the lattice.

    inter_1        one such frame (one stream's P-frame)
    inter_8        8 such frames in one call (8 streams)

Per shape: wall time per call, warm, host clock around the whole call (checks, packing, copy in, four launches,
synchronisation, copy-out) on descriptors and result buffers built once, results in movba_host_alloc memory and in ordinary
memory; movba_express on the same block items - one DESCRIBE item per candidate, the macroblocks and the lattice as DETECT
items: the part of the path that call covers, without the walk; and the same walk on one host thread (tests/dev/advance_loop.cpp,
built here with g++ -O2), its results compared with the device's through a checksum.

    python tests/dev/advance_time.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/dev/advance_time.py --reps 20 --no-host --only inter_1
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
import advance_ref as A  # noqa: E402
import express_ref as R  # noqa: E402
from express_time import make_frame, timed  # noqa: E402

ROWS, COLS, THRESHOLD = 1080, 1920, 25
N_PREV, N_MV, N_KPS = 3000, 1500, 4000


def make_inter_frame(rng, image, first_id):
    """previous features at random places whose descriptors are those of where they stand in `image` with up to 30 bits flipped
    (the previous frame looked alike), vectors of up to 6 pixels, each with the macroblock it points to or none"""
    kp = np.concatenate([R.random_rects(rng, ROWS, COLS, s, N_KPS // 4) for s in R.SHAPES])
    kp = kp[rng.permutation(len(kp))]
    mv_pt = (rng.integers(-24, 25, (N_MV, 2)) / 4).astype(np.float32)
    mv_dindx = np.where(rng.random(N_MV) < 0.8, rng.integers(0, len(kp), N_MV), -1).astype(np.int32)
    mb = np.array([R.SHAPES[k] for k in rng.integers(0, 4, N_PREV)], np.int32)
    pt = np.stack([rng.uniform(20, COLS - 40, N_PREV), rng.uniform(20, ROWS - 40, N_PREV)], axis=1).astype(np.float32)
    n_cand = rng.integers(0, 5, N_PREV)
    cand = np.where(np.arange(4)[None, :] < n_cand[:, None], rng.integers(0, N_MV, (N_PREV, 4)), -1).astype(np.int32)
    desc = np.zeros((N_PREV, 4), np.uint64)
    for i in range(N_PREV):
        x, y = int(pt[i, 0]) - mb[i, 0] // 2, int(pt[i, 1]) - mb[i, 1] // 2
        desc[i] = R.words(A.flipped(A.true_desc(image, (x, y, mb[i, 0], mb[i, 1]), THRESHOLD), int(rng.integers(0, 30)), rng))
    return dict(image=image, threshold=THRESHOLD, force_grid=0, first_id=first_id, prev_pt=pt, prev_mb=mb,
                prev_age=rng.integers(0, 30, N_PREV).astype(np.int32), prev_track=np.arange(N_PREV, dtype=np.int32), prev_desc=desc,
                prev_coverage=(rng.random(N_PREV) < 0.05).astype(np.uint8), prev_cand=cand, mv_pt=mv_pt, mv_dindx=mv_dindx, kp_rect=kp,
                grid_covered=(rng.random(len(A.lattice(ROWS, COLS))) < 0.5).astype(np.uint8))


def express_items(fr):
    """the block items of a frame as movba_express takes them: one DESCRIBE item per candidate, the macroblocks, the lattice"""
    rects, refs = [], []
    for i in np.flatnonzero((fr["prev_coverage"] == 0) & (fr["prev_cand"][:, 0] >= 0)):
        for c in fr["prev_cand"][i]:
            if c < 0:
                break
            rects.append(A.rect_of(fr["prev_pt"][i], fr["mv_pt"][c], *fr["prev_mb"][i])[1])
            refs.append(fr["prev_desc"][i])
    n = len(rects)
    rects = np.concatenate([np.array(rects, np.int32).reshape(-1, 4), fr["kp_rect"], capi.express_grid(ROWS, COLS)])
    modes = np.concatenate([np.ones(n, np.int32), np.zeros(len(rects) - n, np.int32)])
    refs = np.concatenate([np.array(refs, np.uint64).reshape(-1, 4), np.zeros((len(rects) - n, 4), np.uint64)])
    return (rects, modes), refs


def checksum(res, frames):
    """what tests/dev/advance_loop.cpp adds up, from the device's arrays"""
    total = 0
    for f, fr in enumerate(frames):
        s = [int(v) for v in res["seg_ptr"][4 * f:4 * f + 4]]
        count = np.array([sum(bin(int(w)).count("1") for w in row) for row in res["feat_desc"][s[0]:s[3]]], np.int64)
        kept = slice(s[0], s[1])
        total += int(res["feat_track"][kept].astype(np.int64).sum() + res["feat_src"][kept].astype(np.int64).sum()
                     + res["feat_rect"][kept, :2].astype(np.int64).sum())
        rest = slice(s[1], s[3])
        total += int(res["feat_track"][rest].astype(np.int64).sum() + res["feat_src"][rest].astype(np.int64).sum()) + int(count.sum())
        total += 1000003 * (s[1] - s[0]) + 1009 * (s[2] - s[1]) + 7 * (s[3] - s[2]) + int(res["next_id"][f])
    return total


def write_call(path, keep, frames):
    """the format of tests/advance/adv_main.cpp"""
    lat = [len(A.lattice(*fr["image"].shape)) for fr in frames]
    with open(path, "wb") as f:
        f.write(np.array([len(frames), len(keep["prev_age"]), len(keep["mv_dindx"]), len(keep["kp_rect"]), keep["n_grid"]], np.int32).tobytes())
        for a in (keep["rows"], keep["cols"], keep["threshold"], keep["force_grid"].astype(np.int32), keep["first_id"], keep["prev_ptr"], keep["mv_ptr"],
                  keep["kp_ptr"], np.concatenate([[0], np.cumsum(lat)]).astype(np.int32), keep["prev_pt"], keep["prev_mb"], keep["prev_age"],
                  keep["prev_track"], keep["prev_cand"], keep["prev_desc"], keep["prev_coverage"], keep["mv_pt"], keep["mv_dindx"], keep["kp_rect"],
                  keep["grid_covered"]):
            f.write(a.tobytes())
        for fr in frames:
            f.write(np.ascontiguousarray(fr["image"]).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host loop (profiler runs)")
    ap.add_argument("--only", default=None, help="shape names, comma-separated: time those shapes alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    images = [make_frame(rng) for _ in range(2)]
    distinct = [make_inter_frame(rng, images[k], 1000 * k) for k in range(2)]
    shapes = dict(inter_1=[distinct[0]], inter_8=[distinct[k % 2] for k in range(8)])
    out = dict(rows=ROWS, cols=COLS, threshold=THRESHOLD, reps=a.reps, warmup=a.warmup)
    tmp = tempfile.mkdtemp(prefix="advance_time_")
    exe = None
    if not a.no_host:
        exe = os.path.join(tmp, "advance_loop")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(os.path.dirname(os.path.abspath(__file__)), "advance_loop.cpp"), "-o", exe])
    s = capi.Solver()
    for name, frames in shapes.items():
        if a.only and name not in a.only.split(","):
            continue
        full = s.advance(frames)
        d, keep = capi.advance_desc(frames)
        n_prev, n_kps = len(keep["prev_age"]), len(keep["kp_rect"])
        fates = np.bincount(full["fate"], minlength=20)
        row = dict(n_frames=len(frames), n_prev=n_prev, n_kps=n_kps, n_grid=keep["n_grid"], kept=int(fates[1]), coverage=int(fates[2]), no_mv=int(fates[16]),
                   rej_bounds=int(fates[17]), lost_claim=int(fates[18]), far=int(fates[19]), mov_cnt=full["mov_cnt"].tolist(), grid_ran=full["grid_ran"].tolist(),
                   features=int(full["seg_ptr"][-1]))
        for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
            r, buf = capi.advance_result(d.n_frames, n_prev, n_kps, keep["n_grid"], alloc)

            def call():
                assert s._L.movba_advance(s._h, C.byref(d), C.byref(r)) == 0
            row[f"call_{where}"] = [timed(call, a.warmup, a.reps) for _ in range(2)]
            assert np.array_equal(buf["feat_desc"], full["feat_desc"]) and np.array_equal(buf["fate"], full["fate"])
        # movba_express on the same block items
        items, refs = zip(*[express_items(fr) for fr in frames])
        ed, ekeep = capi.express_desc([fr["image"] for fr in frames], list(items), THRESHOLD, list(refs))
        er, _ = capi.express_result(len(ekeep["item_rect"]), ed.n_images, s._pinned)

        def express_call():
            assert s._L.movba_express(s._h, C.byref(ed), C.byref(er)) == 0
        row["express_items"] = len(ekeep["item_rect"])
        row["express_pinned"] = timed(express_call, a.warmup, a.reps)
        if exe:
            path = os.path.join(tmp, f"call_{name}.bin")
            write_call(path, keep, frames)
            host = json.loads(subprocess.check_output([exe, path, str(a.host_reps)], text=True))
            os.remove(path)
            assert host["host_loop"]["checksum"] == checksum(full, frames), (name, host["host_loop"]["checksum"], checksum(full, frames))
            row["host_loop"] = dict(median_ms=host["host_loop"]["median_ms"], min_ms=host["host_loop"]["min_ms"])
        out[name] = row
    s.close()
    for k, v in out.items():
        print(k, v)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
