"""Developer timer of movba_mv_raster (not collected by pytest) at the workload's own shape: a 1080 x 1920 P-frame whose records
stand on the macroblock grid with motion of up to 6 pixels, 3 000 point queries and the 7 973 rects of the lattice.

    mb16_1         one frame, one record of 16 x 16 per macroblock: 8 040 records, 7 973 kept (the last column's dst_x + 8 = W)
    mb8_1          one frame, one record of 8 x 8 per quarter: 32 400 records
    mb16_8         8 frames of mb16_1's kind in one call (8 streams)
    n<k>           mb16_1 thinned to k records: where the call breaks even with the host loop
    qvga, tiny     a 240 x 320 frame with 300 records and 300 queries, a 64 x 96 frame with 24 and 30: small frames
    floor          one 16 x 16 frame, one record, one query: what a call costs whatever it holds

Per shape: wall time per call, warm, host clock around the whole call (checks, packing, copy in, the launches, synchronisation,
copy-out) on descriptors and result buffers built once, results in movba_host_alloc memory and in ordinary memory, each timed
twice (the spread between the two is the noise of the box); and the same loop on one host thread (tests/dev/mv_raster_loop.cpp,
built here with g++ -O2: clear the 4-channel image, walk, paint, gather), its results compared with the device's through a
checksum.  --chain adds movba_advance on the frame of tests/dev/advance_time.py fed from mb16_1's outputs: the call alone, and
what stands in front of it either way (the host loop, or movba_mv_raster).

    python tests/dev/mv_raster_time.py [--out FILE] [--chain]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/dev/mv_raster_time.py --reps 20 --no-host --only mb16_1
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
import mv_raster_ref as M  # noqa: E402
from express_time import timed  # noqa: E402

ROWS, COLS, N_Q = 1080, 1920, 3000


def grid_records(rng, rows, cols, size, keep=None):
    """one record of size x size per block of the frame's grid, in raster order, its source up to 6 pixels away; keep: thin to
    that many, in order"""
    ys, xs = np.mgrid[0:(rows + size - 1) // size, 0:(cols + size - 1) // size]
    dst = np.stack([xs.reshape(-1) * size + size // 2, ys.reshape(-1) * size + size // 2], axis=1)
    if keep is not None:
        dst = dst[np.sort(rng.choice(len(dst), keep, replace=False))]
    src = dst - rng.integers(-6, 7, dst.shape)
    return [(int(s[0]), int(s[1]), int(d[0]), int(d[1]), size, size) for s, d in zip(src, dst)]


def make_frame(rng, rows, cols, size, n_q, keep=None, q_pt=None):
    q = np.stack([rng.uniform(0, cols, n_q), rng.uniform(0, rows, n_q)], axis=1) if q_pt is None else q_pt
    return M.frame(rows, cols, grid_records(rng, rows, cols, size, keep), q, threshold=0.3, want_grid=1)


def checksum(res):
    """what tests/dev/mv_raster_loop.cpp adds up, from the device's arrays"""
    total = int(((res["cand"].astype(np.int64) + 1) * np.arange(1, 5)).sum()) + 1000003 * int(res["kept_ptr"][-1]) + 1009 * int(res["grid_covered"].sum())
    return total + int(res["cover_px"].astype(np.int64).sum()) + 7 * int(res["force_grid"].sum())


def write_call(path, keep, n_frames):
    """the format of tests/mv_raster/mvr_main.cpp"""
    with open(path, "wb") as f:
        f.write(np.array([n_frames, len(keep["src_x"]), len(keep["q_pt"])], np.int32).tobytes())
        for key in ("rows", "cols", "coverage_threshold", "want_grid", "rec_ptr", "q_ptr", "src_x", "src_y", "dst_x", "dst_y", "w", "h", "q_pt"):
            f.write(keep[key].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=9)
    ap.add_argument("--no-host", action="store_true", help="skip the host loop (profiler runs)")
    ap.add_argument("--only", default=None, help="shape names, comma-separated: time those shapes alone")
    ap.add_argument("--chain", action="store_true", help="also movba_advance behind mb16_1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    chain = None
    q_pt = None
    if a.chain:
        from advance_time import make_inter_frame
        from express_time import make_frame as make_image
        chain = make_inter_frame(rng, make_image(rng), 0)
        q_pt = chain["prev_pt"]
    mb16 = make_frame(rng, ROWS, COLS, 16, N_Q, q_pt=q_pt)
    shapes = dict(mb16_1=[mb16], mb8_1=[make_frame(rng, ROWS, COLS, 8, N_Q)], mb16_8=[mb16] + [make_frame(rng, ROWS, COLS, 16, N_Q) for _ in range(7)])
    for k in (50, 200, 800, 2000):
        shapes[f"n{k}"] = [make_frame(rng, ROWS, COLS, 16, N_Q, keep=k)]
    shapes.update(qvga=[make_frame(rng, 240, 320, 16, 300)], tiny=[make_frame(rng, 64, 96, 16, 30)], floor=[M.frame(16, 16, [(6, 6, 7, 7, 4, 4)], [(5.0, 5.0)])])
    out = dict(rows=ROWS, cols=COLS, reps=a.reps, warmup=a.warmup)
    tmp = tempfile.mkdtemp(prefix="mv_raster_time_")
    exe = None
    if not a.no_host:
        exe = os.path.join(tmp, "mv_raster_loop")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mv_raster_loop.cpp"), "-o", exe])
    s = capi.Solver()
    for name, frames in shapes.items():
        if a.only and name not in a.only.split(","):
            continue
        full = s.mv_raster(frames)
        d, keep = capi.mv_raster_desc(frames)
        n_rec, n_q = len(keep["src_x"]), len(keep["q_pt"])
        row = dict(n_frames=len(frames), n_records=n_rec, n_kept=int(full["kept_ptr"][-1]), n_q=n_q, n_grid=keep["n_grid"], covered=int(full["grid_covered"].sum()),
                   slots=np.bincount((full["cand"] >= 0).sum(axis=1), minlength=5).tolist(), coverage_area=full["coverage_area"].tolist()[:2])
        for where, alloc in (("pinned", s._pinned), ("ordinary", np.zeros)):
            r, buf = capi.mv_raster_result(d.n_frames, n_rec, n_q, keep["n_grid"], alloc)

            def call():
                assert s._L.movba_mv_raster(s._h, C.byref(d), C.byref(r)) == 0
            row[f"call_{where}"] = [timed(call, a.warmup, a.reps) for _ in range(2)]
            assert np.array_equal(buf["cand"], full["cand"]) and np.array_equal(buf["kp_rect"], full["kp_rect"]) and np.array_equal(buf["grid_covered"], full["grid_covered"])
        if exe:
            path = os.path.join(tmp, f"call_{name}.bin")
            write_call(path, keep, len(frames))
            host = json.loads(subprocess.check_output([exe, path, str(a.host_reps)], text=True))
            os.remove(path)
            assert host["host_loop"]["checksum"] == checksum(full), (name, host["host_loop"]["checksum"], checksum(full))
            row["host_loop"] = dict(median_ms=host["host_loop"]["median_ms"], min_ms=host["host_loop"]["min_ms"])
        if chain is not None and name == "mb16_1":
            k0, k1 = int(full["kept_ptr"][0]), int(full["kept_ptr"][1])
            fr = dict(chain, force_grid=int(full["force_grid"][0]), prev_cand=full["cand"], mv_pt=full["mv_pt"][k0:k1], mv_dindx=full["mv_dindx"][k0:k1],
                      kp_rect=full["kp_rect"][k0:k1], grid_covered=full["grid_covered"])
            walked = s.advance([fr])
            ad, akeep = capi.advance_desc([fr])
            ar, _ = capi.advance_result(1, len(akeep["prev_age"]), len(akeep["kp_rect"]), akeep["n_grid"], s._pinned)

            def advance_call():
                assert s._L.movba_advance(s._h, C.byref(ad), C.byref(ar)) == 0
            r, _ = capi.mv_raster_result(1, n_rec, n_q, keep["n_grid"], s._pinned)

            def both():
                assert s._L.movba_mv_raster(s._h, C.byref(d), C.byref(r)) == 0
                assert s._L.movba_advance(s._h, C.byref(ad), C.byref(ar)) == 0
            row["chain"] = dict(advance_alone=timed(advance_call, a.warmup, a.reps), mv_raster_then_advance=timed(both, a.warmup, a.reps),
                                fates=np.bincount(walked["fate"], minlength=20)[[1, 2, 16, 17, 18, 19]].tolist(), mov_cnt=walked["mov_cnt"].tolist(),
                                features=int(walked["seg_ptr"][-1]))
        out[name] = row
    s.close()
    for k, v in out.items():
        print(k, v)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
