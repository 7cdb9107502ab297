"""The clock-stamp build (-DMOVBA_CLOCK_STAMP, MOVBA_LIB=build/libmovba_stamp.so) beside the product library: solves tiny, cfg2
and cfg3 and prints a digest of each result - the two builds are expected to print the same lines.  With the stamp build it
also checks the stamp buffer: record counts equal to the launch grids, every record valid, non-zero segment sums, and that a
batched run of two windows leaves each window the records of a solo run."""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd"))
from movba import synth, capi

POINT, SCHUR, SEGMENTS = 0, 1, 2
SEG_CYCLES, SEG_TICKS, SEG_ITER, SEG_PHASE, SEG_WAVE = 0, 1, 2, 10, 18     # clock_stamp.h


s = capi.Solver()
stamped = hasattr(s._L, "movba_stamp_records")
print("library:", os.path.basename(capi.LIB_PATH), "(stamp build)" if stamped else "(no stamps)")
for name in ("tiny", "cfg2", "cfg3"):
    w = synth.cfg(name)
    r = s.solve(w)
    dig = " ".join(k + "=" + hashlib.sha256(np.ascontiguousarray(r[k]).tobytes()).hexdigest()[:16] for k in ("poses", "points", "chi2", "outlier"))
    print(f"{name}: E={len(r['chi2'])} P={len(r['points'])} solves={r['n_solves']} pcg={r['pcg_iters']} band={r['n_band']} direct={r['n_direct']} {dig}")
    if not stamped:
        continue
    assert r["n_solves"] >= 4, "the recorded launch is the one that finds n_solves == 3"
    pt, sc, seg = s.stamp_records(POINT), s.stamp_records(SCHUR), s.stamp_records(SEGMENTS).reshape(-1)
    n_pt_blocks = (len(r["points"]) + 31) // 32                     # kPointsPerBlock
    assert len(pt) == n_pt_blocks + 1, (len(pt), n_pt_blocks)
    assert (pt[:-1, 7] == 1).all() and pt[-1, 7] == 2, "a workgroup of the back-substitution pass left no record"
    assert (np.diff(pt[:-1, :6].astype(np.int64), axis=1) >= 0).all() and pt[-1, 1] >= pt[-1, 0]
    n_waves = capi.structure_probe(w)["n_sched_slots"]            # k_schur's grid by wave: the launch schedule's slots
    assert n_waves > 0 and len(sc) == n_waves, (len(sc), n_waves)
    assert (sc[:, 7] == 1).all(), "a wave of k_schur left no record"
    assert (np.diff(sc[:, :5].astype(np.int64), axis=1) >= 0).all()
    if r["n_band"] > 0:
        assert seg[SEG_PHASE:SEG_PHASE + 8].sum() > 0
    elif r["n_direct"] < r["n_solves"]:
        assert seg[SEG_CYCLES] > 0 and seg[SEG_TICKS] > 0 and seg[SEG_ITER:SEG_ITER + 8].sum() > 0 and seg[SEG_WAVE:SEG_WAVE + 64].sum() > 0
        assert seg[SEG_PHASE:SEG_PHASE + 8].sum() > 0
    solo_iter = int(seg[SEG_ITER:SEG_ITER + 8].sum())               # (cfg3's, the last: what the batched windows are held against)
    print(f"  stamps ok: {len(pt)} point-pass records, {len(sc)} schur records ({int((sc[:, 5] > 0).sum())} busy waves), "
          f"segment sums cycles={seg[SEG_CYCLES]} ticks={seg[SEG_TICKS]} iter={seg[SEG_ITER:SEG_ITER + 8].sum()} phase={seg[SEG_PHASE:SEG_PHASE + 8].sum()}")
s.close()
if stamped:
    # movba_lba_run_batch: each window's buffer is its own, zeroed at the start of the batch as at the start of a solo run
    import torch
    st = torch.cuda.Stream()
    w = synth.cfg("cfg3")
    pair = [capi.Solver(device=0, stream=st.cuda_stream) for _ in range(2)]
    for b in pair: b.upload(w)
    capi.run_batch(pair); capi.run_batch(pair)
    n_waves = capi.structure_probe(w)["n_sched_slots"]
    sums = []
    for b in pair:
        r = b.download()
        pt, sc, seg = b.stamp_records(POINT), b.stamp_records(SCHUR), b.stamp_records(SEGMENTS).reshape(-1)
        assert len(pt) == (len(r["points"]) + 31) // 32 + 1 and (pt[:-1, 7] == 1).all() and pt[-1, 7] == 2
        assert len(sc) == n_waves and (sc[:, 7] == 1).all()
        sums.append(int(seg[SEG_ITER:SEG_ITER + 8].sum()))
        b.close()
    # (the second batch's iterations alone, not both batches': the solo run's sum, not twice it)
    assert all(0 < v < 1.5 * solo_iter for v in sums), (sums, solo_iter)
    print(f"  batch of two cfg3 windows: records ok, per-iteration segment sums {sums}")
print("stamp_check done")
