"""movba_mv_raster on the device against the restatements of tests/mv_raster_ref.py, every comparison exact equality: the full
raster of a 48 x 40 frame (and of its transpose) with every clamp among its records; piles of 3, 4, 5 and 70 records on one
pixel; record and query counts that leave wavefronts partly filled and take the scan's carry over chunk boundaries; the sizes
at which the scans that only the device runs cross a wavefront - 66 chunks in one frame, record counts that are multiples of
the chunk, 1 024 frames with runs of empty ones; the mixed
call with an I-frame, a frame without queries and lattice, the padding and frame-by-frame independence; the coverage gate on
its boundary; queries on and over the edge; the outputs passed unchanged into Solver.advance; pinned results; a solved window
on the same handle left as it was; a refusal and an empty call on a live handle.  (tests/test_mv_raster_cpu.py holds the
library's steps to the same cases under AddressSanitizer first.)"""
import ctypes as C

import numpy as np
import pytest

import advance_ref as A
import express_ref as R
import mv_raster_ref as M
from movba import capi, synth

pytestmark = pytest.mark.gpu


def test_the_full_raster_of_a_frame_with_partial_tiles(solver):
    """every pixel of a 48 x 40 and of a 40 x 48 frame, 1 920 queries each, against the image the literal restatement paints"""
    frames = M.full_case()
    got = solver.mv_raster(frames)
    assert got["status"] == 0
    M.compare(got, M.full_ref(), "full")
    for f, fr in enumerate(frames):
        image = M.paint(fr)["mvi"]
        assert image.shape == (fr["rows"], fr["cols"], 4)
        assert np.array_equal(got["cand"][got["q_ptr"][f]:got["q_ptr"][f + 1]].reshape(image.shape), image)
    M.compare(solver.mv_raster(frames), got, "the same call twice")


def test_piles_of_3_4_5_and_70_records_on_one_pixel(solver):
    got = solver.mv_raster(M.pile_case())
    M.compare(got, M.pile_ref(), "pile")
    x, y = M.PILE_PIXEL
    at = [got["cand"][got["q_ptr"][f] + y * 56 + x] for f in range(4)]
    assert at[0][3] == -1 and all((a >= 0).all() for a in at[1:]) and at[3][3] > at[3][2] + 64


def test_partly_filled_waves_and_the_scans_carry(solver):
    """1, 63, 64, 65, 257 and 2 500 records per frame, the last with every third skipped; 0, 1 and 65 queries"""
    got = solver.mv_raster(M.counts_case())
    M.compare(got, M.counts_ref(), "counts")
    assert np.diff(got["rec_ptr"]).tolist() == list(M.COUNTS) and np.diff(got["q_ptr"]).tolist() == list(M.QUERY_COUNTS)
    big = got["rec_kept"][got["rec_ptr"][5]:]
    assert big[big >= 0].tolist() == list(range(got["kept_ptr"][6] - got["kept_ptr"][5]))


def test_66_chunks_of_one_frame_and_two_tiles_per_thread(solver):
    """one frame of 528 x 544 with 66 600 records and 2 000 queries: the carry of chunks 64 and 65 sums the counts of the chunks
    before them over two wavefronts of k_mvr_keep's scan, and k_mvr_offsets gives every thread two of the 1 122 tiles and the
    threads from 561 on none.  Every array against the numpy restatement; the first chunk's rows against the literal painting
    and every 20th query against the sets."""
    got = solver.mv_raster(M.chunks_case())
    assert got["status"] == 0
    ref = M.chunks_ref()
    assert np.array_equal(got["kept_ptr"], ref["kept_ptr"]), (got["kept_ptr"].tolist(), ref["kept_ptr"].tolist())
    M.compare(got, ref, "chunks")
    M.compare_head(got)
    kept = got["rec_kept"][got["rec_kept"] >= 0]
    assert kept.tolist() == list(range(got["kept_ptr"][1])) and got["rec_kept"][-2:].tolist() == [-1, got["kept_ptr"][1] - 1]


def test_record_counts_that_are_multiples_of_the_chunk(solver):
    """1 024, 2 048 and 1 025 records: a last chunk that is full (the one that writes the frame's kept count), a workgroup that
    finds the frame ended exactly where it would start, and a chunk of one skipped record"""
    frames = M.multiples_case()
    got = solver.mv_raster(frames)
    M.compare(got, M.multiples_ref(), "multiples")
    assert np.diff(got["rec_ptr"]).tolist() == list(M.MULTIPLES)
    for f in range(3):
        assert M.frame_rows(solver.mv_raster([frames[f]]), 0) == M.frame_rows(got, f), f


def test_1024_frames_with_runs_of_empty_ones(solver):
    """MOVBA_MAX_EXPRESS_IMAGES frames of 16 x 16 to 40 x 40 with 0 to 5 records and 0 to 3 queries: the scan over the frames in all
    16 wavefronts, the tile scan across frames with four tiles per thread, the searches over rec_ptr, q_ptr and g_ptr through runs
    of frames without records, queries or lattice.  kept_ptr in full, every array, and six frames alone against their rows."""
    frames, ref = M.frames_case(), M.frames_ref()
    got = solver.mv_raster(frames)
    assert got["status"] == 0 and len(got["kept_ptr"]) == M.N_FRAMES + 1
    assert np.array_equal(got["kept_ptr"], ref["kept_ptr"]), np.flatnonzero(got["kept_ptr"] != ref["kept_ptr"])[:8].tolist()
    M.compare(got, ref, "frames")
    for f in M.FRAMES_ALONE:
        assert M.frame_rows(solver.mv_raster([frames[f]]), 0) == M.frame_rows(got, f) == M.frame_rows(ref, f), f


def test_the_mixed_call_and_frame_by_frame_independence(solver):
    frames, ref = M.mixed_case(), M.mixed_ref()
    got = solver.mv_raster(frames)
    M.compare(got, ref, "mixed")
    # the I-frame: nothing kept, everything -1, no coverage, the grid forced
    assert got["kept_ptr"][1] == got["kept_ptr"][2] and (got["cand"][got["q_ptr"][1]:got["q_ptr"][2]] == -1).all()
    assert got["cover_px"][1] == 0 and got["coverage_area"][1] == 0.0 and got["force_grid"][1] == 1
    assert not got["grid_covered"][got["grid_ptr"][1]:got["grid_ptr"][2]].any()
    # pointers and padding
    assert np.diff(got["grid_ptr"]).tolist() == [capi.lattice_size(fr["rows"], fr["cols"]) for fr in frames]
    total = got["kept_ptr"][-1]
    assert total < len(got["mv_dindx"]) and (got["mv_dindx"][total:] == -1).all() and (got["kp_rect"][total:] == -1).all() and np.isnan(got["mv_pt"][total:]).all()
    assert np.array_equal(got["mv_dindx"][:total], np.concatenate([np.arange(n) for n in np.diff(got["kept_ptr"])]))
    # each frame alone, and the frames reversed, give the bits of the batch
    want = [M.frame_rows(got, f) for f in range(5)]
    for f in range(5):
        assert M.frame_rows(solver.mv_raster([frames[f]]), 0) == want[f], f
    rev = solver.mv_raster(frames[::-1])
    for pos, f in enumerate(range(4, -1, -1)):
        assert M.frame_rows(rev, pos) == want[f], f


def test_the_coverage_gate_on_its_boundary(solver):
    at = solver.mv_raster(M.gate_case(0.5))
    assert at["cover_px"].tolist() == [2048] and at["coverage_area"].tolist() == [0.5] and at["force_grid"].tolist() == [0]
    above = solver.mv_raster(M.gate_case(float(np.nextafter(0.5, 1))))
    assert above["coverage_area"].tolist() == [0.5] and above["force_grid"].tolist() == [1]
    M.compare(at, M.ref_mv_raster(M.gate_case(0.5)), "gate")


def test_queries_on_and_over_the_edge(solver):
    frames = M.edge_case()
    got = solver.mv_raster(frames)
    M.compare(got, M.ref_mv_raster(frames), "edge")
    q = frames[0]["q_pt"].tolist()
    assert q[:3] == [[-0.5, -0.5], [44.0, 0.0], [0.0, 30.0]]
    assert got["cand"][0].tolist() == [0, 3, -1, -1]                    # pixel (0, 0)
    assert (got["cand"][1:3] == -1).all() and (got["cand"][3:5, 0] >= 0).all() and (got["cand"][5:7] == -1).all()


def _chain_frames():
    """a synthetic image, previous features from advance_ref's generators - random ones and ones that carry the descriptor of
    where a record takes them - and the records of that frame -> (the raster's frame, the advance frame without the raster's part)"""
    rng = np.random.default_rng(21)
    rows, cols = 64, 96
    image = R.edge_image(rng, rows, cols)
    base = A.random_frame(image, rng, 30, n_mv=0, n_kps=0, first_id=7)
    recs = M.random_records(rng, rows, cols, 150, margin=6)
    b = A.Builder(image, 25, 7, 0)
    for sx, sy, dx, dy, w, h in recs[:60]:
        rect = (dx - w // 2, dy - h // 2, w, h)
        if w >= 8 and h >= 8 and R.rejected(rect, rows, cols) == 0 and 0 <= sx < cols and 0 <= sy < rows:
            b.prev.append(dict(pt=(np.float32(sx + 0.25), np.float32(sy + 0.5)), mb=(w, h), age=int(rng.integers(0, 4)), track=2000 + len(b.prev),
                               desc=A.flipped(A.true_desc(image, rect, 25), int(rng.integers(0, 50)), rng), coverage=0, cand=[-1] * 4))
    tracked = b.frame()
    assert len(tracked["prev_age"]) >= 10
    prev = {k: np.concatenate([base[k], tracked[k]]) for k in ("prev_pt", "prev_mb", "prev_age", "prev_track", "prev_desc", "prev_coverage")}
    return M.frame(rows, cols, recs, prev["prev_pt"], threshold=0.6, want_grid=1), dict(image=image, threshold=25, first_id=7, **prev)


def _advance_frame(rest, res):
    """one frame's movba_advance input from a mv_raster result, unchanged"""
    a, b = int(res["kept_ptr"][0]), int(res["kept_ptr"][1])
    return dict(rest, force_grid=int(res["force_grid"][0]), prev_cand=res["cand"], mv_pt=res["mv_pt"][a:b], mv_dindx=res["mv_dindx"][a:b],
                kp_rect=res["kp_rect"][a:b], grid_covered=res["grid_covered"])


def test_the_outputs_chain_into_advance(solver):
    raster, rest = _chain_frames()
    got = solver.mv_raster([raster])
    want = M.ref_mv_raster([raster])
    M.compare(got, want, "chain: the raster")
    through = solver.advance([_advance_frame(rest, got)])
    ref = A.ref_advance([_advance_frame(rest, want)])
    A.compare(through, ref, "chain: the walk")
    assert (through["fate"] == A.ADV_KEPT).sum() >= 5 and (ref["kp_found"] != 0).any() and got["grid_covered"].any()


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        for name, case, ref in (("full", M.full_case, M.full_ref), ("counts", M.counts_case, M.counts_ref), ("mixed", M.mixed_case, M.mixed_ref)):
            M.compare(s.mv_raster(case(), pinned=True), s.mv_raster(case()), name + ", pinned")
            M.compare(s.mv_raster(case(), pinned=True), ref(), name + ", pinned against the restatement")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """A solved window's download before and after a call is bit-identical, later runs too; and the call gives after a solve,
    after a reset and between upload and run what it gives on a fresh handle."""
    w = synth.cfg("small")
    frames = M.mixed_case()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")
    s = built_lib.Solver()
    try:
        first = s.solve(w)
        before = s.download()
        M.compare(s.mv_raster(frames), M.mixed_ref(), "after the solve")
        after = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(first[k]), np.asarray(before[k])) and np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
        assert s._L.movba_lba_reset(s._h) == 0
        M.compare(s.mv_raster(frames, pinned=True), M.mixed_ref(), "after the reset, pinned")
        s.run()
        again = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(again[k]), np.asarray(first[k])), k
        s.upload(w)
        M.compare(s.mv_raster(frames), M.mixed_ref(), "between upload and run")
        s.run()
        fresh = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(fresh[k]), np.asarray(first[k])), k
    finally:
        s.close()


def test_a_refusal_and_an_empty_call_on_a_live_handle(solver):
    frames = M.mixed_case()
    d, keep = capi.mv_raster_desc(frames)
    keep["w"][3] = 12                                           # one block width that is none of 4, 8, 16
    r, out = capi.mv_raster_result(d.n_frames, len(keep["src_x"]), len(keep["q_pt"]), keep["n_grid"],
                                   alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
    r.status = 99
    assert solver._L.movba_mv_raster(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    bad = dict(frames[0], records=dict(frames[0]["records"], ref=np.ones(len(frames[0]["records"]["w"]), np.int32)))
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.mv_raster([bad])
    # no frames: MOVBA_OK, and not one result entry is written
    d.n_frames = 0
    r.status = 99
    assert solver._L.movba_mv_raster(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    assert solver.mv_raster([])["status"] == 0
    # frames without anything
    none = M.frame(12, 12, [], [])
    got = solver.mv_raster([none, none])
    M.compare(got, M.ref_mv_raster([none, none]), "frames without records and queries")
    assert got["kept_ptr"].tolist() == [0, 0, 0] and got["force_grid"].tolist() == [1, 1]
    M.compare(solver.mv_raster(frames), M.mixed_ref(), "after the refusal")
