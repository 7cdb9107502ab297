"""movba_advance on the device against the restatements of tests/advance_ref.py, every comparison exact equality: the mixed call
array by array, padding included; previous-feature counts that leave waves and workgroups partly filled and the sort's padding
at work; the bound of 16384 features; the sizes at which the sums and scans that only the device runs take a second pass - 1 024
frames, the bound's frame behind three small ones, 300 macroblocks and 266 lattice rects in one frame; the mov_cnt trio of 59,
60 and 60 + force_grid; independence of a frame from the other
frames, from how the frames are split over calls and from pixels none of its items read, and what a permutation of a frame's
features may change; pinned results; a solved window on the same handle left as it was; a refusal and an empty call on a live
handle.  Every rect the device reads is inside its image by the reference's own test (tests/test_advance_cpu.py holds the
library's steps to the same cases under AddressSanitizer first)."""
import ctypes as C

import numpy as np
import pytest

import advance_ref as A
import express_ref as R
from movba import capi, synth

pytestmark = pytest.mark.gpu


def test_parity_with_the_restatement_on_the_mixed_call(solver):
    frames, _ = A.mixed_case()
    got = solver.advance(frames)
    assert got["status"] == 0
    A.compare(got, A.mixed_ref(), "mixed")
    A.compare(solver.advance(frames), got, "the same call twice")
    # grid_ptr left out: nothing is covered
    bare = [dict(fr, grid_covered=None) for fr in frames]
    A.compare(solver.advance(bare), A.ref_advance(bare, literal=False), "no grid_covered")


def test_counts_that_leave_waves_and_workgroups_partly_filled(solver):
    """0, 1, 63, 64, 65, 257 and 1000 previous features per frame on a 64 x 96 image, ages from 3 values"""
    got = solver.advance(A.counts_case())
    A.compare(got, A.counts_ref(), "counts")
    assert np.diff(got["prev_ptr"]).tolist() == list(A.COUNTS)


def test_the_bound_of_previous_features(solver):
    """16384 previous features in one frame against the vectorised restatement, and against the literal one on the first 500
    positions"""
    got = solver.advance(A.bound_case())
    A.compare(got, A.bound_ref(), "bound")
    A.compare_head(got)
    assert len(got["order"]) == capi.MAX_ADVANCE_PREV and sorted(got["order"].tolist()) == list(range(16384))


def test_1024_frames_take_the_sum_of_the_emit_over_every_pass(solver):
    """MOVBA_MAX_EXPRESS_IMAGES frames of 0 to 4 previous features, 0 to 3 macroblocks and 0 to 3 vectors, frames without anything
    first, last and in the middle: k_adv_emit's sum over the 3 x 1 024 counts, which only the device runs, in 12 passes of its
    stride.  seg_ptr in full, every array, and six frames alone against their rows."""
    frames, ref = A.frames_case(), A.frames_ref()
    got = solver.advance(frames)
    assert got["status"] == 0 and len(got["seg_ptr"]) == 4 * A.N_FRAMES + 1
    assert np.array_equal(got["seg_ptr"], ref["seg_ptr"]), np.flatnonzero(got["seg_ptr"] != ref["seg_ptr"])[:8].tolist()
    A.compare(got, ref, "frames")
    for f in A.FRAMES_ALONE:
        assert A.frame_rows(solver.advance([frames[f]]), 0) == A.frame_rows(got, f) == A.frame_rows(ref, f), f


def test_the_bound_frame_behind_three_small_ones(solver):
    """the 16 384 features of the bound case as the last of four frames: k_adv_emit's workgroups per frame follow the average
    frame, so the frame's items take four passes of the strided loop instead of one"""
    frames = A.behind_case()
    got = solver.advance(frames)
    A.compare(got, A.behind_ref(), "behind")
    A.compare_head(A.frame_part(got, 3))
    assert A.frame_rows(got, 3) == A.frame_rows(solver.advance(A.bound_case()), 0)


def test_two_macroblocks_and_two_lattice_rects_per_thread(solver):
    """two frames of 240 x 320 with 300 macroblocks and the lattice of 266 rects: k_adv_resolve's scans over both give a thread
    two entries.  The first frame emits its lattice (force_grid), the second has 60 new features and more and emits none."""
    frames, ref = A.lattice_case(), A.lattice_ref()
    got = solver.advance(frames)
    A.compare(got, ref, "lattice")
    assert got["grid_ran"].tolist() == [1, 0] and got["seg_ptr"][3] > got["seg_ptr"][2] and got["seg_ptr"][7] == got["seg_ptr"][6]
    for f in range(2):
        assert A.frame_rows(solver.advance([frames[f]]), 0) == A.frame_rows(got, f), f


def test_the_mov_cnt_trio(solver):
    got = solver.advance(A.trio_case())
    A.compare(got, A.trio_ref(), "trio")
    assert got["mov_cnt"].tolist() == [59, 60, 60] and got["grid_ran"].tolist() == [1, 0, 1]


def test_a_frame_depends_on_its_own_data_alone(built_lib):
    frames, _ = A.mixed_case()
    nf = len(frames)
    s = built_lib.Solver()
    try:
        whole = s.advance(frames)
        A.compare(whole, A.mixed_ref(), "whole")
        want = [A.frame_rows(whole, f) for f in range(nf)]
        # frames reversed
        rev = s.advance(frames[::-1])
        for pos, f in enumerate(range(nf - 1, -1, -1)):
            assert A.frame_rows(rev, pos) == want[f], f
        # one call per frame
        for f in range(nf):
            assert A.frame_rows(s.advance([frames[f]]), 0) == want[f], f
        # a frame's features permuted: exactly what the restatement says for the permuted input; and where the permutation
        # keeps the members of every tie (equal age and count) in their order, the same kept features
        fr = frames[0]
        n = len(fr["prev_age"])
        rng = np.random.default_rng(3)
        keys = ("prev_pt", "prev_mb", "prev_age", "prev_track", "prev_desc", "prev_coverage", "prev_cand")
        anyhow = rng.permutation(n)                             # (new index -> old index)
        gentle = anyhow.copy()
        ties = {}
        for i in range(n):
            ties.setdefault((int(fr["prev_age"][i]), A.popcount(R.as_int(fr["prev_desc"][i]))), []).append(i)
        for members in ties.values():
            slots = np.flatnonzero(np.isin(gentle, members))
            gentle[slots] = members                             # (both ascending)
        assert not np.array_equal(gentle, anyhow) and not np.array_equal(gentle, np.arange(n))
        for label, perm in (("any", anyhow), ("ties kept", gentle)):
            moved = dict(fr, **{k: np.ascontiguousarray(fr[k][perm]) for k in keys})
            got = s.advance([moved])
            A.compare(got, A.ref_advance([moved]), "permuted: " + label)
            if label == "ties kept":
                assert np.array_equal(perm[got["order"]], whole["order"][:n])
                seg, seg0 = got["seg_ptr"], whole["seg_ptr"]
                for key in A.FEAT:
                    assert np.array_equal(got[key][:seg[1]], whole[key][:seg0[1]]), key
        # a pixel outside everything the frame's items read changes nothing
        fr = frames[1]
        read = A.read_pixels(fr)
        rows, cols = fr["image"].shape
        free = [(y, x) for y in range(rows) for x in range(cols) if (y, x) not in read]
        assert len(free) >= 2
        changed = fr["image"].copy()
        for y, x in free:
            changed[y, x] ^= 0xFF
        assert A.frame_rows(s.advance([dict(fr, image=changed)]), 0) == want[1]
        # ... and pixels they read do: a checkerboard over the block of the frame's first kept feature
        o = whole["seg_ptr"][4]
        assert whole["seg_ptr"][5] > o
        x, y, w, h = (int(v) for v in whole["feat_rect"][o])
        changed = fr["image"].copy()
        changed[y:y + h, x:x + w + 1] = np.where(np.add.outer(np.arange(h), np.arange(w + 1)) % 2 == 0, 0, 255)
        after = s.advance([dict(fr, image=changed)])
        assert A.frame_rows(after, 0) != want[1]
        A.compare(after, A.ref_advance([dict(fr, image=changed)]), "changed image")
    finally:
        s.close()


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        frames, _ = A.mixed_case()
        A.compare(s.advance(frames, pinned=True), s.advance(frames), "pinned")
        A.compare(s.advance(frames, pinned=True), A.mixed_ref(), "pinned against the restatement")
        A.compare(s.advance(A.counts_case(), pinned=True), A.counts_ref(), "counts, pinned")
        A.compare(s.advance(A.trio_case(), pinned=True), A.trio_ref(), "trio, pinned")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """A solved window's download before and after an advance call is bit-identical, later runs too; and the call gives after a
    solve, after a reset and between upload and run what it gives on a fresh handle."""
    w = synth.cfg("small")
    frames, _ = A.mixed_case()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")
    s = built_lib.Solver()
    try:
        first = s.solve(w)
        before = s.download()
        A.compare(s.advance(frames), A.mixed_ref(), "after the solve")
        after = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(first[k]), np.asarray(before[k])) and np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
        assert s._L.movba_lba_reset(s._h) == 0
        A.compare(s.advance(frames, pinned=True), A.mixed_ref(), "after the reset, pinned")
        s.run()
        again = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(again[k]), np.asarray(first[k])), k
        s.upload(w)
        A.compare(s.advance(frames), A.mixed_ref(), "between upload and run")
        s.run()
        fresh = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(fresh[k]), np.asarray(first[k])), k
    finally:
        s.close()


def test_a_refusal_and_an_empty_call_on_a_live_handle(solver):
    frames, _ = A.mixed_case()
    d, keep = capi.advance_desc(frames)
    keep["prev_mb"][3, 0] = 12                                  # one macroblock width that is neither 8 nor 16
    r, out = capi.advance_result(d.n_frames, len(keep["prev_age"]), len(keep["kp_rect"]), keep["n_grid"],
                                 alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
    r.status = 99
    assert solver._L.movba_advance(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.advance([dict(frames[0], first_id=-1)])
    # no frames: MOVBA_OK, and not one result entry is written
    d.n_frames = 0
    r.status = 99
    assert solver._L.movba_advance(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    assert solver.advance([])["status"] == 0
    # frames without anything: counts and pointers of an empty walk
    none = A.random_frame(R.flat_image(12, 12, 128), np.random.default_rng(0), 0, n_mv=0, n_kps=0, first_id=41)
    got = solver.advance([none, none])
    A.compare(got, A.ref_advance([none, none]), "frames without items")
    assert got["next_id"].tolist() == [41, 41] and got["seg_ptr"].tolist() == [0] * 9 and got["grid_ran"].tolist() == [1, 1]
    A.compare(solver.advance(frames), A.mixed_ref(), "after the refusal")
