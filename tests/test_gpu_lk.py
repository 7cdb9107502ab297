"""movba_lk_track on the device against the restatement of tests/lk_ref.py, every comparison exact equality, bit for bit: every
frame size and window at which the level rule changes (96 x 80 and 80 x 96 with windows 21 and 31, 40 x 36 with 31, 200 x 168 and
200 x 169, 96 x 88, windows 3 and 5), with points whose window hangs over each edge and corner by up to the window and one
beyond; every exit of the walk - the flat patch, eps, all iterations, the oscillation, out of bounds at the start and inside the
loop, and upper levels that fail while the walk goes on; 0, 1, 63, 64, 65 and 4 097 points in a frame; 1 024 tiny frames with runs
of empty ones; fractions that make rint tie; a frame alone against the same frame in a batch; pinned numbers; pinned result
memory; a solved window on the same handle left as it was; a refusal and an empty call on a live handle; and the coverage
features out of Solver.advance tracked by Solver.lk_track.  (tests/test_lk_cpu.py holds the library's steps to the same cases
under AddressSanitizer first, and checks that the cases are what is said here.)"""
import ctypes as C

import numpy as np
import pytest

import advance_ref as A
import lk_ref as K
from movba import capi, synth

pytestmark = pytest.mark.gpu


def test_every_level_rule_window_and_edge(solver):
    frames = K.sizes_case()
    got = solver.lk_track(frames)
    assert got["status"] == 0
    K.compare(got, K.sizes_ref(), "sizes")
    K.compare(solver.lk_track(frames), got, "the same call twice")


def test_every_exit_of_the_walk(solver):
    got = solver.lk_track(K.exits_case())
    K.compare(got, K.exits_ref(), "exits")
    assert {K.EPS, K.OSCILLATION, K.MAX_ITER_RAN, K.REJ_MIN_EIG} <= set(got["exit_code"].tolist())
    # other parameters than the reference's: level 0 alone, two iterations, a tight eps, a high threshold
    for params in (dict(max_level=0), dict(max_level=1, max_iter=2), dict(eps=1e-3, max_iter=30), dict(min_eig_threshold=0.05)):
        K.compare(solver.lk_track(K.exits_case(), **params), K.ref_lk(K.exits_case(), **params), f"exits, {params}")


def test_partly_filled_waves_and_workgroups(solver):
    got = solver.lk_track(K.counts_case())
    K.compare(got, K.counts_ref(), "counts")
    assert np.diff(got["pt_ptr"]).tolist() == list(K.COUNTS)


def test_1024_frames_with_runs_of_empty_ones(solver):
    frames = K.frames_case()
    got = solver.lk_track(frames)
    K.compare(got, K.frames_ref(), "frames")
    for f in K.FRAMES_ALONE:
        K.compare(solver.lk_track([frames[f]]), K.frame_part(K.frames_ref(), f), f"frames, frame {f} alone")


def test_fractions_that_make_rint_tie(solver):
    K.compare(solver.lk_track(K.tie_case()), K.tie_ref(), "tie")


def test_a_frame_alone_equals_the_frame_in_a_batch(solver):
    frames, ref = K.sizes_case(), K.sizes_ref()
    for f in range(len(frames)):
        K.compare(solver.lk_track([frames[f]]), K.frame_part(ref, f), f"sizes, frame {f} alone")
    # the other way round and in another order: the result follows the frame
    mixed = [frames[6], K.exits_case()[0], frames[1]]
    got = solver.lk_track(mixed)
    K.compare(K.frame_part(got, 0), K.frame_part(ref, 6), "frame 6 first")
    K.compare(K.frame_part(got, 1), K.frame_part(K.exits_ref(), 0), "exits second")
    K.compare(K.frame_part(got, 2), K.frame_part(ref, 1), "frame 1 third")


def test_pinned_numbers(solver):
    """what the restatement gave when the cases were written, so that a change of both sides at once is seen"""
    got = solver.lk_track(K.sizes_case())
    for key, value in K.PINNED.items():
        assert K.digest(got)[key] == value, key


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        for name, case, ref in (("sizes", K.sizes_case, K.sizes_ref), ("counts", K.counts_case, K.counts_ref), ("exits", K.exits_case, K.exits_ref)):
            K.compare(s.lk_track(case(), pinned=True), s.lk_track(case()), name + ", pinned")
            K.compare(s.lk_track(case(), pinned=True), ref(), name + ", pinned against the restatement")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """A solved window's download before and after a call is bit-identical, later runs too; and the call gives after a solve,
    after a reset and between upload and run what it gives on a fresh handle."""
    w = synth.cfg("small")
    frames = K.exits_case()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")
    s = built_lib.Solver()
    try:
        first = s.solve(w)
        before = s.download()
        K.compare(s.lk_track(frames), K.exits_ref(), "after the solve")
        after = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(first[k]), np.asarray(before[k])) and np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
        assert s._L.movba_lba_reset(s._h) == 0
        K.compare(s.lk_track(frames, pinned=True), K.exits_ref(), "after the reset, pinned")
        s.run()
        again = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(again[k]), np.asarray(first[k])), k
        s.upload(w)
        K.compare(s.lk_track(frames), K.exits_ref(), "between upload and run")
        s.run()
        fresh = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(fresh[k]), np.asarray(first[k])), k
    finally:
        s.close()


def test_a_refusal_and_an_empty_call_on_a_live_handle(solver):
    frames = K.exits_case()
    d, keep = capi.lk_desc(frames)
    keep["win"][0] = 20                                         # an even window
    r, out = capi.lk_result(d.n_frames, len(keep["pt"]), alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
    r.status = 99
    assert solver._L.movba_lk_track(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.lk_track([dict(frames[0], win=97)])
    # no frames: MOVBA_OK, and not one result entry is written
    d.n_frames = 0
    r.status = 99
    assert solver._L.movba_lk_track(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
    assert solver.lk_track([])["status"] == 0
    # frames without points, with and without images
    none = [dict(frames[0], pt=np.zeros((0, 2), np.float32)), dict(prev=None, next=None, rows=30, cols=40, win=21, pt=np.zeros((0, 2), np.float32))]
    got = solver.lk_track(none)
    assert got["status"] == 0 and got["kept_ptr"].tolist() == [0, 0, 0] and len(got["kept_src"]) == 0
    K.compare(solver.lk_track(frames), K.exits_ref(), "after the refusal")


def test_the_coverage_features_of_advance_chain_into_lk_track(solver):
    """MOVExtractor.cc:337-377: the features movba_advance hands back as MOVBA_ADV_COVERAGE are the points of the P-frame's LK
    call (window 31); keep is the gate of :354"""
    rng = np.random.default_rng(33)
    rows, cols = 64, 96
    prev, nxt = K.texture(rows, cols, 90, (0, 0), 2), K.texture(rows, cols, 90, (-12, 9), 2)
    fr = A.random_frame(nxt, rng, 160)
    walk = solver.advance([fr])
    A.compare(walk, A.ref_advance([fr]), "chain: the walk")
    cov = np.nonzero(walk["fate"] == A.ADV_COVERAGE)[0]
    assert len(cov) >= 5 and np.array_equal(cov, np.nonzero(fr["prev_coverage"])[0])
    lk = [dict(prev=prev, next=nxt, win=31, pt=fr["prev_pt"][cov])]
    got = solver.lk_track(lk)
    want = K.ref_lk(lk)
    K.compare(got, want, "chain: the track")
    assert 0 < got["keep"].sum() and got["kept_ptr"].tolist() == [0, int(want["keep"].sum())]
    assert np.array_equal(got["kept_src"][:got["kept_ptr"][1]], np.nonzero(want["keep"])[0])
