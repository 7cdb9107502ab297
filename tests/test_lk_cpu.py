"""movba_lk_track without a GPU: the two restatements the GPU tests compare against (tests/lk_ref.py) held equal - the loops walk
every point of the small cases and a sample of the large ones, and the pyramids pixel by pixel - and the conditions the cases
must meet before any device comparison, among them that every exit of the walk occurs; the restatement against ground truth
that does not come from it; the symbol, the struct layouts and every refusal of the header through the built library (the checks
run before the handle is touched); the library's own steps on the CPU (tests/lk/lk_main.cpp, under AddressSanitizer +
UndefinedBehaviorSanitizer) against the restatement, exact; and the host side of the call - checks, layout, packing of strided
rows, copy-out, pinned and ordinary results, a handle shared with a window, two handles on two threads - under the sanitizers
(tests/lk: a stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its own).  No sanitizer touches
code loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lk_ref as K
from conftest import ROOT

LK_DIR = os.path.join(ROOT, "tests", "lk")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
CASES = dict(sizes=(K.sizes_case, K.sizes_ref), exits=(K.exits_case, K.exits_ref), counts=(K.counts_case, K.counts_ref),
             frames=(K.frames_case, K.frames_ref), tie=(K.tie_case, K.tie_ref))
ALONE = dict(frames=K.FRAMES_ALONE, counts=(1, 2, 5))           # the frames run alone too; every frame where nothing is said
POINT_KEYS = ("next_pt", "pt_status", "err", "exit_code", "keep")


# ---- the restatements and their cases ------------------------------------------------------------------------------------------

def _same(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype == np.float32 else (a == b).all()


def _hold_equal(fr, ref, first, which, label, **params):
    lit = K.ref_lk_literal(fr, which, **params)
    for key in POINT_KEYS:
        assert lit[key].dtype == ref[key].dtype and _same(lit[key], ref[key][first + np.asarray(which, np.int64)]), (label, key)


def test_the_two_restatements_agree():
    """The loops take about 50 ms per point of a 21 x 21 window: every 5th point of sizes_case (every edge point's kind and every
    frame among them), every point of exits_case and tie_case, every 97th of the 4 097, the first 150 tiny frames."""
    frames, ref = K.sizes_case(), K.sizes_ref()
    for f, fr in enumerate(frames):
        _hold_equal(fr, ref, int(ref["pt_ptr"][f]), list(range(f % 5, len(fr["pt"]), 5)), f"sizes, frame {f}")
    _hold_equal(K.exits_case()[0], K.exits_ref(), 0, list(range(len(K.exits_case()[0]["pt"]))), "exits")
    _hold_equal(K.exits_case()[1], K.exits_ref(), int(K.exits_ref()["pt_ptr"][1]), [0, 1, 2], "exits, the fine frame")
    for params in (dict(max_level=0), dict(max_level=1, max_iter=2), dict(eps=1e-3, max_iter=30), dict(min_eig_threshold=0.05)):
        _hold_equal(K.exits_case()[0], K.ref_lk(K.exits_case(), **params), 0, list(range(0, 83, 4)), f"exits, {params}", **params)
    _hold_equal(K.tie_case()[0], K.tie_ref(), 0, [0, 1], "tie")
    frames, ref = K.counts_case(), K.counts_ref()
    _hold_equal(frames[5], ref, int(ref["pt_ptr"][5]), list(range(0, 4097, 97)), "counts, the large frame")
    _hold_equal(frames[3], ref, int(ref["pt_ptr"][3]), list(range(64)), "counts, 64 points")
    frames, ref = K.frames_case(), K.frames_ref()
    for f in range(150):
        if len(frames[f]["pt"]):
            _hold_equal(frames[f], ref, int(ref["pt_ptr"][f]), list(range(len(frames[f]["pt"]))), f"frames, frame {f}")


def test_the_pyramids_agree_pixel_by_pixel():
    for fr in (K.sizes_case()[0], K.sizes_case()[6], K.sizes_case()[8], K.frames_case()[5]):
        for img in (fr["prev"], fr["next"]):
            level = img
            for _ in range(len(K.level_sizes(img.shape[0], img.shape[1], fr["win"], 3)) - 1):
                a, b = K.pyr_down(level), K.pyr_down_literal(level)
                assert a.dtype == np.uint8 and np.array_equal(a, b)
                level = a
    # an odd and an even side, and a constant image stays constant (the kernel sums to 256)
    assert K.pyr_down(np.full((7, 10), 201, np.uint8)).tolist() == np.full((4, 5), 201).tolist()


def test_the_restatement_recovers_a_known_shift():
    """Ground truth that does not come from the restatement: six sinusoids sampled analytically at x and at x - shift (8-bit
    rounding included), 25 points, window 21, the reference's parameters, shifts of 0.3 to 6 pixels in several directions.  The
    bound cannot be derived here.  Measured on this CPU when the test was written: worst error 0.0209 px (at the shift (-4.25,
    -4.25)), every point tracked with status 1; the assertion is twice that, 0.0418 px."""
    worst = 0.0
    for shift in ((0.3, 0.0), (0.0, -0.3), (0.7, 0.4), (-1.5, 1.0), (2.25, -2.75), (3.0, 3.0), (-4.2, 4.3), (6.0, 0.0), (0.0, 6.0), (-4.25, -4.25)):
        fr = K.shift_truth_case(shift)
        res = K.ref_lk([fr])
        assert res["pt_status"].all() and res["keep"].all()
        worst = max(worst, float(np.abs(res["next_pt"].astype(np.float64) - fr["pt"].astype(np.float64) - np.array(shift)).max()))
    print("worst error of the recovered shift: %.4f px" % worst)
    assert worst <= 0.0418


def test_sizes_case_is_what_the_gpu_tests_ask_for():
    frames, ref = K.sizes_case(), K.sizes_ref()
    assert [(fr["prev"].shape[0], fr["prev"].shape[1], fr["win"]) for fr in frames] == [s[:3] for s in K.SIZES]
    assert [len(K.level_sizes(r, c, w, 3)) - 1 for r, c, w, _ in K.SIZES] == [s[3] for s in K.SIZES]
    assert {s[3] for s in K.SIZES} == {0, 1, 2, 3}
    assert K.level_sizes(200, 168, 21, 3)[-1] == (50, 42) and K.level_sizes(200, 169, 21, 3)[-1] == (25, 22)     # 21 is not above 21
    assert K.level_sizes(96, 80, 21, 3)[-1] == (48, 40) and K.level_sizes(96, 88, 21, 3)[-1] == (24, 22)
    assert K.level_sizes(200, 169, 21, 2)[-1] == (50, 43)                                   # max_level cuts it
    for f, fr in enumerate(frames):
        rows, cols, win = fr["prev"].shape[0], fr["prev"].shape[1], fr["win"]
        half = (win - 1) / 2
        a, b = int(ref["pt_ptr"][f]), int(ref["pt_ptr"][f + 1])
        assert b - a == 64 + K.SIZES_RANDOM
        pt, code, status = fr["pt"].astype(np.float64), ref["exit_code"][a:b], ref["pt_status"][a:b]
        ip = np.floor(pt - half)
        # the window's corner at -win (hanging over by the whole window) is inside the bounds, one further is not; the same at the
        # far side with the corner on the last pixel and one behind it; every combination of the two axes: edges and corners
        assert set(np.unique(ip[:64, 0]).tolist()) >= {-win, -win - 1, 0, cols - 1, cols} and set(np.unique(ip[:64, 1]).tolist()) >= {-win, -win - 1, 0, rows - 1, rows}
        out = (ip[:, 0] < -win) | (ip[:, 0] >= cols) | (ip[:, 1] < -win) | (ip[:, 1] >= rows)
        assert (code[out] == K.REJ_START).all() and (code[~out] != K.REJ_START).all() and out.sum() == 28
        assert (status[out] == 0).all() and (ref["err"][a:b][out] == 0).all()
        for cx in (-win, cols - 1):
            for cy in (-win, rows - 1):
                assert ((ip[:, 0] == cx) & (ip[:, 1] == cy)).any()
    # points that track: the content moved by (1.25, -0.75)
    good = ref["exit_code"] == K.EPS
    flow = ref["next_pt"][good] - np.concatenate([fr["pt"] for fr in frames])[good]
    assert good.sum() > 60 and np.abs(np.median(flow, axis=0) - np.array([1.25, -0.75])).max() < 0.05
    assert 0 < ref["keep"].sum() < len(ref["keep"]) and ((ref["pt_status"] == 1) & (ref["keep"] == 0)).any()        # tracked to outside the image
    assert ref["kept_ptr"][-1] == ref["keep"].sum() and (ref["kept_src"][ref["kept_ptr"][-1]:] == -1).all()
    assert K.digest(ref) == K.PINNED


def test_every_exit_occurs_in_the_committed_cases():
    """From the exit codes of the restatement: the flat patch, eps, all iterations and the oscillation in exits_case itself -
    the oscillation occurs naturally, under the heavy noise of the next image's left strip - and both bounds exits in sizes_case.
    An upper level that fails while the walk goes on: by the matrix test (the flat points of exits_case fail at levels 1 and 0
    after level 2, where the rect is smaller than the window, has run; the points of exits_case's second frame fail at level 1,
    where its fine rows have no derivative, and are tracked at level 0), and by the bounds inside the loop.  A START test that fails at an upper level ONLY cannot occur under the header's rules: floor(pt / 2 - half) >= (cols +
    1) / 2 needs pt >= cols + 2 half, while level 0 needs pt < cols + half + 1; and floor(pt / 2 - half) < -win needs pt < -win -
    1, level 0 pt >= -(win + 1) / 2.  A loop that leaves the bounds at an upper level stores a point that, doubled, is outside
    level 0's bounds as well, so such a point ends at level 0 with MOVBA_LK_REJ_MIN_EIG or, after level 0 has formed its own
    matrix and passed its test, which err shows, with MOVBA_LK_REJ_LOOP."""
    ref = K.exits_ref()
    codes, up = ref["exit_code"], ref["level_exit"]
    assert {K.EPS, K.OSCILLATION, K.MAX_ITER_RAN, K.REJ_MIN_EIG} <= set(codes.tolist())
    assert (codes[:3] == K.REJ_MIN_EIG).all() and (ref["pt_status"][:3] == 0).all() and (ref["err"][:3] == 0).all()
    # (the flat rect is 25 x 25 at level 1, still larger than the window and its Scharr ring, and 12 x 12 at level 2, where the loop ran)
    assert (up[:3, 1] == K.LEVEL_MIN_EIG).all() and (up[:3, 2] < 16).all()
    assert (codes[3:23] == K.EPS).sum() >= 15
    flow = ref["next_pt"][3:23][codes[3:23] == K.EPS] - K.exits_case()[0]["pt"][3:23][codes[3:23] == K.EPS]
    assert np.abs(np.median(flow, axis=0) - np.array([2.5, 1.25])).max() < 0.05
    everything = set()
    for name in CASES:
        everything |= set(CASES[name][1]()["exit_code"].tolist())
    assert everything == {K.EPS, K.OSCILLATION, K.MAX_ITER_RAN, K.REJ_START, K.REJ_MIN_EIG, K.REJ_LOOP}
    # the fine frame: level 1 fails the matrix test, level 0 tracks the edge's pixel
    fine = slice(int(K.exits_ref()["pt_ptr"][1]), int(K.exits_ref()["pt_ptr"][2]))
    assert (up[fine, 1] == K.LEVEL_MIN_EIG).all() and (codes[fine] < 16).all() and ref["pt_status"][fine].all() and (ref["err"][fine] > 1e-4).all()
    assert np.abs(ref["next_pt"][fine][:, 0] - K.exits_case()[1]["pt"][:, 0] - 1).max() < 0.2
    ref = K.sizes_ref()
    codes, up = ref["exit_code"], ref["level_exit"]
    gone = ((up[:, 1] == K.REJ_LOOP) | (up[:, 2] == K.REJ_LOOP)) & (up[:, 0] != K.LEVEL_START)
    assert gone.sum() >= 5 and np.isin(codes[gone], (K.REJ_MIN_EIG, K.REJ_LOOP)).all() and (ref["pt_status"][gone] == 0).all()
    assert (codes[gone] == K.REJ_LOOP).sum() >= 3 and (ref["err"][gone & (codes == K.REJ_LOOP)] > 1e-4).all()
    assert (up[:, 3] != 0).any()                                          # level 3 is reached
    # tighter and looser parameters move points between the exits
    assert (K.ref_lk(K.exits_case(), eps=1e-3, max_iter=30)["exit_code"] == K.OSCILLATION).sum() > (K.exits_ref()["exit_code"] == K.OSCILLATION).sum()
    assert (K.ref_lk(K.exits_case(), max_level=1, max_iter=2)["exit_code"] == K.MAX_ITER_RAN).sum() > 20


def test_counts_frames_and_tie_cases_are_what_the_gpu_tests_ask_for():
    frames, ref = K.counts_case(), K.counts_ref()
    assert tuple(len(fr["pt"]) for fr in frames) == K.COUNTS == (0, 1, 63, 64, 65, 4097)
    big = ref["keep"][ref["pt_ptr"][5]:]
    assert len(big) == 4097 and all(0 < big[c:c + 1024].sum() < 1024 for c in range(0, 4096, 1024))          # kept and not, in every chunk of k_lk_keep
    assert ref["kept_ptr"][0] == ref["kept_ptr"][1] == 0 and (np.diff(ref["kept_ptr"])[2:] > 0).all()
    frames, ref = K.frames_case(), K.frames_ref()
    assert len(frames) == K.N_FRAMES == 1024
    n = np.diff(ref["pt_ptr"])
    assert n.min() == 0 and n.max() == 3 and n[0] == n[1] == n[2] == n[-1] == 0 and (n[66:76] == 0).all() and (n[126:131] == 0).all()
    assert n[65] > 0 and n[76] > 0 and n[125] > 0 and n[131] > 0        # a run inside wavefront 1 and one across wavefronts 1 and 2
    assert any(fr["prev"] is None for fr in frames) and any(fr["prev"] is not None and not len(fr["pt"]) for fr in frames)
    kept = np.diff(ref["kept_ptr"])
    assert all((kept[64 * w:64 * (w + 1)] > 0).any() for w in range(16)) and ((kept == 0) & (n > 0)).any() and (kept < n).any()
    assert K.FRAMES_ALONE == (0, 63, 64, 65, 511, 1023) and all(n[f] == 2 for f in K.FRAMES_ALONE[1:5])
    assert all(6 <= fr["prev"].shape[0] <= 11 and 6 <= fr["prev"].shape[1] <= 11 for fr in frames if fr["prev"] is not None)
    # the tie
    x, y = (np.float32(v) for v in K.TIE_POINT)
    p = np.float32(y) - np.float32(15)
    b = p - np.floor(p)
    assert float(y) == 20.5 + 2.0 ** -15 and float(b) == 0.5 + 2.0 ** -15 and float(x) == 40.0
    lo, hi = (np.float32(1) - b) * np.float32(16384), b * np.float32(16384)
    assert float(lo) == 8191.5 and float(hi) == 8192.5 and np.rint(lo) == 8192 and np.rint(hi) == 8192
    assert K._weights(np.zeros(1, np.float32), np.array([b]))[0][0] == 8192 and K._w_literal(np.float32(0), b) == (8192, 0, 8192, 0)
    assert K.tie_ref()["pt_status"].all()


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_lk_track")
    assert "movba_lk_track" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_lk_desc", built_lib.LkDesc), ("movba_lk_result", built_lib.LkResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d %d %d %d %d %d %d %d %d\\n", MOVBA_LK_MAX_WIN, MOVBA_LK_MAX_LEVEL, MOVBA_LK_MAX_ITER, MOVBA_LK_MAX_PIXELS, MOVBA_LK_EPS, '
            'MOVBA_LK_OSCILLATION, MOVBA_LK_MAX_ITER_RAN, MOVBA_LK_REJ_START, MOVBA_LK_REJ_MIN_EIG, MOVBA_LK_REJ_LOOP);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.LkDesc, built_lib.LkResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.LkDesc) == 96 and C.sizeof(built_lib.LkResult) == 64
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    assert "} movba_lk_desc;   /* 96 bytes */" in hdr and "} movba_lk_result; /* 64 bytes */" in hdr
    assert rows[2] == [built_lib.LK_MAX_WIN, built_lib.LK_MAX_LEVEL, built_lib.LK_MAX_ITER, built_lib.LK_MAX_PIXELS, built_lib.LK_EPS, built_lib.LK_OSCILLATION,
                       built_lib.LK_MAX_ITER_RAN, built_lib.LK_REJ_START, built_lib.LK_REJ_MIN_EIG, built_lib.LK_REJ_LOOP]
    assert rows[2][4:] == [K.EPS, K.OSCILLATION, K.MAX_ITER_RAN, K.REJ_START, K.REJ_MIN_EIG, K.REJ_LOOP]
    for phrase in ("[opencv-upstream]", "the exact sum is the one place where the call is more definite than", "What stays with the caller"):
        assert phrase in hdr[hdr.index("Sparse pyramidal Lucas-Kanade"):]


def _small_case():
    rng = np.random.default_rng(4)

    def pts(rows, cols, n):
        return np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)], axis=1)

    return [K.frame(30, 34, 5, pts(30, 34, 5), seed=1), K.frame(20, 52, 7, pts(20, 52, 4), seed=2), dict(prev=None, next=None, rows=25, cols=25, win=3, pt=np.zeros((0, 2))),
            K.frame(40, 40, 31, pts(40, 40, 3), seed=3)]


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L_ = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.lk_desc(_small_case())
        r, out = built_lib.lk_result(d.n_frames, len(keep["pt"]), alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
        r.status = 99
        if mutate:
            mutate(d, keep, r)
        rc = L_.movba_lk_track(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    def par(field, value):
        return lambda d, keep, r: setattr(d, field, value)

    refusals = {
        "negative n_frames": par("n_frames", -1), "n_frames above the bound": par("n_frames", 1025),
        "pt_ptr not starting at 0": put("pt_ptr", 0, 1), "pt_ptr descending": put("pt_ptr", 2, 3), "pt_ptr negative": put("pt_ptr", 0, -2),
        "points above the bound": put("pt_ptr", slice(1, None), (1 << 22) + 1),
        "win even": put("win", 0, 6), "win 1": put("win", 1, 1), "win 33": put("win", 3, 33), "win -3": put("win", 2, -3),
        "rows == win": put("rows", 3, 31), "cols == win": put("cols", 0, 5), "rows below win": put("rows", 1, 6), "cols 0": put("cols", 2, 0),
        "stride below cols": put("stride", 1, 51),
        "more than 2^26 pixels": lambda d, keep, r: (keep["rows"].__setitem__(slice(None), 4097), keep["cols"].__setitem__(slice(None), 4096),
                                                     keep["stride"].__setitem__(slice(None), 4096)),
        "max_level -1": par("max_level", -1), "max_level 4": par("max_level", 4), "max_iter 0": par("max_iter", 0), "max_iter 31": par("max_iter", 31),
        "eps 0": par("eps", 0.0), "eps negative": par("eps", -0.01), "eps NaN": par("eps", float("nan")), "eps inf": par("eps", float("inf")),
        "eps above 10": par("eps", 10.5),
        "threshold 0": par("min_eig_threshold", 0.0), "threshold NaN": par("min_eig_threshold", float("nan")), "threshold inf": par("min_eig_threshold", float("inf")),
        "pt NaN": put("pt", (0, 1), np.nan), "pt inf": put("pt", (2, 0), np.inf), "pt above 2^20": put("pt", (2, 0), 1048577.0),
        "pt below -2^20": put("pt", (11, 1), -1048577.0),
        "NULL prev image of a frame with points": lambda d, keep, r: keep["prev_image"].__setitem__(0, None),
        "NULL next image of a frame with points": lambda d, keep, r: keep["next_image"].__setitem__(3, None),
    }
    for field in ("prev_image", "next_image", "rows", "cols", "stride", "win", "pt_ptr", "pt"):
        refusals["NULL " + field] = null(field)
    for field, _, _, _ in built_lib.LK_ARRAYS:
        refusals["NULL result " + field] = null(field, res=True)
    for label, mutate in refusals.items():
        rc, status, clean = call(mutate)
        assert rc == built_lib.ERR_ARG and status == built_lib.ERR_ARG and clean, label
    # NULL handle, descriptor, result: not even the status
    rc, status, clean = call(handle=None)
    assert rc == built_lib.ERR_ARG and status == 99 and clean
    rc, status, clean = call(desc=False)
    assert rc == built_lib.ERR_ARG and status == 99 and clean
    assert call(result=False)[0] == built_lib.ERR_ARG
    # no frames: MOVBA_OK, the status and nothing else - whatever else the descriptor holds
    rc, status, clean = call(lambda d, keep, r: (setattr(d, "n_frames", 0), setattr(d, "pt_ptr", None), setattr(r, "kept_ptr", None)))
    assert rc == 0 and status == 0 and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lk_main():
    subprocess.check_call(["make", "-C", LK_DIR, "-s", "lk_main_asan"])
    return os.path.join(LK_DIR, "lk_main_asan")


def run_lk_main(exe, frames, tmp_path, **params):
    """tests/lk/lk_main.cpp on one call -> the fields of Solver.lk_track's dict"""
    from movba import capi
    p = dict(K.PARAMS, **params)
    d, keep = capi.lk_desc(frames, **p)
    nf, n = len(frames), len(keep["pt"])
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([nf, n, p["max_level"], p["max_iter"]], np.int32).tobytes())
        f.write(np.array([p["eps"], p["min_eig_threshold"]], np.float64).tobytes())
        for key in ("rows", "cols", "win", "pt_ptr", "pt"):
            f.write(keep[key].tobytes())
        for fr in frames:
            if len(np.asarray(fr["pt"]).reshape(-1, 2)):
                f.write(np.ascontiguousarray(fr["prev"]).tobytes())
                f.write(np.ascontiguousarray(fr["next"]).tobytes())
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lk_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    at = 0

    def take(count, dtype, width=1):
        nonlocal at
        a = np.frombuffer(blob, dtype, count * width, at)
        at += a.nbytes
        return a.reshape(count, width) if width > 1 else a

    out = dict(next_pt=take(n, np.float32, 2), pt_status=take(n, np.uint8), err=take(n, np.float32), exit_code=take(n, np.uint8), keep=take(n, np.uint8),
               kept_ptr=take(nf + 1, np.int32), kept_src=take(n, np.int32))
    assert at == len(blob)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_the_librarys_steps_on_every_case(lk_main, tmp_path, case):
    frames, ref = CASES[case][0](), CASES[case][1]()
    K.compare(run_lk_main(lk_main, frames, tmp_path), ref, case)
    # frames alone: their pixels are the whole buffer, so a read behind them is seen
    for f in ALONE.get(case, range(len(frames))):
        K.compare(run_lk_main(lk_main, [frames[f]], tmp_path), K.frame_part(ref, f), f"{case}, frame {f} alone")


def test_the_librarys_steps_under_other_parameters(lk_main, tmp_path):
    for params in (dict(max_level=0), dict(max_level=1, max_iter=2), dict(eps=1e-3, max_iter=30), dict(min_eig_threshold=0.05), dict(max_level=2)):
        K.compare(run_lk_main(lk_main, K.exits_case(), tmp_path, **params), K.ref_lk(K.exits_case(), **params), f"exits, {params}")
    K.compare(run_lk_main(lk_main, [K.sizes_case()[6]], tmp_path, max_level=2), K.ref_lk([K.sizes_case()[6]], max_level=2), "level 3 cut by max_level")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["lk_asan", "lk_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/lk/lk_driver.cpp: every refusal of the header with nothing written, calls without frames, frames without points
    and without images, strided rows, pinned against ordinary result memory, calls of growing and shrinking size, the call
    between upload, run, download and reset of a window on the same handle, and two handles on two threads - with the library's
    host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of tests/lk linked into one program."""
    subprocess.check_call(["make", "-C", LK_DIR, "-s", target])
    r = subprocess.run([os.path.join(LK_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "lk driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
