"""movba_advance without a GPU: the two restatements the GPU tests compare against (tests/advance_ref.py) held equal on every case,
and the conditions the cases must meet before any device comparison; the symbol, the struct layouts and every refusal of the
header through the built library (the checks run before the handle is touched); the library's own steps on the CPU
(tests/advance/adv_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement; and the host side of
the call - checks, packing, copy-out, pinned and ordinary results, a handle shared with a window, two handles on two threads -
under the sanitizers (tests/advance: a stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its
own).  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import advance_ref as A
import express_ref as R
from conftest import ROOT

ADV_DIR = os.path.join(ROOT, "tests", "advance")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")


# ---- the restatements and their cases ------------------------------------------------------------------------------------------

def test_the_two_restatements_agree_on_every_case():
    A.compare(A.ref_advance(A.mixed_case()[0], literal=False), A.mixed_ref(), "mixed")
    A.compare(A.ref_advance(A.counts_case(), literal=False), A.counts_ref(), "counts")
    A.compare(A.ref_advance(A.trio_case(), literal=False), A.trio_ref(), "trio")
    # the bound: the literal walk over the first 500 positions (what lies behind them cannot change them)
    A.compare_head(A.bound_ref())
    A.compare(A.ref_advance(A.frames_case(), literal=False), A.frames_ref(), "frames")
    A.compare(A.ref_advance(A.lattice_case(), literal=False), A.lattice_ref(), "lattice")
    # the bound's frame behind three others: the same walk over its rows, and the three literally
    A.compare_head(A.frame_part(A.behind_ref(), 3))
    lit = A.ref_advance(A.behind_case()[:3])
    for f in range(3):
        assert A.frame_rows(lit, f) == A.frame_rows(A.behind_ref(), f), f


def test_mixed_case_meets_the_input_conditions():
    frames, notes = A.mixed_case()
    ref = A.mixed_ref()
    # frames: at most 64 x 96, one with padded, poisoned rows, one without previous features
    assert all(fr["image"].shape[0] <= 64 and fr["image"].shape[1] <= 96 for fr in frames)
    assert frames[1]["image"].strides[0] > frames[1]["image"].shape[1] and (frames[1]["image"].base[:, 56:] == 0xA5).all()
    assert len(frames[2]["prev_age"]) == 0 and len(frames[2]["kp_rect"]) > 0
    fr = frames[0]
    n = len(fr["prev_age"])
    fate, order, chosen, distance = (ref[k][:n] for k in ("fate", "order", "chosen_mv", "distance"))
    position = np.empty(n, np.int64)
    position[order] = np.arange(n)
    age = fr["prev_age"]
    count = np.array([A.popcount(R.as_int(w)) for w in fr["prev_desc"]])
    # sort
    groups = {}
    for i in range(n):
        groups.setdefault((int(age[i]), int(count[i])), []).append(i)
    ties = [g for g in groups.values() if len(g) > 1]
    assert len(ties) >= 3
    for g in ties:                                              # the tie rule: ascending input index, at adjacent positions
        assert position[g].tolist() == list(range(int(position[g[0]]), int(position[g[0]]) + len(g)))
    assert sum(1 for a in set(age.tolist()) if len({int(c) for c in count[age == a]}) > 1) >= 2
    assert order.tolist() != list(range(n))
    key = [(-int(age[i]), -int(count[i]), int(i)) for i in order]
    assert key == sorted(key)
    # candidates
    cand = fr["prev_cand"]
    n_cand = np.array([4 if -1 not in c.tolist() else c.tolist().index(-1) for c in cand])
    plain = fr["prev_coverage"] == 0
    for k in (1, 2, 3, 4):
        assert int(((n_cand == k) & plain).sum()) >= 3, k

    def dists(idx):
        """the distance of every candidate of a feature, None where its rect is out of bounds"""
        out = []
        for c in cand[idx][:n_cand[idx]]:
            mb = A.rect_of(fr["prev_pt"][idx], fr["mv_pt"][c], *fr["prev_mb"][idx])[1]
            out.append(None if R.rejected(mb, 64, 96) else A.popcount(R.as_int(fr["prev_desc"][idx]) ^ A.true_desc(fr["image"], mb, 25)))
        return out

    multi = [i for i in range(n) if plain[i] and n_cand[i] >= 2]
    assert sum(1 for i in multi if chosen[i] != cand[i][0]) >= 3
    equal_best = 0
    for i in multi:
        d = [v for v in dists(i) if v is not None]
        if d and d.count(min(d)) >= 2:
            equal_best += 1
            assert chosen[i] == cand[i][[v == min(d) for v in dists(i)].index(True)]            # the earlier one
    assert equal_best >= 2
    assert sum(1 for i in multi if all(v is None for v in dists(i)) and fate[i] == A.ADV_REJ_BOUNDS and chosen[i] == cand[i][0]) >= 2
    assert sum(1 for i in range(n) if plain[i] and n_cand[i] == 1 and dists(i) == [None] and fate[i] == A.ADV_REJ_BOUNDS) >= 1
    # truncation
    seg = ref["seg_ptr"]
    kept_rect = {int(order[src]): ref["feat_rect"][o] for o, src in zip(range(seg[0], seg[1]), ref["feat_src"][seg[0]:seg[1]])}
    in_gap = below = 0
    odd = even = False
    for i in range(n):
        if fate[i] in (A.ADV_COVERAGE, A.ADV_NO_MV):
            continue
        w, h = fr["prev_mb"][i]
        q = fr["prev_pt"][i] + fr["mv_pt"][chosen[i]]
        fx, fy = np.float32(q[0] - np.float32(w // 2)), np.float32(q[1] - np.float32(h // 2))
        if (-1 < fx < 0 or -1 < fy < 0) and fate[i] == A.ADV_KEPT:
            in_gap += 1
            assert (kept_rect[i][0] == 0) if -1 < fx < 0 else (kept_rect[i][1] == 0)
        below += (fx <= -1 or fy <= -1) and fate[i] == A.ADV_REJ_BOUNDS
        if fx > 0 and fx != np.floor(fx):
            odd |= int(fx) % 2 == 1
            even |= int(fx) % 2 == 0
    assert in_gap >= 2 and below >= 1 and odd and even
    # claims
    dst = np.where(chosen >= 0, fr["mv_dindx"][np.maximum(chosen, 0)], -1)
    arrives = np.isin(fate, (A.ADV_KEPT, A.ADV_FAR, A.ADV_LOST_CLAIM))
    contested = later_winner = far_winner = after_reject = 0
    for m in range(len(fr["kp_rect"])):
        reach = [i for i in range(n) if arrives[i] and dst[i] == m]
        assert bool(ref["kp_found"][m]) == bool(reach)
        if not reach:
            continue
        winner = min(reach, key=lambda i: position[i])
        assert fate[winner] != A.ADV_LOST_CLAIM and all(fate[i] == A.ADV_LOST_CLAIM for i in reach if i != winner)
        contested += len(reach) >= 2
        later_winner += any(i < winner for i in reach if i != winner)
        far_winner += len(reach) >= 2 and fate[winner] == A.ADV_FAR
        after_reject += any(fate[i] == A.ADV_REJ_BOUNDS and dst[i] == m and position[i] < position[winner] for i in range(n))
    assert contested >= 3 and later_winner >= 1 and far_winner >= 1 and after_reject >= 1
    shared = {}
    for i in range(n):
        if arrives[i] and dst[i] == -1:
            shared.setdefault(int(chosen[i]), []).append(i)
    assert any(len(v) >= 3 and all(fate[i] != A.ADV_LOST_CLAIM for i in v) for v in shared.values())
    # the gate, the fates
    assert ((distance == 40) & (fate == A.ADV_KEPT)).any() and ((distance == 41) & (fate == A.ADV_FAR)).any()
    assert not ((distance > 40) & (fate == A.ADV_KEPT)).any() and not ((distance <= 40) & (distance >= 0) & (fate == A.ADV_FAR)).any()
    assert set(fate.tolist()) == set(A.FATES)
    cov_pos = np.sort(position[fate == A.ADV_COVERAGE])
    assert len(cov_pos) >= 2 and (np.diff(cov_pos) > 1).any()
    # macroblocks
    nk = len(fr["kp_rect"])
    code, found = ref["kp_code"][:nk], ref["kp_found"][:nk]
    assert {tuple(r[2:]) for r, c in zip(fr["kp_rect"].tolist(), code) if c == R.EX_FEATURE} == set(R.SHAPES)
    for c in (R.EX_REJ_BOUNDS, R.EX_REJ_SHAPE, R.EX_REJ_FLAT, R.EX_REJ_NO_EDGE):
        assert (code == c).sum() >= 1, c
    assert fr["kp_rect"][code == R.EX_REJ_SHAPE].tolist() == [[4, 4, 4, 4]]
    assert (code == R.EX_FEATURE).sum() >= 5 and ref["mov_cnt"][0] == (code == R.EX_FEATURE).sum()
    assert (code[found != 0] == 0).all()
    assert sum(1 for m in np.flatnonzero(found) if R.fast_item(fr["image"], tuple(fr["kp_rect"][m].tolist()), R.EX_DETECT, 25)[0] == R.EX_FEATURE) >= 2
    # ids: first_id 0 in one frame and 2^30 in another; new ids precede grid ids and are consecutive; next_id matches
    assert frames[0]["first_id"] == 0 and frames[3]["first_id"] == 2 ** 30
    for f, fr in enumerate(frames):
        s = ref["seg_ptr"][4 * f:4 * f + 4]
        ids = ref["feat_track"][s[1]:s[3]]
        assert ids.tolist() == list(range(fr["first_id"] + 1, fr["first_id"] + 1 + len(ids))) and ref["next_id"][f] == fr["first_id"] + len(ids)
        assert (ref["feat_age"][s[1]:s[3]] == 0).all() and s[2] - s[1] == ref["mov_cnt"][f]
    assert ref["seg_ptr"][3] - ref["seg_ptr"][2] >= 1 and ref["seg_ptr"][-1] < len(ref["feat_src"])        # a grid segment, and padding
    assert (ref["feat_src"][ref["seg_ptr"][-1]:] == -1).all() and np.isnan(ref["feat_pt"][ref["seg_ptr"][-1]:]).all()


def test_trio_case_stands_on_the_mov_cnt_boundary():
    frames, ref = A.trio_case(), A.trio_ref()
    assert all(fr["image"] is frames[0]["image"] for fr in frames) and frames[0]["image"].shape == (64, 96)
    assert ref["mov_cnt"].tolist() == [59, 60, 60] and [fr["force_grid"] for fr in frames] == [0, 0, 1]
    assert ref["grid_ran"].tolist() == [1, 0, 1]
    assert (ref["kp_code"] == R.EX_FEATURE).all() and not ref["kp_found"].any()
    lat = A.lattice(64, 96)
    would = np.array([R.fast_item(frames[0]["image"], mb, R.EX_DETECT, 25)[0] == R.EX_FEATURE for mb in lat])
    for f in range(3):
        s = ref["seg_ptr"][4 * f:4 * f + 4]
        n_grid = s[3] - s[2]
        assert n_grid == (0 if f == 1 else int((would & (frames[f]["grid_covered"] == 0)).sum()))
        if f != 1:
            assert n_grid >= 5 and int((would & (frames[f]["grid_covered"] != 0)).sum()) >= 2
        assert ref["next_id"][f] == frames[f]["first_id"] + ref["mov_cnt"][f] + n_grid
    assert frames[0]["first_id"] == 0 and frames[2]["first_id"] == 2 ** 30


def test_counts_case_is_what_the_gpu_test_asks_for():
    frames, ref = A.counts_case(), A.counts_ref()
    assert tuple(len(fr["prev_age"]) for fr in frames) == A.COUNTS == (0, 1, 63, 64, 65, 257, 1000)
    assert all(fr["image"].shape == (64, 96) and len(set(fr["prev_age"].tolist())) <= 3 for fr in frames)
    assert set(ref["fate"].tolist()) == set(A.FATES)
    assert len(A.bound_case()[0]["prev_age"]) == 16384 and A.bound_case()[0]["image"].shape == (64, 96)


def _items(fr):
    return len(fr["prev_age"]) + len(fr["kp_rect"]) + len(A.lattice(*A.shape_of(fr)))


def test_frames_behind_and_lattice_cases_are_what_the_gpu_tests_ask_for():
    """the inputs that take the sums and scans only the device runs - k_adv_emit's sum over the frames' counts and its strided
    item loop, k_adv_resolve's scans over macroblocks and lattice - past their first pass"""
    # many frames
    frames, ref = A.frames_case(), A.frames_ref()
    assert len(frames) == A.N_FRAMES == 1024 and 3 * 85 == 255                    # (the counts of frame 85 lie on both sides of the first pass of 256)
    shapes = [fr["image"].shape for fr in frames if fr["image"] is not None]
    assert all(17 <= r <= 33 and 17 <= c <= 47 for r, c in shapes) and len(set(shapes)) > 200
    n_prev, n_kp = np.diff(ref["prev_ptr"]), np.diff(ref["kp_ptr"])
    n_mv = np.array([len(fr["mv_dindx"]) for fr in frames])
    assert (n_prev.min(), n_prev.max(), n_kp.min(), n_kp.max(), n_mv.min(), n_mv.max()) == (0, 4, 0, 3, 0, 3)
    for f in A.FRAMES_EMPTY:
        assert frames[f]["image"] is None and _items(frames[f]) == 0, f
    assert A.FRAMES_EMPTY[0] == 0 and A.FRAMES_EMPTY[-1] == 1023 and any(0 < f < 1023 for f in A.FRAMES_EMPTY)
    seg = ref["seg_ptr"][:-1].reshape(1024, 4)
    for part, name in enumerate(("kept", "new", "grid")):
        count = seg[:, part + 1] - seg[:, part]
        assert count[:86].sum() > 0 and count[86:].sum() > 0, name                       # on both sides of frame 86
        assert all(count[256 * k:256 * (k + 1)].sum() > 0 for k in range(4)), name
    assert A.FRAMES_ALONE == (0, 85, 86, 255, 256, 1023) and all(_items(frames[f]) >= 3 for f in (85, 86, 255, 256))
    assert ref["seg_ptr"][-1] < len(ref["feat_src"]) and np.array_equal(ref["seg_ptr"][4::4], seg[1:, 0].tolist() + [ref["seg_ptr"][-1]])
    # the bound's frame behind three others
    frames, ref = A.behind_case(), A.behind_ref()
    assert len(frames) == 4 and frames[3] is A.bound_case()[0] and all(0 < _items(fr) < 30 for fr in frames[:3])
    n_items = sum(_items(fr) for fr in frames)
    chunks = A.emit_chunks(n_items, 4)
    # (not 16: the frame's 16 384 features, 40 macroblocks and 15 lattice rects and the small frames' items over 4 frames make 17
    # by the launch rule - what matters is that they are far fewer than the 64 the frame gets alone, and the four passes)
    assert chunks == 17 < A.emit_chunks(_items(frames[3]), 1) == 64
    assert _items(frames[3]) >= 16384 and -(-_items(frames[3]) // (chunks * 256)) >= 4
    s = ref["seg_ptr"][12:16]
    p0 = int(ref["prev_ptr"][3])
    kept_items = ref["order"][p0 + ref["feat_src"][s[0]:s[1]]]                           # the wave items of the frame's kept features
    assert s[0] > 0 and set((kept_items // (256 * chunks)).tolist()) == {0, 1, 2, 3}     # rows come from every pass of the loop
    assert s[2] > s[1] and s[3] > s[2] and (16384 // (256 * chunks)) == 3                # ... the new and the grid features from the last
    # one 240 x 320 frame, and a second whose lattice is not emitted
    frames, ref = A.lattice_case(), A.lattice_ref()
    assert all(fr["image"].shape == (240, 320) and len(fr["kp_rect"]) == 300 for fr in frames)
    from movba import capi
    grid = capi.express_grid(240, 320)
    assert len(grid) == 266 == len(A.lattice(240, 320)) and grid.tolist() == [list(r) for r in A.lattice(240, 320)]
    assert (300 + 255) // 256 == 2 and (266 + 255) // 256 == 2                           # two entries per thread in both scans
    assert [fr["force_grid"] for fr in frames] == [1, 0] and ref["grid_ran"].tolist() == [1, 0] and ref["mov_cnt"][1] >= 60
    seg = ref["seg_ptr"]
    for f in range(2):
        new = ref["feat_src"][seg[4 * f + 1]:seg[4 * f + 2]]
        assert (new < 256).any() and (new >= 256).any() and new.max() < 300, f          # new macroblocks in both ranges
        code = ref["kp_code"][300 * f:300 * (f + 1)]
        assert ((code[:256] != R.EX_FEATURE).any() and (code[256:] != R.EX_FEATURE).any()) and ref["kp_found"][300 * f:300 * (f + 1)].any()
    g = ref["feat_src"][seg[2]:seg[3]]
    assert (g < 256).any() and (g >= 256).any() and g.max() < 266 and len(g) < 266 - 20     # grid features in both ranges, not all
    covered = frames[0]["grid_covered"]
    assert covered[:256].any() and not covered[g].any()
    assert seg[7] == seg[6] and frames[1]["grid_covered"].sum() < 266                    # nothing of the second frame's lattice
    would = [R.fast_item(frames[1]["image"], mb, R.EX_DETECT, 25)[0] == R.EX_FEATURE for mb in A.lattice(240, 320)]
    assert sum(would) > 100                                                              # ... though it has features enough


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_advance")
    assert "movba_advance" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_advance_desc", built_lib.AdvanceDesc), ("movba_advance_result", built_lib.AdvanceResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d %d %d %d %d %d %d\\n", MOVBA_MAX_ADVANCE_PREV, MOVBA_ADV_KEPT, MOVBA_ADV_COVERAGE, MOVBA_ADV_NO_MV, MOVBA_ADV_REJ_BOUNDS, '
            'MOVBA_ADV_LOST_CLAIM, MOVBA_ADV_FAR, MOVBA_VERSION);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.AdvanceDesc, built_lib.AdvanceResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.AdvanceDesc) == 184 and C.sizeof(built_lib.AdvanceResult) == 136
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    assert "} movba_advance_desc;   /* 184 bytes */" in hdr and "} movba_advance_result; /* 136 bytes */" in hdr
    assert rows[2] == [16384, 1, 2, 16, 17, 18, 19, 5]
    assert rows[2][:7] == [built_lib.MAX_ADVANCE_PREV, built_lib.ADV_KEPT, built_lib.ADV_COVERAGE, built_lib.ADV_NO_MV, built_lib.ADV_REJ_BOUNDS,
                           built_lib.ADV_LOST_CLAIM, built_lib.ADV_FAR]
    assert rows[2][1:7] == [A.ADV_KEPT, A.ADV_COVERAGE, A.ADV_NO_MV, A.ADV_REJ_BOUNDS, A.ADV_LOST_CLAIM, A.ADV_FAR]


def _small_case():
    rng = np.random.default_rng(4)
    frames = [A.random_frame(R.edge_image(rng, 30, 34), rng, 6, n_mv=5, n_kps=4), A.random_frame(R.edge_image(rng, 20, 52), rng, 5, n_mv=4, n_kps=3, first_id=9),
              A.random_frame(R.noise_image(rng, 25, 25), rng, 0, n_mv=0, n_kps=2), A.random_frame(R.edge_image(rng, 40, 40), rng, 4, n_mv=3, n_kps=5)]
    for fr in frames:
        fr["grid_covered"] = np.zeros(len(A.lattice(*fr["image"].shape)), np.uint8)
    return frames


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L_ = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)

    def call(mutate=None, handle=h, desc=True, result=True, frames=None):
        d, keep = built_lib.advance_desc(_small_case() if frames is None else frames)
        r, out = built_lib.advance_result(d.n_frames, len(keep["prev_age"]), len(keep["kp_rect"]), keep["n_grid"],
                                          alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
        r.status = 99
        if mutate:
            mutate(d, keep, r)
        rc = L_.movba_advance(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    refusals = {
        "negative n_frames": lambda d, keep, r: setattr(d, "n_frames", -1), "n_frames above the bound": lambda d, keep, r: setattr(d, "n_frames", 1025),
        "prev_ptr not starting at 0": put("prev_ptr", 0, 1), "prev_ptr descending": put("prev_ptr", 2, 3), "mv_ptr negative": put("mv_ptr", 0, -2),
        "kp_ptr descending": put("kp_ptr", 1, 100), "grid_ptr not starting at 0": put("grid_ptr", 0, 1),
        "a grid_covered range that is not the lattice's": put("grid_ptr", slice(1, None), 1),
        "wave items above the bound": put("kp_ptr", slice(1, None), (1 << 22) + 1),
        "a NULL image that has items": lambda d, keep, r: keep["image"].__setitem__(1, None),
        "rows 0": put("rows", 0, 0), "cols 0": put("cols", 3, 0), "stride below cols": put("stride", 1, 51), "threshold -1": put("threshold", 0, -1),
        "threshold 256": put("threshold", 2, 256),
        "more than 2^28 pixels": lambda d, keep, r: (keep["rows"].__setitem__(slice(None), 16384), keep["cols"].__setitem__(slice(None), 16384),
                                                     keep["stride"].__setitem__(slice(None), 16384)),
        "prev_mb 12": put("prev_mb", (0, 0), 12), "prev_mb 32": put("prev_mb", (7, 1), 32), "prev_mb 0": put("prev_mb", (3, 0), 0),
        "prev_age -1": put("prev_age", 2, -1), "prev_age 2^31 - 1": put("prev_age", 0, 2 ** 31 - 1),
        "prev_cand -2": put("prev_cand", (1, 3), -2), "prev_cand = the frame's n_mv": put("prev_cand", (0, 0), 5),
        "prev_cand of another frame's range": put("prev_cand", (7, 0), 4),
        "mv_dindx -2": put("mv_dindx", 0, -2), "mv_dindx = the frame's n_kps": put("mv_dindx", 1, 4),
        "prev_pt NaN": put("prev_pt", (0, 1), np.nan), "prev_pt inf": put("prev_pt", (2, 0), np.inf), "prev_pt above 2^20": put("prev_pt", (2, 0), 1048577.0),
        "mv_pt NaN": put("mv_pt", (0, 0), np.nan), "mv_pt below -2^20": put("mv_pt", (3, 1), -1048577.0),
        "first_id negative": put("first_id", 0, -1), "first_id + n_kps + n_grid above INT32_MAX": put("first_id", 0, 2 ** 31 - 1 - 4),
    }
    for field in ("image", "rows", "cols", "stride", "threshold", "force_grid", "first_id", "prev_ptr", "prev_pt", "prev_mb", "prev_age", "prev_track",
                  "prev_desc", "prev_coverage", "prev_cand", "mv_ptr", "mv_pt", "mv_dindx", "kp_ptr", "kp_rect", "grid_covered"):
        refusals["NULL " + field] = null(field)
    for field, _, _, _ in built_lib.ADVANCE_ARRAYS:
        refusals["NULL result " + field] = null(field, res=True)
    for label, mutate in refusals.items():
        rc, status, clean = call(mutate)
        assert rc == built_lib.ERR_ARG and status == built_lib.ERR_ARG and clean, label
    # 16385 previous features in one frame (16384 are tests/test_gpu_advance.py's bound case)
    big = A.random_frame(R.edge_image(np.random.default_rng(1), 30, 34), np.random.default_rng(2), 3, n_mv=3, n_kps=2)
    for key in ("prev_pt", "prev_mb", "prev_age", "prev_track", "prev_desc", "prev_coverage", "prev_cand"):
        big[key] = np.ascontiguousarray(np.resize(big[key], (16385,) + big[key].shape[1:]))
    rc, status, clean = call(frames=[big])
    assert rc == built_lib.ERR_ARG and status == built_lib.ERR_ARG and clean
    # NULL handle, descriptor, result: not even the status
    rc, status, clean = call(handle=None)
    assert rc == built_lib.ERR_ARG and status == 99 and clean
    rc, status, clean = call(desc=False)
    assert rc == built_lib.ERR_ARG and status == 99 and clean
    assert call(result=False)[0] == built_lib.ERR_ARG
    # no frames: MOVBA_OK, the status and nothing else - whatever else the descriptor holds
    rc, status, clean = call(lambda d, keep, r: (setattr(d, "n_frames", 0), setattr(d, "prev_ptr", None), setattr(r, "order", None)))
    assert rc == 0 and status == 0 and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def adv_main():
    subprocess.check_call(["make", "-C", ADV_DIR, "-s", "adv_main_asan"])
    return os.path.join(ADV_DIR, "adv_main_asan")


def run_adv_main(exe, frames, tmp_path):
    """tests/advance/adv_main.cpp on one call -> the fields of Solver.advance's dict"""
    from movba import capi
    d, keep = capi.advance_desc(frames)
    nf, n_prev, n_mv, n_kps, n_grid = len(frames), len(keep["prev_age"]), len(keep["mv_dindx"]), len(keep["kp_rect"]), keep["n_grid"]
    lat = [len(A.lattice(*A.shape_of(fr))) for fr in frames]
    covered = keep.get("grid_covered", np.zeros(n_grid, np.uint8))
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([nf, n_prev, n_mv, n_kps, n_grid], np.int32).tobytes())
        for a in (keep["rows"], keep["cols"], keep["threshold"], keep["force_grid"].astype(np.int32), keep["first_id"], keep["prev_ptr"], keep["mv_ptr"],
                  keep["kp_ptr"], np.concatenate([[0], np.cumsum(lat)]).astype(np.int32), keep["prev_pt"], keep["prev_mb"], keep["prev_age"],
                  keep["prev_track"], keep["prev_cand"], keep["prev_desc"], keep["prev_coverage"], keep["mv_pt"], keep["mv_dindx"], keep["kp_rect"], covered):
            f.write(a.tobytes())
        for fr in frames:
            f.write(b"\0" if fr["image"] is None else np.ascontiguousarray(fr["image"]).tobytes())     # (None: 1 x 1 in the descriptor, never read)
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "adv_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    at = 0
    cap = n_prev + n_kps + n_grid

    def take(count, dtype, width=1):
        nonlocal at
        a = np.frombuffer(blob, dtype, count * width, at)
        at += a.nbytes
        return a.reshape(count, width) if width > 1 else a

    out = dict(order=take(n_prev, np.int32), chosen_mv=take(n_prev, np.int32), distance=take(n_prev, np.int32), mov_cnt=take(nf, np.int32),
               next_id=take(nf, np.int32), seg_ptr=take(4 * nf + 1, np.int32), feat_src=take(cap, np.int32), feat_track=take(cap, np.int32),
               feat_rect=take(cap, np.int32, 4), feat_age=take(cap, np.int32), feat_pt=take(cap, np.float32, 2), feat_desc=take(cap, np.uint64, 4),
               fate=take(n_prev, np.uint8), kp_found=take(n_kps, np.uint8), kp_code=take(n_kps, np.uint8), grid_ran=take(nf, np.uint8))
    assert at == len(blob)
    return out


ALONE = dict(counts=(0, 1, 4), frames=A.FRAMES_ALONE, behind=(0, 1, 2))         # the frames run alone too; every frame where nothing is said


@pytest.mark.parametrize("case", ["mixed", "counts", "trio", "frames", "behind", "lattice"])
def test_the_librarys_steps_on_every_case(adv_main, tmp_path, case):
    frames, ref = dict(mixed=(A.mixed_case()[0], A.mixed_ref), counts=(A.counts_case(), A.counts_ref), trio=(A.trio_case(), A.trio_ref),
                       frames=(A.frames_case(), A.frames_ref), behind=(A.behind_case(), A.behind_ref), lattice=(A.lattice_case(), A.lattice_ref))[case]
    A.compare(run_adv_main(adv_main, frames, tmp_path), ref(), case)
    # every frame alone: its image is the whole pixel buffer, so a read behind it is seen
    for f, fr in enumerate(frames):
        if f not in ALONE.get(case, range(len(frames))):
            continue
        A.compare(run_adv_main(adv_main, [fr], tmp_path), A.ref_advance([fr], literal=False), f"{case}, frame {f} alone")


def test_the_librarys_steps_at_the_bound(adv_main, tmp_path):
    A.compare(run_adv_main(adv_main, A.bound_case(), tmp_path), A.bound_ref(), "bound")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["advance_asan", "advance_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/advance/advance_driver.cpp: every refusal of the header with nothing written, calls without frames, padded rows,
    frames without items, grid_ptr left out, pinned against ordinary result memory, calls of growing and shrinking size, the call
    between upload, run, download and reset of a window on the same handle, and two handles on two threads - with the library's
    host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of tests/advance linked into one program."""
    subprocess.check_call(["make", "-C", ADV_DIR, "-s", target])
    r = subprocess.run([os.path.join(ADV_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "advance driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
