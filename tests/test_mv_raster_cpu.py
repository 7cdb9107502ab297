"""movba_mv_raster without a GPU: the two restatements the GPU tests compare against (tests/mv_raster_ref.py) held equal on every
case, and the conditions the cases must meet before any device comparison; the symbol, the struct layouts and every refusal of
the header through the built library (the checks run before the handle is touched); the library's own steps on the CPU
(tests/mv_raster/mvr_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement; and the host side of
the call - checks, packing, copy-out, pinned and ordinary results, a handle shared with a window, two handles on two threads -
under the sanitizers (tests/mv_raster: a stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its
own).  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mv_raster_ref as M
from conftest import ROOT

MVR_DIR = os.path.join(ROOT, "tests", "mv_raster")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
CASES = dict(full=(M.full_case, M.full_ref), pile=(M.pile_case, M.pile_ref), counts=(M.counts_case, M.counts_ref), mixed=(M.mixed_case, M.mixed_ref),
             multiples=(M.multiples_case, M.multiples_ref), frames=(M.frames_case, M.frames_ref), chunks=(M.chunks_case, M.chunks_ref))
SMALL = [name for name in CASES if name != "chunks"]       # (what the literal and the set restatement walk in seconds)
ALONE = dict(frames=M.FRAMES_ALONE, chunks=())              # the frames run alone too; every frame where nothing is said


# ---- the restatements and their cases ------------------------------------------------------------------------------------------

def test_the_two_restatements_agree_on_every_case():
    """... and the third, with numpy, equals both"""
    for name in SMALL:
        case, ref = CASES[name]
        M.compare(M.ref_mv_raster(case(), literal=False), ref(), name)
        M.compare(M.ref_mv_raster(case(), vector=True), ref(), name + ", numpy")
        M.compare(M.ref_mv_raster(case(), vector=True), M.ref_mv_raster(case(), literal=False), name + ", numpy against the sets")
    for threshold in (0.5, float(np.nextafter(0.5, 1))):
        M.compare(M.ref_mv_raster(M.gate_case(threshold), literal=False), M.ref_mv_raster(M.gate_case(threshold)), "gate")
        M.compare(M.ref_mv_raster(M.gate_case(threshold), vector=True), M.ref_mv_raster(M.gate_case(threshold)), "gate, numpy")
    M.compare(M.ref_mv_raster(M.edge_case(), literal=False), M.ref_mv_raster(M.edge_case()), "edge")
    M.compare(M.ref_mv_raster(M.edge_case(), vector=True), M.ref_mv_raster(M.edge_case()), "edge, numpy")
    # the frame of 66 600 records: the literal painting of its first chunk and the sets at every 20th query
    M.compare_head(M.chunks_ref())


def test_full_case_meets_the_input_conditions():
    frames, ref = M.full_case(), M.full_ref()
    assert [(fr["rows"], fr["cols"]) for fr in frames] == [(48, 40), (40, 48)]
    assert [len(fr["q_pt"]) for fr in frames] == [1920, 1920] and all(290 <= len(fr["records"]["w"]) <= 310 for fr in frames)
    for f, fr in enumerate(frames):
        H, W = fr["rows"], fr["cols"]
        recs = M.records_of(fr)
        rec_kept = ref["rec_kept"][ref["rec_ptr"][f]:ref["rec_ptr"][f + 1]]
        named = M.named_records(H, W)
        at = {name: recs.index(r) for name, r in named.items()}
        ext = {name: M.extent(r, W, H) for name, r in named.items()}
        # the two ways to straddle a tile border
        assert ext["extent from tile offset 15"][0] % 16 == 15 and ext["extent from tile offset 15"][2] // 16 == ext["extent from tile offset 15"][0] // 16 + 1
        assert ext["extent from tile offset 0"][0] % 16 == 0 and ext["extent from tile offset 0"][2] // 16 == ext["extent from tile offset 0"][0] // 16 + 1
        assert ext["extent from tile offset 0"][1] % 16 == 0 and ext["extent from tile offset 15 in y"][1] % 16 == 15
        # empty extents, each kept with an index of its own
        for name in ("source left of the frame", "source right of the frame", "source above the frame", "source below the frame"):
            x0, y0, x1, y1 = ext[name]
            assert (x0 > x1 or y0 > y1) and rec_kept[at[name]] >= 0, name
            assert not (ref["cand"][ref["q_ptr"][f]:ref["q_ptr"][f + 1]] == rec_kept[at[name]]).any(), name
        assert named["source left of the frame"][0] == -20 and named["source right of the frame"][0] == W + 20
        # clips
        assert ext["source clipped at 0"][:2] == (0, 0) and named["source clipped at 0"][0] - 8 < 0
        assert ext["source clipped at W - 1"][2] == W - 1 and named["source clipped at W - 1"][0] + 8 > W - 1
        assert ext["source clipped at H - 1"][3] == H - 1 and named["source clipped at H - 1"][1] + 8 > H - 1
        # the keep test on its boundary
        for axis, size, skipped, kept in ((2, W, "dst_x + hx == W", "dst_x + hx == W - 1"), (3, H, "dst_y + hy == H", "dst_y + hy == H - 1")):
            assert named[skipped][axis] + named[skipped][4 if axis == 2 else 5] // 2 == size and rec_kept[at[skipped]] == -1
            assert named[kept][axis] + named[kept][4 if axis == 2 else 5] // 2 == size - 1 and rec_kept[at[kept]] >= 0
        # the destination's clamp keeps the size
        k0 = ref["kept_ptr"][f]
        top = ref["kp_rect"][k0 + rec_kept[at["destination whose top clamps to 0"]]]
        assert top.tolist() == [12, 0, 16, 16] and named["destination whose top clamps to 0"][3] - 8 < 0
        assert ref["kp_rect"][k0 + rec_kept[at["destination whose left clamps to 0"]]].tolist()[0] == 0
        assert {(r[4], r[5]) for r, m in zip(recs, rec_kept) if m >= 0} == {(w, h) for w in M.SIZES for h in M.SIZES}
        # the random ones reach every clamp too, and pixels with 0, 1, 2, 3 and more records exist
        cand = ref["cand"][ref["q_ptr"][f]:ref["q_ptr"][f + 1]]
        for k in range(4):
            assert ((cand >= 0).sum(axis=1) == k).any(), k
        assert ((cand[:, 3] >= 0) & (cand[:, 3] > cand[:, 2] + 1)).any()
        assert ref["grid_covered"][ref["grid_ptr"][f]:ref["grid_ptr"][f + 1]].any()


def test_pile_counts_and_mixed_cases_are_what_the_gpu_tests_ask_for():
    frames, ref = M.pile_case(), M.pile_ref()
    x, y = M.PILE_PIXEL
    for f, k in enumerate(M.PILE):
        W = frames[f]["cols"]
        got = ref["cand"][ref["q_ptr"][f] + y * W + x].tolist()
        rec_kept, kept = M.kept_records(frames[f])
        covering = [m for m, r in enumerate(kept) if r[0] != -20]
        assert len(covering) == k and got == covering[:3] + [covering[-1] if k >= 4 else -1]
        assert covering != list(range(k)) and -1 in rec_kept
    assert M.PILE == (3, 4, 5, 70)
    frames, ref = M.counts_case(), M.counts_ref()
    assert tuple(len(fr["records"]["w"]) for fr in frames) == M.COUNTS == (1, 63, 64, 65, 257, 2500)
    assert {len(fr["q_pt"]) for fr in frames} == {0, 1, 65}
    big = ref["rec_kept"][ref["rec_ptr"][5]:]
    assert (big[2::3] == -1).all() and (big[0::3] >= 0).all() and (big[1::3] >= 0).all() and big.max() > 1024
    assert set(ref["force_grid"].tolist()) == {0, 1}
    frames, ref = M.mixed_case(), M.mixed_ref()
    assert len({(fr["rows"], fr["cols"]) for fr in frames}) == 5
    # the I-frame
    assert len(frames[1]["records"]["w"]) == 0 and ref["kept_ptr"][1] == ref["kept_ptr"][2] and ref["cover_px"][1] == 0 and ref["coverage_area"][1] == 0.0
    assert ref["force_grid"][1] == 1 and frames[1]["coverage_threshold"] > 0
    assert (ref["cand"][ref["q_ptr"][1]:ref["q_ptr"][2]] == -1).all() and not ref["grid_covered"][ref["grid_ptr"][1]:ref["grid_ptr"][2]].any()
    assert ref["grid_ptr"][2] > ref["grid_ptr"][1]
    # no queries and no lattice
    assert ref["q_ptr"][2] == ref["q_ptr"][3] and ref["grid_ptr"][2] == ref["grid_ptr"][3] and ref["kept_ptr"][3] > ref["kept_ptr"][2]
    # the lattice, covered and not
    g = ref["grid_covered"][ref["grid_ptr"][3]:ref["grid_ptr"][4]]
    assert len(g) == 15 and 0 < g.sum()
    assert ref["kept_ptr"][-1] < len(ref["mv_dindx"]) and (ref["mv_dindx"][ref["kept_ptr"][-1]:] == -1).all() and np.isnan(ref["mv_pt"][ref["kept_ptr"][-1]:]).all()
    ref = M.ref_mv_raster(M.gate_case(0.5))
    assert ref["cover_px"].tolist() == [2048] and ref["coverage_area"].tolist() == [0.5] and ref["force_grid"].tolist() == [0]
    assert M.ref_mv_raster(M.gate_case(float(np.nextafter(0.5, 1))))["force_grid"].tolist() == [1]


def _tiles(fr):
    return ((fr["rows"] + 15) // 16) * ((fr["cols"] + 15) // 16)


def test_chunks_multiples_and_frames_cases_are_what_the_gpu_tests_ask_for():
    """the inputs that take the scans only the device runs - the carry over a frame's chunks, the sums over frames and over tiles -
    past their first wavefront, onto their edges and over runs of empty frames"""
    # many chunks
    (fr,), ref = M.chunks_case(), M.chunks_ref()
    n = len(fr["records"]["w"])
    assert (fr["rows"], fr["cols"]) == (528, 544) and _tiles(fr) == 33 * 34 == 1122
    per = (1122 + 1023) // 1024
    assert per == 2 and 561 * per >= 1122 > 560 * per                    # two tiles per thread, none from thread 561 on
    assert n == 66600 and (n + 1023) // 1024 == 66 and n - 65 * 1024 == 40 and fr["want_grid"] == 1
    rec_kept = ref["rec_kept"]
    for a, b in ((0, 64 * 1024), (64 * 1024, 65 * 1024), (65 * 1024, n)):           # chunks 0 - 63, chunk 64, chunk 65
        assert (rec_kept[a:b] >= 0).any() and (rec_kept[a:b] == -1).any(), (a, b)
    per_chunk = [int((rec_kept[c * 1024:(c + 1) * 1024] >= 0).sum()) for c in range(66)]
    assert all(0 < k < 1024 for k in per_chunk[:65]) and 0 < per_chunk[65] < 40
    # (the carry of chunk 65 is a sum over lanes of wave 0 and one lane of wave 1; dropping wave 0's part moves every index)
    assert rec_kept[65 * 1024:][rec_kept[65 * 1024:] >= 0][0] == sum(per_chunk[:65]) > 64 * 900
    assert 1900 <= len(fr["q_pt"]) <= 2100
    cand = ref["cand"]
    assert (cand[:, 3] >= 0).sum() > 100 and (cand[:, 3] >= sum(per_chunk[:64])).any()    # the "largest" slot, from records of chunks 64 and 65 too
    px = np.array(M.query_pixels(fr))
    inside = (px[:, 0] >= 0) & (px[:, 1] >= 0) & (px[:, 0] < 544) & (px[:, 1] < 528)
    assert ((cand == -1).all(axis=1) & inside).sum() > 20 and (~inside).any() and (cand[~inside] == -1).all()
    assert (px[(cand == -1).all(axis=1) & inside][:, 1] >= M.CHUNKS_BAND).any()
    assert set(ref["grid_covered"].tolist()) == {0, 1} and len(ref["grid_covered"]) == 32 * 33
    assert ref["cover_px"][0] < 1 << 28
    # exact multiples
    frames, ref = M.multiples_case(), M.multiples_ref()
    assert tuple(len(f["records"]["w"]) for f in frames) == M.MULTIPLES == (1024, 2048, 1025)
    assert all((f["rows"], f["cols"]) == (64, 96) for f in frames)
    for f in range(3):
        a, b = int(ref["rec_ptr"][f]), int(ref["rec_ptr"][f + 1])
        for c in range(a, b, 1024):
            assert (ref["rec_kept"][c:min(c + 1024, b)] == -1).any(), (f, c)          # a skipped record in every chunk
    assert ref["rec_kept"][1023] == ref["kept_ptr"][1] - 1 >= 0                       # the last record of a full last chunk is kept
    assert ref["rec_kept"][1024 + 2047] == ref["kept_ptr"][2] - ref["kept_ptr"][1] - 1 >= 0
    assert ref["rec_kept"][-1] == -1
    # many frames
    frames, ref = M.frames_case(), M.frames_ref()
    assert len(frames) == M.N_FRAMES == 1024
    assert all(16 <= f["rows"] <= 40 and 16 <= f["cols"] <= 40 for f in frames) and {f["rows"] for f in frames} == set(range(16, 41))
    n_rec, n_q = np.diff(ref["rec_ptr"]), np.diff(ref["q_ptr"])
    assert n_rec.min() == 0 and n_rec.max() == 5 and n_q.min() == 0 and n_q.max() == 3
    for counts, none in ((n_rec, M.FRAMES_NO_RECORDS), (n_q, M.FRAMES_NO_QUERIES)):
        assert (counts[list(none)] == 0).all() and none[0] == 0 and none[-1] == 1023
        zero = "".join("0" if c == 0 else "x" for c in counts[1:-1])
        assert "x000" in zero and "000x" in zero                                     # a run of at least 3 in the middle
    assert sum(_tiles(f) for f in frames) > 1024
    kept = np.diff(ref["kept_ptr"])
    assert all((kept[64 * w:64 * (w + 1)] > 0).any() for w in range(16))             # every wavefront of the frame scan holds a count
    assert (kept < n_rec).any() and ((kept == 0) & (n_rec > 0)).any()
    assert M.FRAMES_ALONE == (0, 63, 64, 65, 511, 1023) and all(n_rec[f] > 0 and n_q[f] > 0 for f in (63, 64, 65, 511))
    assert (np.diff(ref["grid_ptr"]) == 0).any() and (np.diff(ref["grid_ptr"]) > 0).any() and ref["grid_covered"].any()
    assert (ref["cand"] >= 0).any() and set(ref["force_grid"].tolist()) == {0, 1}


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_mv_raster")
    assert "movba_mv_raster" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_mv_raster_desc", built_lib.MvRasterDesc), ("movba_mv_raster_result", built_lib.MvRasterResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d %d\\n", MOVBA_MAX_EXPRESS_IMAGES, MOVBA_MAX_EXPRESS_ITEMS, MOVBA_VERSION);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.MvRasterDesc, built_lib.MvRasterResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.MvRasterDesc) == 128 and C.sizeof(built_lib.MvRasterResult) == 96
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    assert "} movba_mv_raster_desc;   /* 128 bytes */" in hdr and "} movba_mv_raster_result; /* 96 bytes */" in hdr
    assert rows[2] == [built_lib.MAX_EXPRESS_IMAGES, built_lib.MAX_EXPRESS_ITEMS, 5]


def _small_case():
    rng = np.random.default_rng(4)

    def q(rows, cols, n):
        return np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)], axis=1)

    return [M.frame(30, 34, M.random_records(rng, 30, 34, 6), q(30, 34, 5), want_grid=1), M.frame(20, 52, M.random_records(rng, 20, 52, 5), q(20, 52, 4)),
            M.frame(25, 25, [], q(25, 25, 2), want_grid=1), M.frame(40, 40, M.random_records(rng, 40, 40, 4), q(40, 40, 3))]


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L_ = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)

    def call(mutate=None, handle=h, desc=True, result=True, frames=None):
        d, keep = built_lib.mv_raster_desc(_small_case() if frames is None else frames)
        r, out = built_lib.mv_raster_result(d.n_frames, len(keep["src_x"]), len(keep["q_pt"]), keep["n_grid"],
                                            alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
        r.status = 99
        if mutate:
            mutate(d, keep, r)
        rc = L_.movba_mv_raster(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    refusals = {
        "negative n_frames": lambda d, keep, r: setattr(d, "n_frames", -1), "n_frames above the bound": lambda d, keep, r: setattr(d, "n_frames", 1025),
        "rec_ptr not starting at 0": put("rec_ptr", 0, 1), "rec_ptr descending": put("rec_ptr", 2, 3), "q_ptr negative": put("q_ptr", 0, -2),
        "q_ptr descending": put("q_ptr", 1, 100),
        "more than 2^20 records in a frame": put("rec_ptr", slice(1, None), (1 << 20) + 1),
        "records above the bound": put("rec_ptr", slice(1, None), (1 << 22) + 1),
        "records, queries and lattice rects above the bound": put("q_ptr", slice(1, None), (1 << 22) - 12),
        "rows 0": put("rows", 0, 0), "cols 0": put("cols", 3, 0), "rows 32768": put("rows", 1, 32768), "cols -5": put("cols", 2, -5),
        "more than 2^28 pixels": lambda d, keep, r: (keep["rows"].__setitem__(slice(None), 16384), keep["cols"].__setitem__(slice(None), 16384)),
        "w 12": put("w", 0, 12), "w 0": put("w", 3, 0), "w 32": put("w", 14, 32), "h 2": put("h", 1, 2), "h 255": put("h", 7, 255),
        "ref 1": put("ref", 2, 1), "ref -1": put("ref", 0, -1), "source 0": put("source", 5, 0), "source 1": put("source", 14, 1),
        "q_pt NaN": put("q_pt", (0, 1), np.nan), "q_pt inf": put("q_pt", (2, 0), np.inf), "q_pt above 2^20": put("q_pt", (2, 0), 1048577.0),
        "q_pt below -2^20": put("q_pt", (13, 1), -1048577.0),
        "coverage_threshold NaN": put("coverage_threshold", 0, np.nan), "coverage_threshold inf": put("coverage_threshold", 3, -np.inf),
    }
    for field in ("rows", "cols", "coverage_threshold", "want_grid", "rec_ptr", "src_x", "src_y", "dst_x", "dst_y", "w", "h", "source", "ref", "q_ptr", "q_pt"):
        refusals["NULL " + field] = null(field)
    for field, _, _, _ in built_lib.MV_RASTER_ARRAYS:
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
    rc, status, clean = call(lambda d, keep, r: (setattr(d, "n_frames", 0), setattr(d, "rec_ptr", None), setattr(r, "kept_ptr", None)))
    assert rc == 0 and status == 0 and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mvr_main():
    subprocess.check_call(["make", "-C", MVR_DIR, "-s", "mvr_main_asan"])
    return os.path.join(MVR_DIR, "mvr_main_asan")


def run_mvr_main(exe, frames, tmp_path):
    """tests/mv_raster/mvr_main.cpp on one call -> the fields of Solver.mv_raster's dict"""
    from movba import capi
    d, keep = capi.mv_raster_desc(frames)
    nf, nr, nq, ng = len(frames), len(keep["src_x"]), len(keep["q_pt"]), keep["n_grid"]
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([nf, nr, nq], np.int32).tobytes())
        for key in ("rows", "cols", "coverage_threshold", "want_grid", "rec_ptr", "q_ptr", "src_x", "src_y", "dst_x", "dst_y", "w", "h", "q_pt"):
            f.write(keep[key].tobytes())
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mvr_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    at = 0

    def take(count, dtype, width=1):
        nonlocal at
        a = np.frombuffer(blob, dtype, count * width, at)
        at += a.nbytes
        return a.reshape(count, width) if width > 1 else a

    out = dict(kept_ptr=take(nf + 1, np.int32), kp_rect=take(nr, np.int32, 4), mv_pt=take(nr, np.float32, 2), mv_dindx=take(nr, np.int32),
               rec_kept=take(nr, np.int32), cand=take(nq, np.int32, 4), grid_ptr=take(nf + 1, np.int32), grid_covered=take(ng, np.uint8),
               cover_px=take(nf, np.int32), coverage_area=take(nf, np.float64), force_grid=take(nf, np.uint8))
    assert at == len(blob)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_the_librarys_steps_on_every_case(mvr_main, tmp_path, case):
    frames, ref = CASES[case][0](), CASES[case][1]()
    M.compare(run_mvr_main(mvr_main, frames, tmp_path), ref, case)
    # every frame alone: its arrays are the whole buffers, so a read behind them is seen
    for f in ALONE.get(case, range(len(frames))):
        M.compare(run_mvr_main(mvr_main, [frames[f]], tmp_path), M.ref_mv_raster([frames[f]]), f"{case}, frame {f} alone")


def test_the_librarys_steps_on_the_gate_and_the_edge(mvr_main, tmp_path):
    for threshold in (0.5, float(np.nextafter(0.5, 1))):
        M.compare(run_mvr_main(mvr_main, M.gate_case(threshold), tmp_path), M.ref_mv_raster(M.gate_case(threshold)), "gate")
    M.compare(run_mvr_main(mvr_main, M.edge_case(), tmp_path), M.ref_mv_raster(M.edge_case()), "edge")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["mv_raster_asan", "mv_raster_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/mv_raster/mv_raster_driver.cpp: every refusal of the header with nothing written, calls without frames, frames
    without records and without queries, pinned against ordinary result memory, calls of growing and shrinking size, the call
    between upload, run, download and reset of a window on the same handle, and two handles on two threads - with the library's
    host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of tests/mv_raster linked into one program."""
    subprocess.check_call(["make", "-C", MVR_DIR, "-s", target])
    r = subprocess.run([os.path.join(MVR_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "mv_raster driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
