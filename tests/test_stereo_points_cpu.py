"""movba_stereo_points without a GPU: the conditions the shared cases (tests/stereo_ref.py) must meet before any device comparison -
every code occurs, every gate's boundary point gets the code its name claims, the median-0 frame really has median 0, the exact
threshold is exact, the walk's lengths are the reference's -; the library's own steps on the CPU (tests/stereo_points/
stereo_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer) against the numpy restatement, exact but for sel_point, which
is held to the derived bound; the symbol, the struct layouts and every refusal of the header through the built library (the
checks run before the handle is touched); and the host side of the call - checks, layout, copy-out, pinned and ordinary results,
optional arrays, a handle shared with a window, two handles on two threads - under the sanitizers (tests/stereo_points: a
stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its own).  No sanitizer touches code loaded
into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_ref as S
from conftest import ROOT

ST_DIR = os.path.join(ROOT, "tests", "stereo_points")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
ALONE = dict(frames=S.FRAMES_ALONE, counts=(1, 2, 4, 5))        # the frames run alone too; every frame where nothing is said
F = np.float32


# ---- the cases are what the GPU tests ask for ------------------------------------------------------------------------------

def test_every_gate_point_gets_the_code_its_name_claims():
    fr = S.gates_case()[0]
    ur, depth, code, pairs = S.gates(fr, 4.0, 0.0)
    for k, (label, _, _, _, want) in enumerate(S.GATE_POINTS):
        assert code[k] == want, label
    by = {p[0]: k for k, p in enumerate(S.GATE_POINTS)}
    dist = dict((i, d) for d, i in pairs)
    # the 0.01 branch: the depth is bf / (float)0.01 and u_right comes from a DOUBLE subtraction, which fp32 would round otherwise
    for label in ("disparity 0: the 0.01 branch", "disparity 0 at a large x"):
        k = by[label]
        assert depth[k] == F(40.0) / F(0.01) and ur[k] == F(np.float64(fr["pt"][k, 0]) - 0.01)
    # (c = 0.01 sits at one place of a binade's grid for every x of the binade, and at none of them do (float)c and c fall on two
    # sides of a rounding boundary: the fp32 subtraction gives the same bits.  The restatement keeps the source's form all the same.)
    assert [dist[by[label]] for label in ("distance 0.99999994", "distance 1.0", "distance just below 2.0", "distance 2.0", "distance 5 from 3 and 4")] == [0, 1, 1, 2, 5]
    assert fr["pt"][by["distance 0.99999994"], 0] == np.nextafter(F(1), F(0)) and np.signbit(fr["next_pt"][by["next.x -0.0 passes"], 0])
    k = by["disparity just below max_disparity"]
    assert fr["pt"][k, 0] - fr["next_pt"][k, 0] == np.nextafter(F(32), F(0)) == np.nextafter(fr["max_disparity"], F(0))
    k = by["row difference just above 4.0"]
    assert fr["next_pt"][k, 1] - fr["pt"][k, 1] == np.nextafter(F(4), F(5))
    ref = S.gates_ref()
    assert set(ref["code"].tolist()) == {S.OK, S.REJ_STATUS, S.REJ_ROW, S.REJ_DISPARITY, S.REJ_FAR}
    assert ref["median_dist"].tolist() == [2, 1] and ref["th_dist"].tolist() == [F(1.5) * F(1.4) * F(2), F(1.5) * F(1.4) * F(1)]
    # the second frame's median holds the threshold at 2.1: distance 2 stays, distance 5 goes
    n = len(S.GATE_POINTS)
    assert ref["code"][n + by["distance 2.0"]] == S.OK and ref["code"][n + by["distance 5 from 3 and 4"]] == S.REJ_FAR
    assert ((ref["depth"] == -1) == (ref["u_right"] == -1)).all() and ((ref["code"] == S.OK) == (ref["depth"] != -1)).all()


def test_the_median_cases_are_what_their_names_claim():
    frames, ref = S.median_case(), S.median_ref()
    m, th = S.exact_threshold()
    assert float(F(1.5) * F(1.4) * F(m)) == th and ref["th_dist"][5] == F(th)
    assert ref["median_dist"].tolist() == [3, 3, 3, 4, 0, m, -1, -1]         # 2 candidates: the UPPER one; odd; even; zero; none
    assert ref["th_dist"][6] == 0 and ref["th_dist"][7] == 0 and len(frames[6]["pt"]) == 3 and len(frames[7]["pt"]) == 0
    # median 0: everything accepted is pruned, nothing is left, nothing is selected
    a, b = int(ref["pt_ptr"][4]), int(ref["pt_ptr"][5])
    assert (ref["code"][a:b] == S.REJ_FAR).all() and ref["n_stereo"][4] == 0 and ref["sel_ptr"][4] == ref["sel_ptr"][5]
    # (float)dist == thDist: pruned; one below: kept
    a = int(ref["pt_ptr"][5])
    assert ref["code"][a + 5] == S.REJ_FAR and ref["code"][a + 6] == S.OK and ref["n_stereo"][5] == 8
    assert (ref["code"][ref["pt_ptr"][6]:ref["pt_ptr"][7]] == S.REJ_STATUS).all()
    assert ref["n_stereo"].tolist() == [1, 2, 4, 5, 0, 8, 0, 0]


def test_the_walk_cases_give_the_references_lengths():
    frames, ref = S.walk_case(), S.walk_ref()
    n = len(S.WALK)
    assert np.diff(ref["sel_ptr"])[:n].tolist() == list(S.WALK_LENGTHS) == [min(c, max(k, 100) + 1) for c, k in S.WALK]
    assert ref["n_stereo"][:n].tolist() == [c for c, _ in S.WALK] and (ref["code"] != S.REJ_FAR).all()
    for f, (cand, close) in enumerate(S.WALK):
        a, b = int(ref["pt_ptr"][f]), int(ref["pt_ptr"][f + 1])
        z = ref["depth"][a:b]
        assert ((z > 0) & (z <= frames[f]["th_depth"])).sum() == close
        s0, s1 = int(ref["sel_ptr"][f]), int(ref["sel_ptr"][f + 1])
        zs = z[ref["sel_src"][s0:s1]]
        assert (np.diff(zs) > 0).all() and (zs == np.sort(z[z > 0])[:s1 - s0]).all()        # ascending, and the nearest ones
        want_new = 1 - frames[f]["has_point"][ref["sel_src"][s0:s1]] if "has_point" in frames[f] else np.ones(s1 - s0)
        assert (ref["sel_new"][s0:s1] == want_new).all()
    assert any("has_point" in fr for fr in frames) and any("has_point" not in fr for fr in frames)
    assert 0 < ref["sel_new"][:ref["sel_ptr"][n]].sum() < ref["sel_ptr"][n]
    # equal depths: by index inside a depth
    s0, s1 = int(ref["sel_ptr"][n]), int(ref["sel_ptr"][n + 1])
    assert ref["sel_src"][s0:s1].tolist() == [0, 2, 4, 6, 8, 10, 1, 3, 5, 7, 9, 11] and len(set(ref["depth"][ref["pt_ptr"][n]:ref["pt_ptr"][n + 1]].tolist())) == 2
    assert [fr["select"] for fr in frames[n:]] == [S.CLOSE, S.ALL, S.NONE]
    s0, s1 = int(ref["sel_ptr"][n + 1]), int(ref["sel_ptr"][n + 2])
    assert s1 - s0 == 130 and (np.diff(ref["sel_src"][s0:s1]) > 0).all() and ref["sel_ptr"][n + 3] == s1      # ALL: index order; NONE: nothing
    # max_point 0 and 1: one more than the larger of max_point and the close ones
    for max_point in (0, 1):
        got = np.diff(S.ref_stereo(frames, max_point=max_point)["sel_ptr"])[:n].tolist()
        assert got == [min(c, max(k, max_point) + 1) for c, k in S.WALK] and got[0] == max_point + 1
    assert (ref["sel_src"][ref["sel_ptr"][-1]:] == -1).all() and np.isnan(ref["sel_cam"][ref["sel_ptr"][-1]:]).all()


def test_counts_and_frames_cases_are_what_the_gpu_tests_ask_for():
    frames, ref = S.counts_case(), S.counts_ref()
    assert tuple(len(fr["pt"]) for fr in frames[:len(S.COUNTS)]) == S.COUNTS == (0, 1, 63, 64, 65, 1025, 4097, 16384)
    assert all(fr["select"] == S.CLOSE for fr in frames[:8]) and all(fr["select"] == S.ALL for fr in frames[8:])
    assert set(ref["code"].tolist()) >= {S.OK, S.REJ_STATUS, S.REJ_ROW, S.REJ_FAR}
    big = np.diff(ref["sel_ptr"])[7]
    assert 4096 < big < ref["n_stereo"][7] < 16384                  # the walk stops inside the largest frame's candidates
    assert any(fr.get("pose") is None for fr in frames) and any(fr.get("pose") is not None and abs(fr["pose"][4]) > 1e4 for fr in frames)
    assert any("pt_un" in fr for fr in frames)
    assert all("pose" not in fr for fr in S.counts_nopose_case())
    ref = S.counts_nopose_ref()
    total = int(ref["sel_ptr"][-1])
    assert total > 500 and (ref["sel_point"][:total] == ref["sel_cam"][:total].astype(np.float64)).all()
    frames, ref = S.frames_case(), S.frames_ref()
    n = np.diff(ref["pt_ptr"])
    assert len(frames) == S.N_FRAMES == 1024 and n.min() == 0 and n.max() == 3
    assert n[0] == n[1] == n[2] == n[-1] == 0 and (n[66:76] == 0).all() and (n[126:131] == 0).all() and all(n[f] == 2 for f in S.FRAMES_ALONE[1:5])
    sel = np.diff(ref["sel_ptr"])
    assert all((sel[64 * w:64 * (w + 1)] > 0).any() for w in range(16)) and ((sel == 0) & (n > 0)).any()
    assert {fr["select"] for fr in frames} == {S.NONE, S.ALL, S.CLOSE} and ref["sel_ptr"][-1] < ref["pt_ptr"][-1]
    assert S.PINNED["counts"] == S.digest(S.counts_ref()) and S.PINNED["walk"] == S.digest(S.walk_ref())


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_stereo_points")
    assert "movba_stereo_points" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_stereo_desc", built_lib.StereoDesc), ("movba_stereo_result", built_lib.StereoResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d %d %d %d %d %d %d %d\\n", MOVBA_MAX_STEREO_POINTS, MOVBA_STEREO_SELECT_NONE, MOVBA_STEREO_SELECT_ALL, MOVBA_STEREO_SELECT_CLOSE, '
            'MOVBA_STEREO_OK, MOVBA_STEREO_REJ_STATUS, MOVBA_STEREO_REJ_ROW, MOVBA_STEREO_REJ_DISPARITY, MOVBA_STEREO_REJ_FAR);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.StereoDesc, built_lib.StereoResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.StereoDesc) == 136 and C.sizeof(built_lib.StereoResult) == 96
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    assert "} movba_stereo_desc;   /* 136 bytes */" in hdr and "} movba_stereo_result; /* 96 bytes */" in hdr
    assert rows[2] == [built_lib.MAX_STEREO_POINTS, built_lib.STEREO_SELECT_NONE, built_lib.STEREO_SELECT_ALL, built_lib.STEREO_SELECT_CLOSE, built_lib.STEREO_OK,
                       built_lib.STEREO_REJ_STATUS, built_lib.STEREO_REJ_ROW, built_lib.STEREO_REJ_DISPARITY, built_lib.STEREO_REJ_FAR]
    assert rows[2][1:] == [S.NONE, S.ALL, S.CLOSE, S.OK, S.REJ_STATUS, S.REJ_ROW, S.REJ_DISPARITY, S.REJ_FAR]
    for phrase in ("the value read is\n *     indeterminate", "What stays with the caller", "prunes EVERY accepted point", "max_point + 1 where few are close"):
        assert phrase in hdr[hdr.index("Stereo depths and new map points"):]
    assert "are movba_stereo_points" in hdr[hdr.index("Sparse pyramidal Lucas-Kanade"):hdr.index("Stereo depths and new map points")]


def _small_case():
    frames = [S.random_frame(n, 40 + k, (S.CLOSE, S.ALL, S.NONE, S.CLOSE)[k], pose=S.POSE_NEAR, un=True) for k, n in enumerate((9, 5, 0, 12))]
    for fr in frames:
        if not len(fr["pt"]):
            continue
        fr["pt_status"][:2] = (1, 0)
        fr["next_pt"][:1] = fr["pt"][:1] - F(3)
    return frames


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L_ = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.stereo_desc(_small_case())
        r, out = built_lib.stereo_result(d.n_frames, len(keep["pt"]), alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
        r.status = 99
        if mutate:
            mutate(d, keep, r)
        rc = L_.movba_stereo_points(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = all((a == np.full(1, 0x77, a.dtype)[0]).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    def par(field, value):
        return lambda d, keep, r: setattr(d, field, value)

    nan, inf = float("nan"), float("inf")
    refusals = {
        "negative n_frames": par("n_frames", -1), "n_frames above the bound": par("n_frames", 1025),
        "pt_ptr not starting at 0": put("pt_ptr", 0, 1), "pt_ptr descending": put("pt_ptr", 2, 3), "pt_ptr negative": put("pt_ptr", 0, -2),
        "points above the bound": put("pt_ptr", slice(1, None), (1 << 22) + 1),
        "a frame above MOVBA_MAX_STEREO_POINTS": put("pt_ptr", slice(1, None), 16385),
        "rows 0": put("rows", 0, 0), "cols negative": put("cols", 3, -1), "select 3": put("select", 1, 3), "select -1": put("select", 0, -1),
        "max_point -1": par("max_point", -1),
        "bf 0": put("bf", 0, 0.0), "bf negative": put("bf", 1, -2.0), "bf NaN": put("bf", 2, nan), "bf inf": put("bf", 3, inf),
        "max_disparity NaN": put("max_disparity", 0, nan), "max_disparity inf": put("max_disparity", 2, inf),
        "th_depth NaN": put("th_depth", 1, nan), "th_depth -inf": put("th_depth", 3, -inf),
        "fx 0": put("cam", (0, 0), 0.0), "fy negative": put("cam", (1, 1), -1.0), "cx NaN": put("cam", (2, 2), nan), "cy inf": put("cam", (3, 3), inf),
        "max_row_diff NaN": par("max_row_diff", nan), "max_row_diff inf": par("max_row_diff", inf), "min_disparity NaN": par("min_disparity", nan),
        "min_disparity -inf": par("min_disparity", -inf),
        "pt NaN": put("pt", (0, 1), nan), "pt inf": put("pt", (2, 0), inf), "pt above 2^20": put("pt", (2, 0), 1048577.0), "pt below -2^20": put("pt", (11, 1), -1048577.0),
        "pt_un NaN": put("pt_un", (3, 0), nan), "pt_un above 2^20": put("pt_un", (20, 1), 1048577.0),
        "next_pt NaN where the status is set": put("next_pt", (0, 0), nan), "next_pt above 2^20 where the status is set": put("next_pt", (9, 1), 1048577.0),
        "pose NaN": put("poses", (0, 2), nan), "pose inf": put("poses", (3, 6), inf), "zero quaternion": put("poses", (1, slice(0, 4)), 0.0),
    }
    for field in ("pt_ptr", "pt", "next_pt", "pt_status", "rows", "cols", "bf", "max_disparity", "th_depth", "cam", "select"):
        refusals["NULL " + field] = null(field)
    for field, _, _, _ in built_lib.STEREO_ARRAYS:
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
    rc, status, clean = call(lambda d, keep, r: (setattr(d, "n_frames", 0), setattr(d, "pt_ptr", None), setattr(r, "sel_ptr", None)))
    assert rc == 0 and status == 0 and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stereo_main():
    subprocess.check_call(["make", "-C", ST_DIR, "-s", "stereo_main_asan"])
    return os.path.join(ST_DIR, "stereo_main_asan")


def run_stereo_main(exe, frames, tmp_path, **params):
    """the sanitized build of tests/stereo_points/stereo_main.cpp on one call (stereo_ref.run_stereo_main)"""
    return S.run_stereo_main(exe, frames, tmp_path, env=SAN_ENV, **params)


@pytest.mark.parametrize("case", list(S.CASES))
def test_the_librarys_steps_on_every_case(stereo_main, tmp_path, case):
    frames, ref = S.CASES[case][0](), S.CASES[case][1]()
    got = run_stereo_main(stereo_main, frames, tmp_path)
    S.compare(got, ref, case)
    # frames alone: their points are the whole buffer, so a read behind them is seen; and the same bits as in the batch
    for f in ALONE.get(case, range(len(frames))):
        alone = run_stereo_main(stereo_main, [frames[f]], tmp_path)
        S.compare(alone, S.frame_part(ref, f), f"{case}, frame {f} alone")
        S.compare(alone, S.frame_part(got, f), f"{case}, frame {f} alone against the batch", point="exact")
    if case == "counts_nopose":
        total = int(got["sel_ptr"][-1])
        assert (got["sel_point"][:total] == got["sel_cam"][:total].astype(np.float64)).all()


def test_the_librarys_steps_under_other_parameters(stereo_main, tmp_path):
    for params in (dict(max_point=0), dict(max_point=1), dict(max_point=7)):
        S.compare(run_stereo_main(stereo_main, S.walk_case(), tmp_path, **params), S.ref_stereo(S.walk_case(), **params), f"walk, {params}")
    for params in (dict(max_row_diff=1.5), dict(min_disparity=2.0), dict(min_disparity=-3.0, max_row_diff=0.0)):
        S.compare(run_stereo_main(stereo_main, S.counts_case()[4:7], tmp_path, **params), S.ref_stereo(S.counts_case()[4:7], **params), f"counts, {params}")
        S.compare(run_stereo_main(stereo_main, S.gates_case(), tmp_path, **params), S.ref_stereo(S.gates_case(), **params), f"gates, {params}")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["stereo_points_asan", "stereo_points_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/stereo_points/stereo_driver.cpp: every refusal of the header with nothing written, calls without frames, frames
    without points, optional arrays present and absent, pinned against ordinary result memory, calls of growing and shrinking
    size, the call between upload, run, download and reset of a window on the same handle, and two handles on two threads - with
    the library's host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of tests/stereo_points linked
    into one program."""
    subprocess.check_call(["make", "-C", ST_DIR, "-s", target])
    r = subprocess.run([os.path.join(ST_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "stereo driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
