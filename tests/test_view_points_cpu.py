"""movba_view_points without a GPU: properties of the numpy restatement the GPU tests compare against (tests/view_points_ref.py)
and of its committed cases; the symbol, the constants, the struct layouts and every refusal of the header through the built
library (the checks run before the handle is touched); the library's own per-item arithmetic and the serial form of its radix
select on the CPU (tests/view_points/vp_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement
on the cases of the GPU parity, gate and median tests; and the host side of the call - checks, chunk table, packing, copy-out,
handle sharing, two handles on two threads - under the sanitizers (tests/view_points: a stand-alone driver against the stand-in
runtime of tests/hipstub and a fake launch of its own)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import view_points_ref as V
from conftest import ROOT

VP_DIR = os.path.join(ROOT, "tests", "view_points")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")


# ---- the restatement and its cases ---------------------------------------------------------------------------------------

def test_parity_case_reaches_every_code_and_sits_on_no_gate():
    points, views = V.parity_case()
    ref = V.parity_ref()
    assert [len(v["items"]) for v in views] == list(V.PARITY_LENGTHS) and len(points["points"]) == 1200
    assert sorted(v["mode"] for v in views) == [0] * 3 + [1] * 3 + [2] * 3
    n = len(ref["code"])
    dropped = int(ref["near"].sum())
    print("items", n, "dropped", dropped)
    assert dropped == 0 and dropped <= 0.01 * n
    assert (np.abs(ref["z"]) >= 0.1).all()
    codes, counts = np.unique(ref["code"], return_counts=True)
    print(dict(zip(codes.tolist(), counts.tolist())))
    # every gate rejects a visible share: at least 3 % of the items of the two modes that have gates
    gated = int((ref["code"] != V.DEPTH_ITEM).sum())
    for c in (V.VISIBLE, V.FUSE_CANDIDATE, V.REJ_BEHIND, V.REJ_U, V.REJ_V, V.REJ_IMAGE, V.REJ_DIST, V.REJ_ANGLE):
        assert counts[list(codes).index(c)] >= 0.03 * gated, c
    lv = ref["level"][ref["code"] == V.VISIBLE]
    assert lv.min() == 0 and lv.max() == 7 and (ref["level"][ref["code"] != V.VISIBLE] == -1).all()
    # NaN exactly where the reference had not got to the value
    c = ref["code"]
    has_gates = c != V.DEPTH_ITEM
    assert not np.isnan(ref["z"]).any()
    assert np.array_equal(~np.isnan(ref["uv"][:, 0]), has_gates & (c != V.REJ_BEHIND))
    assert np.array_equal(~np.isnan(ref["dist"]), has_gates & ~np.isin(c, (V.REJ_BEHIND, V.REJ_U, V.REJ_V, V.REJ_IMAGE)))
    assert np.array_equal(~np.isnan(ref["view_cos"]), np.isin(c, (V.VISIBLE,)) | ((c == V.REJ_ANGLE) & (np.repeat([v["mode"] for v in views], V.PARITY_LENGTHS) == V.FRUSTUM)))
    assert np.array_equal(~np.isnan(ref["ur"]), c == V.VISIBLE) and np.array_equal(~np.isnan(ref["track_depth"]), c == V.VISIBLE)
    # the counts, and the medians: an empty DEPTH view gives -1, the others an element of their own list
    ptr = ref["view_ptr"]
    for k, v in enumerate(views):
        seg = slice(ptr[k], ptr[k + 1])
        assert ref["n_accepted"][k] == int(np.isin(c[seg], (V.VISIBLE, V.FUSE_CANDIDATE, V.DEPTH_ITEM)).sum())
        if v["mode"] != V.DEPTH:
            assert np.isnan(ref["median_depth"][k])
        elif len(v["items"]) == 0:
            assert ref["median_depth"][k] == -1.0
        else:
            assert ref["median_depth"][k] == np.sort(ref["z"][seg])[(len(v["items"]) - 1) // v["q"]]


def test_gate_case_decides_as_the_comparisons_say():
    points, views, labels, want = V.gate_case()
    ref = V.ref_view_points(points, views)
    n = len(labels)
    for i, label in enumerate(labels):
        frustum, fuse, level = want[label]
        assert ref["code"][i] == frustum and ref["code"][n + i] == fuse, label
        if level is not None:
            assert ref["level"][i] == level, label
    at = labels.index
    # the view with log 1.05: the level clamps at both ends far from a boundary
    assert ref["level"][2 * n + at("dist == 1.2 max")] == 0 and ref["level"][2 * n + at("ratio 8: level 3 of 4")] == 3
    # cos_limit 0.25: the item below 0.5 is on the new limit, and passes
    assert ref["code"][3 * n + at("viewCos below cos_limit")] == V.VISIBLE


def test_order_key_sort_is_the_median_rule():
    points, views, lists = V.median_case()
    ref = V.ref_view_points(points, views)
    for k, (v, z) in enumerate(zip(views, lists)):
        assert V.same_bits(ref["z"][ref["view_ptr"][k]:ref["view_ptr"][k + 1]], z)          # (z is the list to the bit, -0 included)
        m = ref["median_depth"][k]
        if len(z) == 0:
            assert m == -1.0
            continue
        # count ranks over the total order: numbers by value, -0 below +0, NaN above everything
        keys = V.order_key(z)
        below, equal = int((keys < V.order_key(np.array([m]))[0]).sum()), int((keys == V.order_key(np.array([m]))[0]).sum())
        r = (len(z) - 1) // v["q"]
        assert equal >= 1 and below <= r < below + equal
        fin = z[~np.isnan(z)]
        if not np.isnan(m):
            assert int((fin < m).sum()) <= r
    assert V.key_value(V.order_key(np.array([-0.0])))[0].tobytes() == np.float64(-0.0).tobytes()
    k = V.order_key(np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan]))
    assert (np.diff(k.astype(object)) > 0).all()


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_constants_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_view_points")
    assert "movba_view_points" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    hdr = open(os.path.join(ROOT, "include", "movba.h")).read()
    for name, val in (("VIEW_FRUSTUM", 0), ("VIEW_FUSE", 1), ("VIEW_DEPTH", 2), ("MAX_VIEW_BATCH", 4096), ("VP_VISIBLE", 1),
                      ("VP_FUSE_CANDIDATE", 2), ("VP_DEPTH_ITEM", 3), ("VP_REJ_BEHIND", 16), ("VP_REJ_U", 17), ("VP_REJ_V", 18),
                      ("VP_REJ_IMAGE", 19), ("VP_REJ_DIST", 20), ("VP_REJ_ANGLE", 21)):
        assert int(re.search(r"#define\s+MOVBA_%s\s+(\d+)" % name, hdr).group(1)) == val == getattr(built_lib, name), name
    assert (V.FRUSTUM, V.FUSE, V.DEPTH) == (built_lib.VIEW_FRUSTUM, built_lib.VIEW_FUSE, built_lib.VIEW_DEPTH)
    assert (V.VISIBLE, V.FUSE_CANDIDATE, V.DEPTH_ITEM, V.REJ_BEHIND, V.REJ_ANGLE) == (1, 2, 3, 16, 21)
    # the layouts the C compiler gives the header's structs are the ctypes ones
    fields = dict(movba_view_desc=[f[0] for f in built_lib.ViewDesc._fields_], movba_view_result=[f[0] for f in built_lib.ViewResult._fields_])
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, names in fields.items():
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {n}));' for n in names]
        src.append('printf("\\n");')
    src += ['return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.ViewDesc, built_lib.ViewResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.ViewDesc) == 128 and C.sizeof(built_lib.ViewResult) == 88


def _small_call(built_lib):
    rng = np.random.default_rng(3)
    points = dict(points=rng.normal(size=(50, 3)), normals=rng.normal(size=(50, 3)), max_distance=np.full(50, 9.0), min_distance=np.full(50, 0.1))
    pose = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 4.0)
    views = [dict(mode=m, pose=pose, cam=(400.0, 400.0, 320.0, 240.0), bounds=(0.0, 640.0, 0.0, 480.0), items=rng.integers(0, 50, n))
             for m, n in ((0, 20), (1, 0), (2, 30), (0, 5))]
    return points, views


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)
    points, views = _small_call(built_lib)
    nan, inf = float("nan"), float("inf")

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.view_desc(points, views)
        n, nv = len(keep["item_point"]), len(views)
        r, out = built_lib.view_result(n, nv, alloc=lambda shape, dtype: np.full(shape, 99 if dtype != np.float64 else -7.0, dtype))
        r.status = 99; r.pad = 77
        if mutate:
            mutate(d, keep, r)
        rc = L.movba_view_points(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = r.pad == 77 and all((a == (-7.0 if a.dtype == np.float64 else 99)).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    refusals = {
        "negative n_views": lambda d, keep, r: setattr(d, "n_views", -1),
        "negative n_points": lambda d, keep, r: setattr(d, "n_points", -1),
        "too many views": lambda d, keep, r: setattr(d, "n_views", built_lib.MAX_VIEW_BATCH + 1),
        "view_ptr not starting at 0": put("view_ptr", 0, 1),
        "view_ptr descending": put("view_ptr", 2, 10),
        "point index too large": put("item_point", 7, 50),
        "point index negative": put("item_point", 0, -1),
        "unknown mode": put("mode", 1, 3),
        "negative mode": put("mode", 0, -1),
        "fx zero": put("cam", (0, 0), 0.0), "fy infinite": put("cam", (1, 1), inf), "fx negative": put("cam", (2, 0), -400.0),
        "cx NaN": put("cam", (3, 2), nan), "bf infinite": put("bf", 1, inf), "bounds NaN": put("bounds", (2, 1), nan),
        "cos_limit NaN": put("cos_limit", 0, nan), "log_scale_factor infinite": put("log_scale_factor", 1, inf),
        "n_levels 0": put("n_levels", 3, 0), "q 0 on a DEPTH view": put("q", 2, 0),
        "log_scale_factor 0 on a FRUSTUM view": put("log_scale_factor", 0, 0.0),
        "log_scale_factor negative on a FRUSTUM view": put("log_scale_factor", 3, -0.2),
        "pose NaN": put("poses", (2, 5), nan), "pose infinite": put("poses", (0, 3), inf),
        "zero quaternion": put("poses", (1, slice(0, 4)), 0.0),
    }
    for field in ("mode", "poses", "cam", "view_ptr", "item_point", "points", "normals", "max_distance", "min_distance", "bounds",
                  "log_scale_factor", "n_levels", "cos_limit", "q"):
        refusals["NULL " + field] = null(field)
    for field in ("code", "n_accepted", "median_depth"):
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
    # no views: MOVBA_OK, the status and nothing else
    rc, status, clean = call(lambda d, keep, r: setattr(d, "n_views", 0))
    assert rc == 0 and status == 0 and clean


def test_views_without_items_need_no_device(built_lib):
    L = built_lib.lib()
    dummy = C.create_string_buffer(64)
    points, views = _small_call(built_lib)
    for v in views:
        v["items"] = np.zeros(0, np.int32)
    d, keep = built_lib.view_desc(points, views)
    r, out = built_lib.view_result(0, len(views))
    out["n_accepted"][:] = -5
    assert L.movba_view_points(C.cast(dummy, C.c_void_p), C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert (out["n_accepted"] == 0).all() and out["median_depth"][2] == -1.0 and np.isnan(out["median_depth"][[0, 1, 3]]).all()


# ---- the library's own arithmetic on the CPU -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vp_main():
    subprocess.check_call(["make", "-C", VP_DIR, "-s", "vp_main_asan"])
    return os.path.join(VP_DIR, "vp_main_asan")


def run_vp_main(exe, points, views, tmp_path):
    """tests/view_points/vp_main.cpp on one call -> the fields of Solver.view_points' dict"""
    from movba import capi
    d, keep = capi.view_desc(points, views)
    n, nv, npnt = len(keep["item_point"]), len(views), len(keep["points"])
    table = "normals" in keep
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([npnt, nv, n, int(table)], np.int32).tobytes())
        for key in ("mode", "n_levels", "q", "view_ptr", "item_point", "points") + (("normals", "max_distance", "min_distance") if table else ()) + \
                ("poses", "cam", "bf", "bounds", "log_scale_factor", "cos_limit"):
            f.write(keep[key].tobytes())
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "vp_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    out, at = dict(status=0, view_ptr=keep["view_ptr"]), 0
    for key, dtype, count in (("code", np.uint8, n), ("level", np.int32, n), ("n_accepted", np.int32, nv), ("z", np.float64, n),
                              ("uv", np.float64, 2 * n), ("dist", np.float64, n), ("view_cos", np.float64, n), ("ur", np.float64, n),
                              ("track_depth", np.float64, n), ("median_depth", np.float64, nv)):
        out[key] = np.frombuffer(blob, dtype, count, at)
        at += count * np.dtype(dtype).itemsize
    assert at == len(blob)
    out["uv"] = out["uv"].reshape(-1, 2)
    return out


def test_the_librarys_arithmetic_on_the_parity_case(vp_main, tmp_path):
    points, views = V.parity_case()
    V.compare(run_vp_main(vp_main, points, views, tmp_path), V.parity_ref(), "parity")


def test_the_librarys_arithmetic_on_the_gates(vp_main, tmp_path):
    points, views, labels, want = V.gate_case()
    got = run_vp_main(vp_main, points, views, tmp_path)
    ref = V.ref_view_points(points, views)
    assert np.array_equal(got["code"], ref["code"]) and np.array_equal(got["level"], ref["level"]) and np.array_equal(got["n_accepted"], ref["n_accepted"])
    for key in V.VALUE_KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), key          # (every quantity is exact)


def test_the_serial_radix_select_on_the_median_lists(vp_main, tmp_path):
    points, views, lists = V.median_case()
    got = run_vp_main(vp_main, points, views, tmp_path)
    ref = V.ref_view_points(points, views)
    assert V.same_bits(got["median_depth"], ref["median_depth"]) and np.array_equal(got["n_accepted"], [len(z) for z in lists])
    assert V.same_bits(got["z"], ref["z"])


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["view_points_asan", "view_points_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/view_points/view_points_driver.cpp: every refusal of the header with nothing written, a call without views, empty
    views, optional arrays left out, pinned against ordinary result memory, a call between the upload and the runs of a window
    on the same handle, and two handles on two threads - with the library's host sources, the stand-in runtime and fakes of
    tests/hipstub and the fake launch of tests/view_points linked into one program."""
    subprocess.check_call(["make", "-C", VP_DIR, "-s", target])
    r = subprocess.run([os.path.join(VP_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "view_points driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
