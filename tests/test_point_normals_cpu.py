"""movba_point_normals and movba_lba_point_normals without a GPU: properties of the restatement the GPU tests compare against
(tests/point_normals_ref.py) and of its committed cases; the symbols, the struct layouts and every refusal of the header through
the built library (the checks run before the handle is touched); the library's own per-point arithmetic on the CPU
(tests/point_normals/pn_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement on the cases of
the GPU tests; and the host side of both calls - checks, packing, copy-out, pinned and ordinary results, MOVBA_ERR_STATE, the
resident variant against the array variant, two handles on two threads - under the sanitizers (tests/point_normals: a
stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its own).  No sanitizer touches code
loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import point_normals_ref as N
from conftest import ROOT

PN_DIR = os.path.join(ROOT, "tests", "point_normals")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")


# ---- the restatement and its cases ---------------------------------------------------------------------------------------

def test_parity_case_is_what_the_gpu_test_asks_for():
    case, ref = N.parity_case(), N.parity_ref()
    assert case["views"].shape == (300, 7) and case["points"].shape == (1000, 3)
    assert sorted(set(len(l) for l in case["lists"])) == sorted(N.PARITY_LENGTHS)
    assert all(len(set(l.tolist())) == len(l) for l in case["lists"])
    assert set(case["ref_level"].tolist()) == set(range(8))
    t = np.linalg.norm(case["views"][:, 4:], axis=1)
    assert t.max() <= 10.0 and np.abs(np.linalg.norm(case["views"][:, :4], axis=1) - 1.0).max() > 0.1       # (general position, not normalised)
    Ow = np.array([N.centre(v) for v in case["views"]])
    assert np.linalg.norm(case["points"][:, None, :] - Ow[None, :, :], axis=2).min() >= 0.5
    # a reference outside the list, and an unreadable one on an empty list
    assert any(len(l) and case["ref_view"][p] not in l for p, l in enumerate(case["lists"]))
    assert any(len(l) == 0 and case["ref_view"][p] == -1 for p, l in enumerate(case["lists"]))
    empty = np.array([len(l) == 0 for l in case["lists"]])
    for key in N.KEYS:
        assert np.array_equal(np.isnan(ref[key]).reshape(1000, -1).all(axis=1), empty), key      # NaN for empty lists, and only there
        assert np.array_equal(np.isnan(ref[key]).reshape(1000, -1).any(axis=1), empty), key


def test_restatement_sums_unit_terms_counts_observations_and_scales():
    case, ref = N.parity_case(), N.parity_ref()
    for p, terms in enumerate(ref["terms"]):
        assert len(terms) == len(case["lists"][p])                      # n is counted per observation
        if terms:
            assert np.abs(np.array(terms) - 1.0).max() <= 4e-16         # every term has unit length
            assert np.linalg.norm(ref["normals"][p]) <= 1.0 + 1e-15     # so their mean is no longer than 1
    ok = ~np.isnan(ref["max_distance"])
    assert N.same_bits(ref["min_distance"][ok], ref["max_distance"][ok] / N.SCALE_12[-1])
    # a point seen once has the unit vector itself; seen twice from the same side, their mean
    one = [p for p, l in enumerate(case["lists"]) if len(l) == 1]
    for p in one[:20]:
        d = case["points"][p] - N.centre(case["views"][case["lists"][p][0]])
        np.testing.assert_allclose(ref["normals"][p], d / np.linalg.norm(d), rtol=0, atol=1e-15)
    # the distances against numpy's own norm
    for p in np.flatnonzero(ok)[:50]:
        dist = np.linalg.norm(case["points"][p] - N.centre(case["views"][case["ref_view"][p]]))
        np.testing.assert_allclose(ref["max_distance"][p], dist * N.SCALE_12[case["ref_level"][p]], rtol=1e-15)
    # a duplicated observer counts twice
    sub = N.subset(case, [2])
    twice = dict(sub, lists=[np.concatenate([sub["lists"][0], sub["lists"][0][:1]])])
    a, b = N.ref_point_normals(**sub), N.ref_point_normals(**twice)
    assert len(b["terms"][0]) == len(a["terms"][0]) + 1 and not N.same_bits(a["normals"], b["normals"])


def test_exact_case_is_exact():
    for table in (N.SCALE_12, N.SCALE_POW2, np.array([2.0])):
        case = N.exact_case(table)
        ref = N.ref_point_normals(**case)
        Ow = np.array([N.centre(v) for v in case["views"]])
        assert np.array_equal(Ow, np.round(Ow))
        for p, l in enumerate(case["lists"]):
            d = case["points"][p] - Ow[l]
            length = np.sqrt((d * d).sum(axis=1))
            assert np.array_equal(length, np.round(length))              # integer lengths: Pythagorean triples, or 0
            assert set(length.tolist()) <= {0.0} | {m * s for m in (3.0, 7.0, 9.0, 11.0) for s in (1.0, 2.0, 4.0)}
        assert np.isnan(ref["normals"][5]).all() and ref["max_distance"][5] == 0.0 and ref["min_distance"][5] == 0.0
        assert np.isnan(ref["normals"][6]).all() and ref["max_distance"][6] > 0.0
        others = [p for p in range(len(case["lists"])) if p not in (5, 6)]
        assert not np.isnan(ref["normals"][others]).any()
        if len(table) == 1:
            assert N.same_bits(ref["min_distance"], ref["max_distance"] / 2.0)
    # sequential order and division are observable on this case: a pairwise sum, or a reciprocal, changes bits somewhere
    case = N.exact_case()
    ref = N.ref_point_normals(**case)
    rev = N.ref_point_normals(**dict(case, lists=[l[::-1] for l in case["lists"]]))
    assert not N.same_bits(ref["normals"], rev["normals"])
    Ow = np.array([N.centre(v) for v in case["views"]])
    recip = np.array([((case["points"][p] - Ow[l]) * (1.0 / np.linalg.norm(case["points"][p] - Ow[l], axis=1))[:, None]).sum(axis=0) / len(l)
                      for p, l in enumerate(case["lists"]) if p not in (5, 6)])
    assert not N.same_bits(recip, ref["normals"][[p for p in range(len(case["lists"])) if p not in (5, 6)]])


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbols_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        for name in ("movba_point_normals", "movba_lba_point_normals"):
            assert hasattr(built_lib.lib(hooks), name)
            assert name in built_lib.EXPORTS
    assert built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_normals_desc", built_lib.NormalsDesc), ("movba_normals_result", built_lib.NormalsResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.NormalsDesc, built_lib.NormalsResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.NormalsDesc) == 72 and C.sizeof(built_lib.NormalsResult) == 32


def _small_case():
    rng = np.random.default_rng(3)
    lists = [rng.integers(0, 6, n).astype(np.int32) for n in (3, 0, 1, 5, 2, 0, 4, 4)]
    return dict(points=rng.normal(size=(8, 3)) + 5.0, views=np.concatenate([rng.normal(size=(6, 4)), rng.normal(size=(6, 3))], 1), lists=lists,
                ref_view=np.array([0, -1, 2, 5, 1, 99, 3, 4], np.int32), ref_level=np.arange(8, dtype=np.int32) % 8, scale_factors=N.SCALE_12.copy())


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.normals_desc(**_small_case())
        r, out = built_lib.normals_result(d.n_points, alloc=lambda shape, dtype: np.full(shape, -7.0, dtype))
        r.status = 99; r.pad = 77
        if mutate:
            mutate(d, keep, r)
        rc = L.movba_point_normals(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = r.pad == 77 and all((a == -7.0).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    def count(field, value):
        return lambda d, keep, r: setattr(d, field, value)

    def huge(d, keep, r):               # n_obs above 2^28: the prefix says so, nothing behind it is read
        keep["obs_ptr"][1:] = (1 << 28) + 1

    refusals = {
        "negative n_views": count("n_views", -1), "negative n_points": count("n_points", -1), "negative n_levels": count("n_levels", -1),
        "n_levels 0": count("n_levels", 0), "n_obs above 2^28": huge,
        "obs_ptr not starting at 0": put("obs_ptr", 0, 1), "obs_ptr descending": put("obs_ptr", 4, 2),
        "observer too large": put("obs_view", 2, 6), "observer negative": put("obs_view", 0, -1),
        "ref_view too large on a point with observers": put("ref_view", 0, 6), "ref_view negative on a point with observers": put("ref_view", 3, -1),
        "ref_level too large": put("ref_level", 7, 8), "ref_level negative": put("ref_level", 2, -1),
        "ref_level too large on a point without observers": put("ref_level", 1, 8),
        "ref_level beyond a shorter table": count("n_levels", 7),
        "scale factor zero": put("scale_factors", 3, 0.0), "scale factor negative": put("scale_factors", 0, -1.2),
        "scale factor infinite": put("scale_factors", 7, inf), "scale factor NaN": put("scale_factors", 1, nan),
        "pose NaN": put("poses", (2, 5), nan), "pose infinite": put("poses", (0, 3), inf), "zero quaternion": put("poses", (1, slice(0, 4)), 0.0),
    }
    for field in ("poses", "points", "obs_ptr", "obs_view", "ref_view", "ref_level", "scale_factors"):
        refusals["NULL " + field] = null(field)
    for field in ("normals", "max_distance", "min_distance"):
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
    # no points: MOVBA_OK, the status and nothing else
    rc, status, clean = call(count("n_points", 0))
    assert rc == 0 and status == 0 and clean
    # the resident variant: NULL arguments and n_levels < 1 are refused before the handle is looked at
    a3, a1, b1 = np.full(3, -7.0), np.full(1, -7.0), np.full(1, -7.0)
    z, s = np.zeros(1, np.int32), np.ones(1)
    _i, _d = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    good = [h, z.ctypes.data_as(_i), z.ctypes.data_as(_i), s.ctypes.data_as(_d), 1, None, a3.ctypes.data_as(_d), a1.ctypes.data_as(_d), b1.ctypes.data_as(_d)]
    for k in (0, 1, 2, 3, 6, 7, 8):
        args = list(good); args[k] = None
        assert L.movba_lba_point_normals(*args) == built_lib.ERR_ARG, k
    for n_levels in (0, -3):
        args = list(good); args[4] = n_levels
        assert L.movba_lba_point_normals(*args) == built_lib.ERR_ARG
    assert (a3 == -7.0).all() and (a1 == -7.0).all() and (b1 == -7.0).all()


def test_points_without_observations_need_no_device(built_lib):
    L = built_lib.lib()
    dummy = C.create_string_buffer(64)
    case = dict(_small_case(), lists=[[] for _ in range(8)])
    d, keep = built_lib.normals_desc(**case)
    r, out = built_lib.normals_result(8)
    assert L.movba_point_normals(C.cast(dummy, C.c_void_p), C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all(np.isnan(out[key]).all() for key in N.KEYS)


# ---- the library's own arithmetic on the CPU -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pn_main():
    subprocess.check_call(["make", "-C", PN_DIR, "-s", "pn_main_asan"])
    return os.path.join(PN_DIR, "pn_main_asan")


def run_pn_main(exe, case, tmp_path, perm=None, mask=None):
    """tests/point_normals/pn_main.cpp on one call -> the fields of Solver.point_normals' dict; perm, mask: the resident variant's
    list source (grouped position -> caller edge, flags by caller edge)"""
    from movba import capi
    d, keep = capi.normals_desc(**case)
    n_obs = len(keep["obs_view"])
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([d.n_views, d.n_points, d.n_levels, n_obs, int(mask is not None)], np.int32).tobytes())
        for key in ("poses", "points", "obs_ptr", "obs_view", "ref_view", "ref_level", "scale_factors"):
            f.write(keep[key].tobytes())
        if mask is not None:
            f.write(np.ascontiguousarray(perm, np.int32).tobytes())
            f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pn_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = np.frombuffer(open(dst, "rb").read(), np.float64)
    n = d.n_points
    assert len(blob) == 5 * n
    return dict(status=0, normals=blob[:3 * n].reshape(n, 3), max_distance=blob[3 * n:4 * n], min_distance=blob[4 * n:])


def test_the_librarys_arithmetic_on_the_parity_case(pn_main, tmp_path):
    N.compare(run_pn_main(pn_main, N.parity_case(), tmp_path), N.parity_ref(), "parity")


def test_the_librarys_arithmetic_on_the_exact_case(pn_main, tmp_path):
    for table in (N.SCALE_12, N.SCALE_POW2, np.array([2.0])):
        case = N.exact_case(table)
        got, ref = run_pn_main(pn_main, case, tmp_path), N.ref_point_normals(**case)
        for key in N.KEYS:
            assert N.same_bits(got[key], ref[key]), (len(table), key)


def test_a_masked_permuted_list_source_is_the_filtered_list(pn_main, tmp_path):
    """The resident variant's list source on the CPU: the lists of the parity case, a random permutation between list position
    and flag, every third point's flags all set: the bits of the call over the lists without the flagged entries."""
    case = N.parity_case()
    rng = np.random.default_rng(9)
    n_obs = sum(len(l) for l in case["lists"])
    perm = rng.permutation(n_obs).astype(np.int32)
    flag_at = rng.random(n_obs) < 0.3                   # by list position
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in case["lists"]])])
    for p in range(0, 1000, 3):
        flag_at[ptr[p]:ptr[p + 1]] = True
    mask = np.zeros(n_obs, np.uint8)
    mask[perm] = flag_at
    filtered = dict(case, lists=[l[~flag_at[ptr[p]:ptr[p + 1]]] for p, l in enumerate(case["lists"])])
    # (a point whose entries are all flagged has an empty list: its reference entry is not read in either form)
    got = run_pn_main(pn_main, case | dict(ref_view=np.where([len(l) == 0 for l in case["lists"]], 0, case["ref_view"]).astype(np.int32)), tmp_path, perm, mask)
    want = run_pn_main(pn_main, filtered, tmp_path)
    for key in N.KEYS:
        assert N.same_bits(got[key], want[key]), key
    assert np.isnan(got["max_distance"][::3]).all() and not np.isnan(got["max_distance"]).all()
    N.compare(want, N.ref_point_normals(**filtered), "filtered")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["point_normals_asan", "point_normals_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/point_normals/point_normals_driver.cpp: every refusal of the header with nothing written, calls without points and
    without observations, pinned against ordinary result memory, MOVBA_ERR_STATE before an upload, before a run and after a
    reset, the resident variant against the array variant on grouped and shuffled edges with and without flags, the window's
    downloads and runs around the calls, and two handles on two threads - with the library's host sources, the stand-in runtime
    and fakes of tests/hipstub and the fake launch of tests/point_normals linked into one program."""
    subprocess.check_call(["make", "-C", PN_DIR, "-s", target])
    r = subprocess.run([os.path.join(PN_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "point_normals driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
