"""movba_covisibility without a GPU: properties of the restatement the GPU tests compare against (tests/covisibility_ref.py) and
of its committed cases; the symbol, the struct layouts and every refusal of the header through the built library (the checks run
before the handle is touched); the library's own per-query steps on the CPU (tests/covisibility/cv_main.cpp, under
AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement on the cases of the GPU tests; and the host side of the
call - checks, packing, copy-out, pinned and ordinary results, a handle shared with a window, two handles on two threads - under
the sanitizers (tests/covisibility: a stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its
own).  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covisibility_ref as R
from conftest import ROOT

CV_DIR = os.path.join(ROOT, "tests", "covisibility")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")


# ---- the restatement and its cases ---------------------------------------------------------------------------------------

def _order(ref, q):
    n = int(ref["n_counted"][q])
    return ref["out_view"][q, :n], ref["out_weight"][q, :n]


def test_parity_case_is_what_the_gpu_test_asks_for():
    case, ref = R.parity_case(), R.parity_ref()
    nq = len(case["queries"])
    assert case["n_views"] == 300 and len(case["lists"]) == 2000 and nq == 40 and case["min_weight"] == 15
    assert sorted(set(len(l) for l in case["lists"])) == sorted(R.PARITY_LIST_LENGTHS)
    assert sorted(set(len(q) for q in case["queries"])) == sorted(R.PARITY_QUERY_LENGTHS)
    hub = next(l for l in case["lists"] if len(l) == 300)
    assert sorted(hub.tolist()) == list(range(300))                                     # a hub is seen by every view
    assert any(len(set(q.tolist())) < len(q) for q in case["queries"])                  # some queries repeat a point
    zeros = int((case["eligible"] == 0).sum())
    assert 15 <= zeros <= 45 and case["eligible"][R.HIDDEN_BEST] == 0                   # about 10 %
    # query_self: inside the lists, outside them, -1
    named = [set(int(v) for p in q for v in case["lists"][p]) for q in case["queries"]]
    selfs = case["query_self"]
    assert any(s >= 0 and s in named[q] for q, s in enumerate(selfs)) and any(s >= 0 and s not in named[q] and named[q] for q, s in enumerate(selfs))
    assert (selfs == -1).sum() >= 10
    # a view that would otherwise be best is not eligible
    open_ref = R.ref_covisibility(**dict(case, eligible=None))
    assert open_ref["best_view"][5] == R.HIDDEN_BEST and ref["best_view"][5] != R.HIDDEN_BEST and R.HIDDEN_BEST not in ref["out_view"][5]
    counted, best_w = ref["n_counted"], ref["best_weight"]
    fallback = [q for q in range(nq) if counted[q] > 0 and best_w[q] < 15]
    assert fallback and all(ref["n_connected"][q] == 1 for q in fallback)               # no view reaches 15, counts > 0
    top_tie = [q for q in range(nq) if counted[q] > 1 and ref["out_weight"][q, 0] == ref["out_weight"][q, 1]]
    assert top_tie and all(ref["best_view"][q] != ref["out_view"][q, 0] and ref["best_view"][q] < ref["out_view"][q, 0] for q in top_tie)
    assert any(best_w[q] >= 15 for q in top_tie)                                        # one of them above the threshold
    assert any(ref["best_view"][q] != ref["out_view"][q, 0] for q in fallback)          # the fallback's connection is not the front
    below = 0
    for q in range(nq):
        w = _order(ref, q)[1]
        w = w[w < w[0]] if len(w) else w
        below += bool(len(w) and np.bincount(w).max() >= 3)
    assert below >= 5                                                                    # ties of three or more below the top
    assert any(len(q) == 0 for q in case["queries"])
    assert any(len(q) > 0 and counted[k] == 0 for k, q in enumerate(case["queries"]))   # only empty-list or ineligible observers
    assert counted[8] == 0 and counted[15] == 0 and len(case["lists"][case["queries"][15][0]]) == 1
    assert any(0 < ref["n_connected"][q] < counted[q] and ref["n_connected"][q] > 1 for q in range(nq))


def test_restatement_orders_counts_and_picks_as_the_header_says():
    case, ref = R.parity_case(), R.parity_ref()
    for q, counter in enumerate(ref["counters"]):
        views, weights = _order(ref, q)
        assert len(counter) == ref["n_counted"][q] and sorted(views.tolist()) == sorted(counter)
        assert all(counter[int(v)] == w for v, w in zip(views, weights))
        keys = weights.astype(np.int64) * (1 << 32) + views
        assert (np.diff(keys) < 0).all()                                                # weight descending, ties by view descending
        assert (ref["out_view"][q, len(views):] == -1).all() and (ref["out_weight"][q, len(views):] == 0).all()
        if counter:
            top = max(counter.values())
            assert ref["best_weight"][q] == top and ref["best_view"][q] == min(v for v, w in counter.items() if w == top)
            reaching = int((weights >= 15).sum())
            assert ref["n_connected"][q] == (reaching if reaching else 1)
        else:
            assert ref["best_view"][q] == -1 and ref["best_weight"][q] == 0 and ref["n_connected"][q] == 0
        self_view = int(case["query_self"][q])
        assert self_view not in counter and all(case["eligible"][v] for v in counter)
    # a point in two slots counts twice; a list that names a view twice counts it twice
    one = R.ref_covisibility(3, [[0, 1], [1, 1, 2]], [[0], [0, 0], [1]], max_out=3)
    assert one["out_weight"].tolist() == [[1, 1, 0], [2, 2, 0], [2, 1, 0]] and one["out_view"].tolist() == [[1, 0, -1], [1, 0, -1], [1, 2, -1]]
    # a shorter hand-out is a prefix, and the scalars do not change
    short = R.ref_covisibility(**dict(case, max_out=7))
    assert np.array_equal(short["out_view"], ref["out_view"][:, :7]) and np.array_equal(short["n_counted"], ref["n_counted"])
    assert np.array_equal(short["n_connected"], ref["n_connected"])


def test_wide_and_tiny_cases_are_what_the_gpu_test_asks_for():
    case, ref = R.wide_case(), R.wide_ref()
    assert case["n_views"] == 8192 and len(case["lists"]) == 64 and len(case["queries"]) == 3 and case["max_out"] == 8192
    assert max(len(l) for l in case["lists"]) == 8192 and min(len(l) for l in case["lists"]) == 1
    assert ref["n_counted"].tolist() == [8192, 8192, 8191]                              # the largest sort; the self entry is missing
    assert (ref["out_weight"][1] == 1).all() and np.array_equal(ref["out_view"][1], np.arange(8191, -1, -1))
    assert ref["best_view"][1] == 0 and ref["n_connected"][1] == 1
    assert 4000 not in ref["out_view"][2] and ref["out_view"][2, -1] == -1
    short = R.wide_ref(7)
    assert short["out_view"].shape == (3, 7) and np.array_equal(short["out_view"], ref["out_view"][:, :7])
    a, b = R.ref_covisibility(**R.tiny_case(0), max_out=1), R.ref_covisibility(**R.tiny_case(-1), max_out=1)
    assert [a[k].tolist() for k in R.KEYS] == [[0], [0], [-1], [0], [[-1]], [[0]]]
    assert [b[k].tolist() for k in R.KEYS] == [[1], [1], [0], [1], [[0]], [[1]]]


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_covisibility")
    assert "movba_covisibility" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_covis_desc", built_lib.CovisDesc), ("movba_covis_result", built_lib.CovisResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d\\n", MOVBA_MAX_COVIS_VIEWS, MOVBA_MAX_COVIS_QUERIES);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.CovisDesc, built_lib.CovisResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.CovisDesc) == 72 and C.sizeof(built_lib.CovisResult) == 56
    assert rows[2] == [8192, 4096] == [built_lib.MAX_COVIS_VIEWS, built_lib.MAX_COVIS_QUERIES]


def _small_case():
    rng = np.random.default_rng(3)
    lists = [rng.integers(0, 6, n).astype(np.int32) for n in (3, 0, 1, 5, 2, 0, 4, 4)]
    queries = [np.array(q, np.int32) for q in ([0, 3, 3], [], [2, 7, 6, 4], [1, 5])]
    return dict(n_views=6, lists=lists, queries=queries, query_self=np.array([2, -1, 0, 5], np.int32), eligible=np.array([1, 1, 0, 1, 1, 1], np.uint8),
                min_weight=15, max_out=4)


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.covis_desc(**_small_case())
        r, out = built_lib.covis_result(d.n_queries, d.max_out, alloc=lambda shape, dtype: np.full(shape, -7, dtype))
        r.status = 99; r.pad = 77
        if mutate:
            mutate(d, keep, r)
        rc = L.movba_covisibility(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = r.pad == 77 and all((a == -7).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    def count(field, value):
        return lambda d, keep, r: setattr(d, field, value)

    def huge(key):                      # n_obs / n_items above 2^28: the prefix says so, nothing behind it is read
        return lambda d, keep, r: keep[key].__setitem__(slice(1, None), (1 << 28) + 1)

    refusals = {
        "negative n_views": count("n_views", -1), "negative n_points": count("n_points", -1), "negative n_queries": count("n_queries", -1),
        "negative max_out": count("max_out", -1), "n_views above the bound": count("n_views", 8193), "n_queries above the bound": count("n_queries", 4097),
        "n_obs above 2^28": huge("obs_ptr"), "n_items above 2^28": huge("query_ptr"), "n_queries x max_out above 2^28": count("max_out", (1 << 26) + 1),
        "min_weight 0": count("min_weight", 0), "min_weight negative": count("min_weight", -3),
        "obs_ptr not starting at 0": put("obs_ptr", 0, 1), "obs_ptr descending": put("obs_ptr", 4, 2),
        "query_ptr not starting at 0": put("query_ptr", 0, 1), "query_ptr descending": put("query_ptr", 2, 1),
        "observer too large": put("obs_view", 2, 6), "observer negative": put("obs_view", 0, -1),
        "point too large": put("query_point", 1, 8), "point negative": put("query_point", 0, -1),
        "query_self too large": put("query_self", 0, 6), "query_self below -1": put("query_self", 1, -2),
        "fewer views than the lists name": count("n_views", 5), "fewer points than the items name": count("n_points", 7),
    }
    for field in ("obs_ptr", "obs_view", "query_ptr", "query_point"):
        refusals["NULL " + field] = null(field)
    for field in R.KEYS:
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
    # no queries: MOVBA_OK, the status and nothing else - but the counts are still looked at
    rc, status, clean = call(count("n_queries", 0))
    assert rc == 0 and status == 0 and clean
    rc, status, clean = call(lambda d, keep, r: (setattr(d, "n_queries", 0), setattr(d, "min_weight", 0)))
    assert rc == built_lib.ERR_ARG and status == built_lib.ERR_ARG and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cv_main():
    subprocess.check_call(["make", "-C", CV_DIR, "-s", "cv_main_asan"])
    return os.path.join(CV_DIR, "cv_main_asan")


def run_cv_main(exe, case, tmp_path):
    """tests/covisibility/cv_main.cpp on one call -> the fields of Solver.covisibility's dict"""
    from movba import capi
    d, keep = capi.covis_desc(**case)
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([d.n_views, d.n_points, d.n_queries, d.min_weight, d.max_out, len(keep["obs_view"]), len(keep["query_point"]),
                          int("query_self" in keep), int("eligible" in keep)], np.int32).tobytes())
        for key in ("obs_ptr", "obs_view", "query_ptr", "query_point", "query_self", "eligible"):
            if key in keep:
                f.write(keep[key].tobytes())
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cv_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = np.frombuffer(open(dst, "rb").read(), np.int32)
    nq, mo = d.n_queries, d.max_out
    assert len(blob) == 4 * nq + 2 * nq * mo
    out = {key: blob[k * nq:(k + 1) * nq] for k, key in enumerate(R.KEYS[:4])}
    out["out_view"], out["out_weight"] = blob[4 * nq:4 * nq + nq * mo].reshape(nq, mo), blob[4 * nq + nq * mo:].reshape(nq, mo)
    return out


def test_the_librarys_steps_on_the_parity_case(cv_main, tmp_path):
    R.compare(run_cv_main(cv_main, R.parity_case(), tmp_path), R.parity_ref(), "parity")
    R.compare(run_cv_main(cv_main, dict(R.parity_case(), max_out=7), tmp_path), R.ref_covisibility(**dict(R.parity_case(), max_out=7)), "parity, 7 handed out")


def test_the_librarys_steps_on_the_wide_case(cv_main, tmp_path):
    for max_out in (8192, 7):
        R.compare(run_cv_main(cv_main, R.wide_case(max_out), tmp_path), R.wide_ref(max_out), f"wide {max_out}")


def test_the_librarys_steps_on_the_tiny_case(cv_main, tmp_path):
    for self_view in (0, -1):
        case = dict(R.tiny_case(self_view), max_out=1)
        R.compare(run_cv_main(cv_main, case, tmp_path), R.ref_covisibility(**case), f"tiny {self_view}")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["covisibility_asan", "covisibility_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/covisibility/covisibility_driver.cpp: every refusal of the header with nothing written, calls without queries, the
    optional arrays left out, pinned against ordinary result memory, calls of growing and shrinking size up to the bounds, the
    call between upload, run, download and reset of a window on the same handle, and two handles on two threads - with the
    library's host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of tests/covisibility linked into
    one program."""
    subprocess.check_call(["make", "-C", CV_DIR, "-s", target])
    r = subprocess.run([os.path.join(CV_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "covisibility driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
