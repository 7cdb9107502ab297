"""movba_track_match without a GPU: the restatement the GPU tests compare against (tests/track_match_ref.py) on one hand-built case
per rule of the header, its dict-based fast version against the literal one on every small case, and the committed cases; the
symbol, the struct layouts and every refusal of the header through the built library (the checks run before the handle is
touched); the library's own steps on the CPU (tests/track_match/tm_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer)
against the restatement on the cases of the GPU tests; and the host side of the call - checks, packing, copy-out, pinned and
ordinary results, a handle shared with a window, two handles on two threads - under the sanitizers (tests/track_match: a
stand-alone driver against the stand-in runtime of tests/hipstub and a fake launch of its own).  No sanitizer touches code loaded
into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_match_ref as R
from conftest import ROOT

TM_DIR = os.path.join(ROOT, "tests", "track_match")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
T, L = R.TM_TRIANGULATION, R.TM_LOOKUP


# ---- the restatement and its cases ---------------------------------------------------------------------------------------

def _answers(res, queries):
    out = []
    for query, row in zip(queries, R.rows(res, range(len(queries)))):
        out.append(list(zip(row[0], row[1])) if query[0] == T else row[3])
    return out


@pytest.mark.parametrize("label,views,queries,want", R.hand_cases(), ids=[c[0] for c in R.hand_cases()])
def test_restatement_behaves_as_the_header_says(label, views, queries, want):
    for literal in (True, False):
        res = R.ref_track_match(views, queries, literal)
        assert _answers(res, queries) == want, (label, literal)
        counts = [len(w) if q[0] == T else 0 for q, w in zip(queries, want)]
        assert res["pair_ptr"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() and res["n_matches"] == sum(counts)
        assert res["n_found"].tolist() == [0 if q[0] == T else sum(1 for j in w if j >= 0) for q, w in zip(queries, want)]
        assert (res["match_slot1"][res["n_matches"]:] == -1).all() and (res["match_slot2"][res["n_matches"]:] == -1).all()
        assert len(res["match_slot1"]) == sum(len(views[q[1]]["track"]) for q in queries if q[0] == T)


def test_fast_restatement_equals_the_literal_one_on_every_small_case():
    for label, views, queries, _ in R.hand_cases():
        R.compare(R.ref_track_match(views, queries, literal=False), R.ref_track_match(views, queries), label)
    R.compare(R.ref_track_match(*R.mixed_case(), literal=False), R.mixed_ref(), "mixed")
    _, views, queries = R.chain_case()
    R.compare(R.ref_track_match(views, queries, literal=False), R.ref_track_match(views, queries), "chain")
    # and on a cut of the large case that the double loop still walks quickly
    views, _ = R.full_case()
    cut = [{k: v[:700] for k, v in views[0].items()}, views[1]]
    queries = [(T, 0, 0), (T, 0, 1), (T, 1, 0), (L, 0, views[0]["track"][300:900].copy())]
    R.compare(R.ref_track_match(cut, queries, literal=False), R.ref_track_match(cut, queries), "cut of the full case")


def test_mixed_case_is_what_the_gpu_test_asks_for():
    views, queries = R.mixed_case()
    ref = R.mixed_ref()
    sizes = [len(v["track"]) for v in views]
    assert tuple(sizes[:9]) == R.MIXED_SIZES and 38 <= len(queries) <= 42
    modes = [q[0] for q in queries]
    assert modes.count(T) >= 15 and modes.count(L) >= 15
    slots = sum(sizes[:9])
    repeats = sum(n - len(set(v["track"].tolist())) for n, v in zip(sizes[:9], views[:9]))
    assert 0.18 <= repeats / slots <= 0.32                                                # about a quarter of the slots repeat an id
    taken = sum(int(v["taken"].sum()) for v in views[:9])
    assert 0.45 <= taken / slots <= 0.55                                                  # half the slots are taken
    assert views[9]["taken"].all() and len(set(views[10]["track"].tolist())) == 1
    assert any(q[0] == T and q[1] == q[2] and sizes[q[1]] > 256 for q in queries)       # a view against itself
    assert any(q[0] == L and len(q[2]) == 0 for q in queries)                           # a LOOKUP without items
    look = [k for k, q in enumerate(queries) if q[0] == L and len(q[2])]
    assert any(0 < ref["n_found"][k] < len(queries[k][2]) for k in look)                 # some items are absent from their view
    # the view with every slot taken matches nothing in either role but is found by LOOKUP; the one-id view joins its lowest free slot
    counts = np.diff(ref["pair_ptr"])
    for k, q in enumerate(queries):
        if q[0] == T and 9 in q[1:]:
            assert counts[k] == 0
        if q[0] == L and q[1] == 9 and len(q[2]) == 40:          # (the lookup of the view's own first 40 ids)
            assert ref["n_found"][k] == 40
    k = queries.index((T, 10, 10))
    low = int(np.flatnonzero(views[10]["taken"] == 0)[0])
    a, b = ref["pair_ptr"][k], ref["pair_ptr"][k + 1]
    assert low == 3 and b - a == int((views[10]["taken"] == 0).sum()) and (ref["match_slot2"][a:b] == low).all()
    assert (np.diff(ref["match_slot1"][a:b]) > 0).all()
    # matches of every query ascend in i; some j is shared by two i
    shared = False
    for k in range(len(queries)):
        a, b = ref["pair_ptr"][k], ref["pair_ptr"][k + 1]
        assert (np.diff(ref["match_slot1"][a:b]) > 0).all()
        shared |= len(set(ref["match_slot2"][a:b].tolist())) < b - a
    assert shared and 0 < ref["n_matches"] < len(ref["match_slot1"])
    # the payload: distinct words per slot, NaNs with payload bits among them
    words = np.concatenate([R.bits(v["obs"]).reshape(-1) for v in views] + [R.bits(v["ur"]) for v in views] + [R.bits(v["depth"]) for v in views])
    assert len(set(words.tolist())) == len(words)
    nans = np.isnan(words.view(np.float64))
    assert nans.any() and len(set(words[nans].tolist())) == int(nans.sum()) and not nans.all()
    n = ref["n_matches"]
    assert np.isnan(ref["matches"]["obs1"][:n]).any() and np.isnan(ref["matches"]["obs1"][n:]).all()


def test_full_case_is_what_the_gpu_test_asks_for():
    views, queries = R.full_case()
    ref = R.full_ref()
    ids = views[0]["track"]
    assert len(ids) == R.MAX_SLOTS == 16384 and len(set(ids.tolist())) == R.MAX_SLOTS and len(views[1]["track"]) == 1
    assert np.iinfo(np.int32).min in ids and 0 in ids and -1 in ids and (ids < 0).sum() > 4000
    assert [q[0] for q in queries] == [T, T, T, L, L, L]
    free = np.flatnonzero(views[0]["taken"] == 0)
    counts = np.diff(ref["pair_ptr"]).tolist()
    assert counts == [len(free), 1, 1, 0, 0, 0] and len(ref["match_slot1"]) == 2 * R.MAX_SLOTS + 1
    assert np.array_equal(ref["match_slot1"][:len(free)], free) and np.array_equal(ref["match_slot2"][:len(free)], free)
    assert ref["match_slot1"][len(free):len(free) + 2].tolist() == [11000, 0] and ref["match_slot2"][len(free):len(free) + 2].tolist() == [0, 11000]
    assert ref["n_found"].tolist() == [0, 0, 0, len(queries[3][2]) - 2, 1, R.MAX_SLOTS]
    a = ref["query_ptr"][5]
    assert np.array_equal(ref["item_slot"][a:], np.arange(R.MAX_SLOTS))                  # LOOKUP does not look at taken


def test_many_case_is_what_the_gpu_test_asks_for():
    """what takes k_tm_pack's sums over the query counts (stride 256) through all their passes and over every wavefront"""
    views, queries = R.many_case()
    ref = R.many_ref()
    assert len(queries) == R.MANY_QUERIES == 4096 and len(views) == 64
    sizes = [len(v["track"]) for v in views]
    assert min(sizes) == 0 and max(sizes) == 300 and len(set(sizes)) > 40
    counts = np.diff(ref["pair_ptr"])
    modes = np.array([q[0] for q in queries])
    # non-zero counts in the first pass of the stride, in the second and in the last
    assert (counts[:256] > 0).any() and (counts[256:512] > 0).any() and (counts[3841:] > 0).any()
    # ... and in every wavefront of every pass but few (a wrong wave term moves pair_ptr)
    assert ((counts.reshape(16, 4, 64) > 0).sum(axis=2) > 0).all()
    # both modes interleaved: neither runs for more than a few queries; LOOKUP queries count 0 between queries that match
    assert (modes == T).sum() > 1500 and (modes == L).sum() > 1500
    runs = np.diff(np.flatnonzero(np.diff(modes) != 0))
    assert runs.max() <= 12
    assert (counts[modes == L] == 0).all()
    between = [q for q in range(1, 4095) if modes[q] == L and counts[q - 1] > 0 and counts[q + 1] > 0]
    assert len(between) > 100
    # TRIANGULATION queries without a match and with several hundred
    assert (counts[modes == T] == 0).sum() > 10 and counts.max() >= 200
    for q in R.MANY_ALONE:
        assert modes[q] == T and counts[q] >= 200, q
    assert R.MANY_ALONE == (0, 255, 256, 257, 4095)
    # LOOKUP queries with and without items, items found and absent
    n_items = np.diff(ref["query_ptr"])
    assert (n_items[modes == L] == 0).any() and (n_items > 0).any() and 0 < ref["n_found"].sum() < n_items.sum()
    # the padding tail is not empty
    cap = len(ref["match_slot1"])
    assert cap == sum(sizes[q[1]] for q in queries if q[0] == T) and 0 < ref["n_matches"] < cap
    assert (ref["match_slot1"][ref["n_matches"]:] == -1).all()


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_track_match")
    assert "movba_track_match" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_track_desc", built_lib.TrackDesc), ("movba_track_result", built_lib.TrackResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d %d %d\\n", MOVBA_MAX_TRACK_SLOTS, MOVBA_MAX_TRACK_QUERIES, MOVBA_TM_TRIANGULATION, MOVBA_TM_LOOKUP);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.TrackDesc, built_lib.TrackResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.TrackDesc) == 88 and C.sizeof(built_lib.TrackResult) == 96
    assert rows[2] == [16384, 4096, 0, 1] == [built_lib.MAX_TRACK_SLOTS, built_lib.MAX_TRACK_QUERIES, built_lib.TM_TRIANGULATION, built_lib.TM_LOOKUP]


def _small_case():
    rng = np.random.default_rng(4)
    views = []
    for n in (5, 0, 8, 3):
        views.append(dict(track=rng.integers(-3, 4, n).astype(np.int32), taken=(rng.random(n) < 0.3).astype(np.uint8), obs=rng.random((n, 2)),
                          ur=rng.random(n), depth=rng.random(n)))
    queries = [(T, 0, 2), (T, 2, 2), (L, 2, [1, -3, 9]), (T, 1, 3), (L, 0, [0]), (T, 3, 0)]
    return views, queries


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L_ = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)
    payload = [key for key, _, _ in R.PAYLOAD]

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.track_desc(*_small_case())
        r, out = built_lib.track_result(d.n_queries, len(keep["item_track"]), keep["match_cap"], payload,
                                        alloc=lambda shape, dtype: np.full(shape, -7, dtype))
        r.status = 99; r.n_matches = 4242
        if mutate:
            mutate(d, keep, r)
        rc = L_.movba_track_match(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = r.n_matches == 4242 and all((a == -7).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    def count(field, value):
        return lambda d, keep, r: setattr(d, field, value)

    def huge(key, value=(1 << 28) + 1):         # n_slots / n_items above 2^28: the prefix says so, nothing behind it is read
        return lambda d, keep, r: keep[key].__setitem__(slice(1, None), value)

    refusals = {
        "negative n_views": count("n_views", -1), "negative n_queries": count("n_queries", -1), "n_queries above the bound": count("n_queries", 4097),
        "a view above the slot bound": huge("view_ptr", 16385), "n_slots above 2^28": huge("view_ptr"), "n_items above 2^28": huge("query_ptr"),
        "view_ptr not starting at 0": put("view_ptr", 0, 1), "view_ptr descending": put("view_ptr", 2, 4),
        "query_ptr not starting at 0": put("query_ptr", 0, 1), "query_ptr descending": put("query_ptr", 4, 2),
        "unknown mode": put("query_mode", 1, 2), "negative mode": put("query_mode", 0, -1),
        "view 2 too large": put("query_view", (0, 1), 4), "view 2 negative": put("query_view", (1, 1), -1),
        "view 1 too large": put("query_view", (0, 0), 4), "view 1 of a TRIANGULATION query -1": put("query_view", (3, 0), -1),
        "a LOOKUP query whose first view is not -1": put("query_view", (2, 0), 0), "a LOOKUP query's view out of range": put("query_view", (4, 1), 4),
        "a TRIANGULATION query with items": lambda d, keep, r: (keep["query_mode"].__setitem__(2, 0), keep["query_view"].__setitem__((2, 0), 0)),
        "fewer views than the queries name": count("n_views", 3),
        "obs1 without slot_obs": null("slot_obs"), "ur without slot_ur": null("slot_ur"), "depth without slot_depth": null("slot_depth"),
    }
    for field in ("view_ptr", "slot_track", "query_mode", "query_view", "query_ptr", "item_track"):
        refusals["NULL " + field] = null(field)
    for field in R.INT_KEYS:
        refusals["NULL result " + field] = null(field, res=True)
    for label, mutate in refusals.items():
        rc, status, clean = call(mutate)
        assert rc == built_lib.ERR_ARG and status == built_lib.ERR_ARG and clean, label
    # (match_cap above 2^28 is on the header's list and in the library's check, but no call reaches it: MOVBA_MAX_TRACK_QUERIES
    # queries whose view 1 has MOVBA_MAX_TRACK_SLOTS slots make 2^26)
    assert built_lib.MAX_TRACK_QUERIES * built_lib.MAX_TRACK_SLOTS < 1 << 28
    # NULL handle, descriptor, result: not even the status
    rc, status, clean = call(handle=None)
    assert rc == built_lib.ERR_ARG and status == 99 and clean
    rc, status, clean = call(desc=False)
    assert rc == built_lib.ERR_ARG and status == 99 and clean
    assert call(result=False)[0] == built_lib.ERR_ARG
    # no queries: MOVBA_OK, the status and nothing else - but the counts are still looked at
    rc, status, clean = call(count("n_queries", 0))
    assert rc == 0 and status == 0 and clean
    rc, status, clean = call(lambda d, keep, r: (setattr(d, "n_queries", 0), setattr(d, "n_views", -1)))
    assert rc == built_lib.ERR_ARG and status == built_lib.ERR_ARG and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tm_main():
    subprocess.check_call(["make", "-C", TM_DIR, "-s", "tm_main_asan"])
    return os.path.join(TM_DIR, "tm_main_asan")


def run_tm_main(exe, views, queries, tmp_path):
    """tests/track_match/tm_main.cpp on one call -> the fields of Solver.track_match's dict"""
    from movba import capi
    d, keep = capi.track_desc(views, queries)
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    have = [int(k in keep) for k in ("slot_taken", "slot_obs", "slot_ur", "slot_depth")]
    with open(src, "wb") as f:
        f.write(np.array([d.n_views, d.n_queries, len(keep["slot_track"]), len(keep["item_track"])] + have, np.int32).tobytes())
        for key in ("view_ptr", "slot_track", "query_mode", "query_view", "query_ptr", "item_track", "slot_taken", "slot_obs", "slot_ur", "slot_depth"):
            if key in keep:
                f.write(keep[key].tobytes())
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tm_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    cap = int(np.frombuffer(blob, np.int32, 1)[0])
    assert cap == keep["match_cap"]
    nq, ni, at = d.n_queries, len(keep["item_track"]), 4

    def take(count, dtype):
        nonlocal at
        a = np.frombuffer(blob, dtype, count, at)
        at += a.nbytes
        return a

    out = dict(pair_ptr=take(nq + 1, np.int32), match_slot1=take(cap, np.int32), match_slot2=take(cap, np.int32), item_slot=take(ni, np.int32),
               n_found=take(nq, np.int32), matches={})
    for key, src_key, _ in R.PAYLOAD:
        if "slot_" + src_key in keep:
            out["matches"][key] = take(2 * cap, np.float64).reshape(cap, 2) if src_key == "obs" else take(cap, np.float64)
    assert at == len(blob)
    out["n_matches"] = int(out["pair_ptr"][-1])
    out["pairs"] = dict(pair_view=keep["query_view"], pair_ptr=out["pair_ptr"])
    out["query_ptr"] = keep["query_ptr"]
    return out


def test_the_librarys_steps_on_the_mixed_case(tm_main, tmp_path):
    R.compare(run_tm_main(tm_main, *R.mixed_case(), tmp_path), R.mixed_ref(), "mixed")
    views, queries = R.mixed_case()
    bare = R.strip(views, ("taken", "obs", "ur", "depth"))
    R.compare(run_tm_main(tm_main, bare, queries, tmp_path), R.ref_track_match(bare, queries), "mixed, no slot taken, no payload")
    for label, views, queries, _ in R.hand_cases():
        R.compare(run_tm_main(tm_main, views, queries, tmp_path), R.ref_track_match(views, queries), label)


def test_the_librarys_steps_on_the_full_case(tm_main, tmp_path):
    R.compare(run_tm_main(tm_main, *R.full_case(), tmp_path), R.full_ref(), "full")


def test_the_librarys_steps_on_the_many_case(tm_main, tmp_path):
    R.compare(run_tm_main(tm_main, *R.many_case(), tmp_path), R.many_ref(), "many")


def test_the_librarys_steps_on_the_chain_case(tm_main, tmp_path):
    _, views, queries = R.chain_case()
    R.compare(run_tm_main(tm_main, views, queries, tmp_path), R.ref_track_match(views, queries), "chain")


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["track_match_asan", "track_match_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/track_match/track_match_driver.cpp: every refusal of the header with nothing written, calls without queries, the
    optional arrays left out, pinned against ordinary result memory, calls of growing and shrinking size up to the bounds, the
    call between upload, run, download and reset of a window on the same handle, and two handles on two threads - with the
    library's host sources, the stand-in runtime and fakes of tests/hipstub and the fake launch of tests/track_match linked into
    one program."""
    subprocess.check_call(["make", "-C", TM_DIR, "-s", target])
    r = subprocess.run([os.path.join(TM_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "track_match driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
