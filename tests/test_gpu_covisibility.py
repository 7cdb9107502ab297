"""movba_covisibility on the device against the restatement of tests/covisibility_ref.py, every comparison exact integer equality:
the parity call entry by entry with its -1 / 0 padding, the wide call at MOVBA_MAX_COVIS_VIEWS with the whole order and with 7
entries handed out, the tiny call and the call without queries, independence of a query from everything but its own items
(identical reversed, split over calls, alone, twice, into pinned memory), a solved window on the same handle left as it was,
and a refusal on a live handle."""
import ctypes as C

import numpy as np
import pytest

import covisibility_ref as R
import view_points_ref as V
from movba import capi, synth

pytestmark = pytest.mark.gpu


def test_parity_with_the_restatement(solver):
    """300 views, 2 000 points with lists of 0 .. 65 and 300 observers, 40 queries of 0 .. 1 500 items, self entries inside and
    outside the lists, a tenth of the views not eligible: all six arrays equal the restatement's."""
    got = solver.covisibility(**R.parity_case())
    assert got["status"] == 0
    R.compare(got, R.parity_ref(), "parity")


def test_wide_case_whole_order_and_its_front(solver):
    """8 192 views - the largest LDS, the longest list and the largest sort: 8 192 keys - handed out whole, and 7 entries of it:
    the front of the same order, n_counted unchanged."""
    whole = solver.covisibility(**R.wide_case())
    R.compare(whole, R.wide_ref(), "wide, 8192 handed out")
    front = solver.covisibility(**R.wide_case(7))
    R.compare(front, R.wide_ref(7), "wide, 7 handed out")
    assert np.array_equal(front["out_view"], whole["out_view"][:, :7]) and np.array_equal(front["out_weight"], whole["out_weight"][:, :7])
    for key in R.KEYS[:4]:
        assert np.array_equal(front[key], whole[key]), key
    assert front["n_counted"].tolist() == [8192, 8192, 8191]


def test_tiny_case_and_a_call_without_queries(solver):
    for self_view in (0, -1):
        case = dict(R.tiny_case(self_view), max_out=1)
        R.compare(solver.covisibility(**case), R.ref_covisibility(**case), f"tiny, self {self_view}")
    # no queries: MOVBA_OK, and not one result entry is written
    d, keep = capi.covis_desc(**dict(R.parity_case(), queries=[], query_self=None))
    r, out = capi.covis_result(3, 4, alloc=lambda shape, dtype: np.full(shape, -7, dtype))
    r.status = 99
    assert solver._L.movba_covisibility(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all((a == -7).all() for a in out.values())


def test_a_query_depends_on_its_own_items_alone(built_lib):
    case, ref = R.parity_case(), R.parity_ref()
    n = len(case["queries"])
    s = built_lib.Solver()
    try:
        whole = s.covisibility(**case)
        R.compare(whole, ref, "whole")
        R.compare(s.covisibility(**case), whole, "the whole call twice")
        R.compare(s.covisibility(**case, pinned=True), whole, "pinned")
        rev = s.covisibility(**R.subset(case, range(n - 1, -1, -1)))
        R.compare({key: rev[key][::-1] for key in R.KEYS}, whole, "reversed query order")
        a, b = s.covisibility(**R.subset(case, range(0, 17))), s.covisibility(**R.subset(case, range(17, n)))
        R.compare({key: np.concatenate([a[key], b[key]]) for key in R.KEYS}, whole, "split over two calls")
        for q in range(n):
            R.compare(s.covisibility(**R.subset(case, [q])), R.rows(whole, [q]), f"query {q} alone")
    finally:
        s.close()


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        for case in (R.parity_case(), dict(R.parity_case(), max_out=7), R.wide_case(7)):
            R.compare(s.covisibility(**case, pinned=True), s.covisibility(**case), "pinned")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """The sequence of test_gpu_point_normals.py's test of the same name with movba_covisibility in the places of its calls:
    download, marginals, reset + run and a fresh upload + run give the bits they give without the calls, and the call gives on
    the handle of a solved window what it gives on a fresh one."""
    w = synth.cfg("small")
    case, ref = R.parity_case(), R.parity_ref()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")

    def sequence(with_calls):
        s = built_lib.Solver()
        try:
            out = []
            out.append(s.solve(w))
            before = s.marginals()
            if with_calls:
                R.compare(s.covisibility(**case), ref, "after the solve")
            out.append(s.download())
            after = s.marginals()
            assert after["status"] == before["status"]
            assert V.same_bits(after["pose_cov"], before["pose_cov"]) and V.same_bits(after["point_cov"], before["point_cov"])
            if with_calls:
                R.compare(s.covisibility(**case, pinned=True), ref, "after the marginals, pinned")
            assert s._L.movba_lba_reset(s._h) == 0
            if with_calls:
                R.compare(s.covisibility(**R.wide_case(7)), R.wide_ref(7), "after the reset")
            s.run()
            out.append(s.download())
            s.upload(w)
            if with_calls:
                R.compare(s.covisibility(**case), ref, "between upload and run")
            s.run()
            out.append(s.download())
            return out, before
        finally:
            s.close()

    (plain, cov0), (mixed, cov1) = sequence(False), sequence(True)
    assert V.same_bits(cov0["pose_cov"], cov1["pose_cov"]) and V.same_bits(cov0["point_cov"], cov1["point_cov"])
    for a, b in zip(plain, mixed):
        for k in keys:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for k in keys:
        assert np.array_equal(np.asarray(mixed[2][k]), np.asarray(mixed[0][k])), k


def test_a_refusal_on_a_live_handle_writes_nothing_and_leaves_it_usable(solver):
    case = R.parity_case()
    d, keep = capi.covis_desc(**case)
    keep["obs_view"][1234] = case["n_views"]                    # one observer index out of range
    r, out = capi.covis_result(d.n_queries, d.max_out, alloc=lambda shape, dtype: np.full(shape, -7, dtype))
    r.status = 99; r.pad = 77
    assert solver._L.movba_covisibility(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and r.pad == 77 and all((a == -7).all() for a in out.values())
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.covisibility(**dict(case, lists=[np.array([300], np.int32)] + list(case["lists"][1:])))
    R.compare(solver.covisibility(**case), R.parity_ref(), "after the refusal")
