"""movba_track_match on the device against the restatement of tests/track_match_ref.py, every comparison exact integer equality or
equality of the payload's 64-bit words: the mixed call entry by entry with its -1 / NaN tails, the call at MOVBA_MAX_TRACK_SLOTS,
the call at MOVBA_MAX_TRACK_QUERIES (the pack's sums over the query counts, which only the device runs, over every pass),
the gather with and without its sources, the chain into movba_triangulate, independence of a query from everything but its own
views and items (reordered, split over calls), pinned results, a solved window on the same handle left as it was, a refusal on
a live handle and a call without queries."""
import ctypes as C

import numpy as np
import pytest

import track_match_ref as R
import view_points_ref as V
from movba import capi, synth

pytestmark = pytest.mark.gpu
T, L = R.TM_TRIANGULATION, R.TM_LOOKUP


def test_parity_with_the_restatement_on_a_mixed_call(solver):
    """40 queries of both modes over views of 0, 1, 63, 64, 65, 255, 256, 257 and 1 000 slots, a quarter of the slots repeating an
    id, half of them taken, a view with every slot taken, a view with one id, a view against itself, absent items, a LOOKUP
    without items: every array equals the literal restatement's."""
    got = solver.track_match(*R.mixed_case())
    assert got["status"] == 0
    R.compare(got, R.mixed_ref(), "mixed")
    R.compare(solver.track_match(*R.mixed_case()), got, "the same call twice")


def test_one_view_at_the_slot_bound(solver):
    """16 384 slots with all-distinct ids (INT32_MIN, 0, -1 and negatives among them) against itself and against a 1-slot view, in
    both modes: the full table, 64 chunks of the scan, the largest LDS request.  The dict-based restatement is the reference."""
    got = solver.track_match(*R.full_case())
    R.compare(got, R.full_ref(), "full")
    assert got["n_found"].tolist()[3:] == [len(R.full_case()[1][3][2]) - 2, 1, R.MAX_SLOTS]


def test_4096_queries_take_the_sums_of_the_pack_over_every_pass(solver):
    """MOVBA_MAX_TRACK_QUERIES queries of both modes over 64 views of 0 to 300 slots: k_tm_pack's sums over the counts of all
    queries take 16 passes of their stride and all four wavefronts, which only the device runs (the host build keeps a running
    count).  pair_ptr in full, every array with its tails, and queries 0, 255, 256, 257 and 4 095 alone against their rows."""
    views, queries = R.many_case()
    ref = R.many_ref()
    got = solver.track_match(views, queries)
    assert got["status"] == 0 and len(got["pair_ptr"]) == R.MANY_QUERIES + 1
    assert np.array_equal(got["pair_ptr"], ref["pair_ptr"]), np.flatnonzero(got["pair_ptr"] != ref["pair_ptr"])[:8].tolist()
    R.compare(got, ref, "many")
    n = got["n_matches"]
    assert 0 < n < len(got["match_slot1"]) and (got["match_slot1"][n:] == -1).all() and np.isnan(got["matches"]["ur2"][n:]).all()
    want = R.rows(got, R.MANY_ALONE)
    for q, row in zip(R.MANY_ALONE, want):
        assert len(row[0]) >= 200, q
        assert R.rows(solver.track_match(views, [queries[q]]), [0]) == [row], q
        assert R.rows(R.ref_track_match(views, [queries[q]]), [0]) == [row], q          # (the literal double loop)


def test_gather_copies_bits_and_pads_the_tails(solver):
    views, queries = R.mixed_case()
    ref = R.mixed_ref()
    got = solver.track_match(views, queries)
    n = got["n_matches"]
    assert 0 < n < len(got["match_slot1"]) and sorted(got["matches"]) == sorted(k for k, _, _ in R.PAYLOAD)
    for key, src, side in R.PAYLOAD:
        g = got["matches"][key]
        assert np.array_equal(R.bits(g[:n]), R.bits(ref["matches"][key][:n])), key          # compared as uint64
        assert np.isnan(g[n:]).all(), key
        assert np.isnan(g[:n]).any() and not np.isnan(g[:n]).all(), key                     # NaNs with payload bits came through
    assert (got["match_slot1"][n:] == -1).all() and (got["match_slot2"][n:] == -1).all()
    # a NULL source with a NULL output is accepted: the join alone, then one payload array of three
    bare = R.strip(views, ("obs", "ur", "depth"))
    alone = solver.track_match(bare, queries)
    assert alone["matches"] == {}
    R.compare(alone, R.ref_track_match(bare, queries), "no payload")
    only_ur = R.strip(views, ("obs", "depth"))
    R.compare(solver.track_match(only_ur, queries), R.ref_track_match(only_ur, queries), "ur alone")
    # an output left out beside its source: the others arrive as before
    d, keep = capi.track_desc(views, queries)
    r, out = capi.track_result(d.n_queries, len(keep["item_track"]), keep["match_cap"], ("obs2", "depth1"))
    assert solver._L.movba_track_match(solver._h, C.byref(d), C.byref(r)) == 0 and r.n_matches == n
    assert np.array_equal(R.bits(out["obs2"][:n]), R.bits(ref["matches"]["obs2"][:n])) and np.array_equal(R.bits(out["depth1"][:n]), R.bits(ref["matches"]["depth1"][:n]))
    assert np.array_equal(out["match_slot1"], ref["match_slot1"]) and np.isnan(out["obs2"][n:]).all()


def test_chain_into_triangulate(solver):
    """3 pairs of about 200 slots: track_match's pairs / matches handed to Solver.triangulate unchanged give the bits of a
    triangulate call fed the host-joined matches."""
    sc, views, queries = R.chain_case()
    ref = R.ref_track_match(views, queries)
    n = ref["n_matches"]
    assert n > 400 and np.diff(ref["pair_ptr"]).min() > 100
    got = solver.track_match(views, queries)
    R.compare(got, ref, "chain")
    chained = solver.triangulate(sc["views"], got["pairs"], got["matches"], sc["reproj_gate"], sc["far_threshold"])
    host = solver.triangulate(sc["views"], ref["pairs"], {k: np.ascontiguousarray(v[:n]) for k, v in ref["matches"].items()},
                              sc["reproj_gate"], sc["far_threshold"])
    assert chained["status"] == host["status"] == 0 and chained["n_accepted"] == host["n_accepted"] > 100
    assert chained["points"].shape == (n, 3) and np.array_equal(chained["code"], host["code"])
    assert np.array_equal(chained["points"].view(np.uint64), host["points"].view(np.uint64))
    assert len(set(chained["code"].tolist())) > 2                                          # accepted and rejected matches among them


def test_a_query_depends_on_its_own_data_alone(built_lib):
    views, queries = R.mixed_case()
    nq = len(queries)
    s = built_lib.Solver()
    try:
        whole = s.track_match(views, queries)
        R.compare(whole, R.mixed_ref(), "whole")
        want = R.rows(whole, range(nq))
        order = list(range(nq - 1, -1, -1))
        rev = s.track_match(views, [queries[q] for q in order])
        assert R.rows(rev, range(nq)) == [want[q] for q in order]
        rng = np.random.default_rng(5)
        order = rng.permutation(nq).tolist()
        assert R.rows(s.track_match(views, [queries[q] for q in order]), range(nq)) == [want[q] for q in order]
        a, b = s.track_match(views, queries[:17]), s.track_match(views, queries[17:])
        assert R.rows(a, range(17)) + R.rows(b, range(nq - 17)) == want
        # the views a query does not name do not matter either: query 3 with its two views alone
        q = queries[3]
        assert q[0] == T
        assert R.rows(s.track_match([views[q[1]], views[q[2]]], [(T, 0, 1)]), [0]) == [want[3]]
    finally:
        s.close()


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        for views, queries in (R.mixed_case(), R.full_case(), R.chain_case()[1:]):
            R.compare(s.track_match(views, queries, pinned=True), s.track_match(views, queries), "pinned")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """The sequence of test_gpu_covisibility.py's test of the same name with movba_track_match in the places of its calls:
    download, marginals, reset + run and a fresh upload + run give the bits they give without the calls, and the call gives on
    the handle of a solved window what it gives on a fresh one."""
    w = synth.cfg("small")
    case, ref = R.mixed_case(), R.mixed_ref()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")

    def sequence(with_calls):
        s = built_lib.Solver()
        try:
            out = []
            out.append(s.solve(w))
            before = s.marginals()
            if with_calls:
                R.compare(s.track_match(*case), ref, "after the solve")
            out.append(s.download())
            after = s.marginals()
            assert after["status"] == before["status"]
            assert V.same_bits(after["pose_cov"], before["pose_cov"]) and V.same_bits(after["point_cov"], before["point_cov"])
            if with_calls:
                R.compare(s.track_match(*case, pinned=True), ref, "after the marginals, pinned")
            assert s._L.movba_lba_reset(s._h) == 0
            if with_calls:
                R.compare(s.track_match(*R.full_case()), R.full_ref(), "after the reset")
            s.run()
            out.append(s.download())
            s.upload(w)
            if with_calls:
                R.compare(s.track_match(*case), ref, "between upload and run")
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


def test_a_refusal_and_a_call_without_queries_on_a_live_handle(solver):
    views, queries = R.mixed_case()
    payload = [key for key, _, _ in R.PAYLOAD]
    d, keep = capi.track_desc(views, queries)
    keep["query_view"][7, 1] = len(views)                       # one view index out of range
    r, out = capi.track_result(d.n_queries, len(keep["item_track"]), keep["match_cap"], payload, alloc=lambda shape, dtype: np.full(shape, -7, dtype))
    r.status = 99; r.n_matches = 4242
    assert solver._L.movba_track_match(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and r.n_matches == 4242 and all((a == -7).all() for a in out.values())
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.track_match(views, list(queries) + [(L, len(views), [1])])
    # no queries: MOVBA_OK, and not one result entry is written
    d, keep = capi.track_desc(views, [])
    r, out = capi.track_result(3, 4, 5, payload, alloc=lambda shape, dtype: np.full(shape, -7, dtype))
    r.status = 99; r.n_matches = 4242
    assert solver._L.movba_track_match(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0 and r.n_matches == 4242
    assert all((a == -7).all() for a in out.values())
    empty = solver.track_match(views, [])
    assert empty["status"] == 0 and len(empty["match_slot1"]) == 0
    R.compare(solver.track_match(views, queries), R.mixed_ref(), "after the refusal")
