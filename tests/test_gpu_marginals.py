"""movba_lba_marginals on the device: every block against the numpy reference of test_marginals_cpu.py at the downloaded
estimate (relative Frobenius error <= 1e-7 per block), the blocks' properties, and a window, its results and later runs left
exactly as they were."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from movba import synth
from test_marginals_cpu import marginals_schur, rel_block_err

pytestmark = pytest.mark.gpu

TOL = 1e-7


def _check(w, r, mc, damping, label):
    assert mc["status"] == 0, label
    ref = marginals_schur(w, r["poses"], r["points"], damping)
    ep = rel_block_err(mc["pose_cov"], ref["pose_cov"])
    epts = rel_block_err(mc["point_cov"], ref["point_cov"])
    print(f"{label}: damping {damping:g}, cond(S) {ref['cond_S']:.3g}, pose err {ep:.2e}, point err {epts:.2e}")
    assert ep <= TOL and epts <= TOL, label
    pc, qc = mc["pose_cov"], mc["point_cov"]
    fixed = np.asarray(w.pose_fixed) != 0
    assert np.all(pc[fixed] == 0.0)
    assert np.array_equal(np.isnan(pc), np.isnan(ref["pose_cov"])) and np.array_equal(np.isnan(qc), np.isnan(ref["point_cov"]))
    assert np.array_equal(pc, np.swapaxes(pc, 1, 2), equal_nan=True)          # exactly symmetric
    assert np.array_equal(qc, np.swapaxes(qc, 1, 2), equal_nan=True)
    for blk in pc[~fixed]:
        np.linalg.cholesky(blk)
    for blk in qc[np.isfinite(qc).all((1, 2))]:
        np.linalg.cholesky(blk)
    return ref


GOLDEN_CASES = [("small", 0.0), ("hard", 0.0), ("stereo", 0.0), ("cameras", 0.0), ("tiny", 1e-3), ("norobust", 1e-3),
                ("small", 1e-2), ("stereo", 0.5)]


@pytest.mark.parametrize("name,damping", GOLDEN_CASES)
def test_golden_windows_match_the_reference(solver, name, damping):
    w, _ = load_golden("lba_" + name)
    r = solver.solve(w)
    assert r["status"] == 0
    mc = solver.marginals(damping)
    _check(w, r, mc, damping, name)
    again = solver.marginals(damping)                                           # two calls: the same bits
    assert np.array_equal(again["pose_cov"], mc["pose_cov"], equal_nan=True)
    assert np.array_equal(again["point_cov"], mc["point_cov"], equal_nan=True)
    poses_only = solver.marginals(damping, points=False)
    assert poses_only["point_cov"] is None and np.array_equal(poses_only["pose_cov"], mc["pose_cov"], equal_nan=True)


def test_cfg2(solver):
    w = synth.cfg("cfg2")
    r = solver.solve(w)
    _check(w, r, solver.marginals(0.0), 0.0, "cfg2")


def test_window_beyond_the_pcg_spans_thirteen_tile_columns(built_lib):
    """100 free keyframes: the run itself takes the dense solver, S is 600 x 600 (13 tile columns of 48)"""
    w = synth.make_window(100, 2, 3000, seed=5101, run_lo=2, run_hi=8)
    s = built_lib.Solver()
    try:
        r = s.solve(w)
        assert r["status"] == 0 and r["n_direct"] > 0
        _check(w, r, s.marginals(0.0), 0.0, "100 free keyframes")
    finally:
        s.close()


def test_covisibility_renumbering_is_undone(built_lib):
    """A window whose keyframe ids do not follow its covisibility graph is renumbered inside the library: the blocks still come
    back in caller order, equal to those of a handle that keeps the caller's numbering and to the reference."""
    w = synth.shuffle_ids(synth.cfg("cfg2"), 77)
    info = built_lib.structure_probe(w)
    assert info["reordered"] and not np.array_equal(info["free_index"][info["free_index"] >= 0],
                                                    np.arange((info["free_index"] >= 0).sum()))
    a, b = built_lib.Solver(), built_lib.Solver(reorder=False)
    try:
        ra, rb = a.solve(w), b.solve(w)
        ma, mb = a.marginals(0.0), b.marginals(0.0)
        _check(w, ra, ma, 0.0, "renumbered")
        _check(w, rb, mb, 0.0, "caller order")
        assert rel_block_err(ma["pose_cov"], mb["pose_cov"]) <= TOL and rel_block_err(ma["point_cov"], mb["point_cov"]) <= TOL
        # blocks left in the library's own numbering (caller pose i given the block of free index rank(i)) would fail the bound
        fidx = info["free_index"]
        free = np.flatnonzero(fidx >= 0)
        unmapped = ma["pose_cov"].copy()
        for rank, i in enumerate(free):
            unmapped[i] = ma["pose_cov"][free[np.flatnonzero(fidx[free] == rank)[0]]]
        ref = marginals_schur(w, ra["poses"], ra["points"], 0.0)
        assert rel_block_err(unmapped, ref["pose_cov"]) > 1e-3
    finally:
        a.close(); b.close()


def _raw(s, damping, NP, P, fill=7.25):
    pc = np.full((NP, 6, 6), fill); qc = np.full((P, 3, 3), fill)
    rc = s._L.movba_lba_marginals(s._h, damping, pc.ctypes.data_as(C.POINTER(C.c_double)), qc.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, pc, qc


def test_results_and_later_runs_are_left_alone(built_lib):
    w = synth.cfg("cfg2")
    a, b = built_lib.Solver(), built_lib.Solver()
    try:
        ref = b.solve(w)
        a.upload(w); assert a.run() == 0
        a.marginals(0.0)
        got = a.download()                                  # marginals between run and download
        for k in ("poses", "points", "chi2", "outlier"):
            assert np.array_equal(got[k], ref[k]), k
        assert got["cost"] == ref["cost"] and got["n_solves"] == ref["n_solves"]
        assert a._L.movba_lba_reset(a._h) == 0 and a.run() == 0       # reset + run after a marginals call
        again = a.download()
        for k in ("poses", "points", "chi2", "outlier"):
            assert np.array_equal(again[k], ref[k]), k
    finally:
        a.close(); b.close()


def test_batched_run_gives_each_window_its_solo_marginals(built_lib):
    import torch
    ws = [synth.cfg("cfg2"), synth.cfg("small"), synth.make_window(12, 2, 800, seed=5202, run_lo=2, run_hi=6)]
    st = torch.cuda.Stream(device=0)
    solvers = [built_lib.Solver(device=0, stream=st.cuda_stream) for _ in ws]
    solo = built_lib.Solver()
    try:
        want = []
        for w in ws:
            solo.solve(w)
            want.append(solo.marginals(0.0))
        for s, w in zip(solvers, ws):
            s.upload(w)
        assert built_lib.run_batch(solvers) == 0
        for s, m in zip(solvers, want):
            got = s.marginals(0.0)
            assert np.array_equal(got["pose_cov"], m["pose_cov"], equal_nan=True)
            assert np.array_equal(got["point_cov"], m["point_cov"], equal_nan=True)
    finally:
        for s in solvers + [solo]:
            s.close()


def test_call_order_and_arguments(built_lib):
    w = synth.cfg("small")
    NP, P = w.n_poses, w.n_points
    s = built_lib.Solver()
    try:
        assert _raw(s, 0.0, NP, P)[0] == built_lib.ERR_STATE                   # before any upload
        s.upload(w)
        assert _raw(s, 0.0, NP, P)[0] == built_lib.ERR_STATE                   # uploaded, not run
        assert s.run() == 0
        assert s._L.movba_lba_marginals(s._h, 0.0, None, None) == built_lib.ERR_ARG
        for bad in (-1e-3, float("nan"), float("inf")):
            rc, pc, qc = _raw(s, bad, NP, P)
            assert rc == built_lib.ERR_ARG and np.all(pc == 7.25) and np.all(qc == 7.25)
        assert _raw(s, 0.0, NP, P)[0] == 0
        assert s._L.movba_lba_reset(s._h) == 0
        assert _raw(s, 0.0, NP, P)[0] == built_lib.ERR_STATE                   # reset, not run again
        stop = np.ones(1, np.uint8)                                             # a run stopped by the flag
        s.upload(w, stop=stop)
        assert s.run() == built_lib.STOPPED
        rc, pc, qc = _raw(s, 0.0, NP, P)
        assert rc == built_lib.ERR_STATE and np.all(pc == 7.25) and np.all(qc == 7.25)
    finally:
        s.close()


def test_a_point_without_information_is_singular_undamped(built_lib):
    w = synth.cfg("small")
    l = int(w.edge_point[len(w.edge_point) // 2])
    isg = np.array(w.inv_sigma2, np.float64)
    isg[np.asarray(w.edge_point) == l] = 0.0
    w.inv_sigma2 = isg
    s = built_lib.Solver()
    try:
        r = s.solve(w)
        assert r["status"] == 0
        rc, pc, qc = _raw(s, 0.0, w.n_poses, w.n_points)
        assert rc == built_lib.SINGULAR and np.all(pc == 7.25) and np.all(qc == 7.25)
        assert s.marginals(0.0)["status"] == built_lib.SINGULAR
        mc = s.marginals(1e-3)
        ref = _check(w, r, mc, 1e-3, "point without information")
        np.testing.assert_allclose(mc["point_cov"][l], 1e3 * np.eye(3), rtol=1e-12)
        assert np.array_equal(ref["point_cov"][l], 1e3 * np.eye(3))
    finally:
        s.close()
