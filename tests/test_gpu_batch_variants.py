"""Batched runs in which the BATCH, not the window, picks the kernel.

movba_lba_run_batch folds ldsp / overflow / padded / stereo over the windows of a call and launches k_point_b, k_schur_b and
k_pcg_rows_b with that fold as template arguments (api.cpp), so one window beyond the point kernels' LDS image (BIG), one whose
gather lists spill (SPILL) or one with a long block row (WIDE) moves every other window of the batch onto an instantiation it
never runs solo.  The promise of include/movba.h stands all the same: every window takes exactly the steps, and produces
exactly the bits, of its solo movba_lba_run.  Every case here runs solo -> upload -> batch -> download, compares bit patterns
(a zero's sign included), asserts WHICH variant the batch launched (the test build's record, hook "batch_variant") and holds one
bystander to the oracle.  The windows and the conditions that send each one where it goes: tests/test_batch_variants_cpu.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_batch_variants_cpu as cases
from test_gpu_parity import _shared_stream_solvers, check_against

pytestmark = pytest.mark.gpu

ARRAYS = ("poses", "points", "chi2", "outlier")
TRACES = ("pcg", "accept")
SCALARS = ("n_solves", "lam", "cost", "n_band", "n_direct")


def _bits(x):
    a = np.asarray(x)
    return a.dtype.str, a.shape, a.tobytes()


def assert_same_bits(a, b, what):
    """the solo run's result and another run's: bit patterns, not values (-0.0 is not 0.0 here)"""
    assert a["status"] == b["status"] == 0, what
    for k in ARRAYS:
        assert _bits(a[k]) == _bits(b[k]), (what, k, int((a[k] != b[k]).sum()))
    for k in TRACES:
        assert _bits(a["trace"][k]) == _bits(b["trace"][k]), (what, "trace", k, a["trace"][k], b["trace"][k])
    for k in SCALARS:
        assert _bits(a[k]) == _bits(b[k]), (what, k, a[k], b[k])


def handle_options(name, default_solver=False):
    """SPILL keeps its spilling PCG; the bystanders run the PCG (solver = 3) except the one left to the default choice, which
    gives it to k_band; BIG and WIDE take the default choice."""
    if name == "SPILL":
        return dict(pcg_spill=True)
    if default_solver or name.startswith(("band", "BIG", "WIDE")):
        return {}
    return dict(solver=3)


class Batch:
    """The handles of one batch on one stream, all from one library image (hooks: the test build), one window each."""

    def __init__(self, lib, names, hooks=True, default_solver=False, leaves=()):
        """leaves: windows whose handles take the default options and which the direct solver therefore takes out of the batch"""
        self.lib, self.names, self.hooks, self.leaves = lib, list(names), hooks, tuple(leaves)
        opts = lambda n: {} if n in self.leaves else handle_options(n, default_solver)       # noqa: E731
        self.windows = [cases.window(n) for n in self.names]
        self.iters = [cases.MAX_ITERS.get(n) for n in self.names]
        self.st, self.solvers = _shared_stream_solvers(lib, 1, hooks=hooks, **opts(self.names[0]))
        try:
            for n in self.names[1:]:
                self.solvers.append(lib.Solver(device=0, stream=self.st.cuda_stream, hooks=hooks, **opts(n)))
        except Exception:
            self.close()
            raise
        self.solo_results = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        for s in self.solvers:
            s.close()

    def solo(self):
        self.solo_results = [s.solve(w, max_iters=it) for s, w, it in zip(self.solvers, self.windows, self.iters)]
        for n, r in zip(self.names, self.solo_results):
            assert r["status"] == 0 and r["n_sync_timeouts"] == 0, n
            # every window stays in the batched kernels to the end: none parks itself for the direct solver
            if n in self.leaves:
                assert r["n_direct"] == r["n_solves"] and r["pcg_iters"] == 0, n
            else:
                assert r["n_direct"] == 0 and r["n_pcg_giveups"] == 0, (n, r["n_direct"], r["n_pcg_giveups"])
        return self.solo_results

    def upload(self):
        for s, w, it in zip(self.solvers, self.windows, self.iters):
            s.upload(w, max_iters=it)

    def run(self, expect, names=None):
        """run_batch over `names` (default: all, in the order given), download, solo bits, the recorded variant -> results"""
        idx = list(range(len(self.names))) if names is None else [self.names.index(n) for n in names]
        assert self.lib.run_batch([self.solvers[i] for i in idx]) == 0
        out = []
        for i in idx:
            r = self.solvers[i].download()
            assert_same_bits(self.solo_results[i], r, self.names[i])
            if self.hooks:
                where = dict(batched=0, solo=1) if self.names[i] in self.leaves else dict(batched=1, solo=0)
                assert self.solvers[i].batch_variant() == dict(expect, **where), (self.names[i], self.solvers[i].batch_variant())
            out.append(r)
        return out

    def result_of(self, results, name):
        return results[self.names.index(name)]


@functools.lru_cache(maxsize=None)
def _oracle(oracle_mod, name):
    return oracle_mod.solve(cases.window(name))


def variant(ldsp, overflow, padded, stereo=0, groups=2):
    return dict(ldsp=ldsp, overflow=overflow, padded=padded, stereo=stereo, groups=groups)


# case -> (windows in batch order, the variant every launch of the batch takes, the bystander held to the oracle)
CASES = {
    "a": (cases.MONO, variant(1, 0, 1), "cfg2"),
    "a-stereo": (cases.STEREO, variant(1, 0, 1, stereo=1), "nf17-st"),
    "b-first": (["BIG"] + cases.MONO, variant(0, 0, 1), "nf9"),
    "b-last": (cases.MONO + ["BIG"], variant(0, 0, 1), "nf17"),
    "b-stereo": (cases.STEREO[:4] + ["BIG-st"] + cases.STEREO[4:], variant(0, 0, 1, stereo=1), "cfg2-st"),
    "c": (cases.MONO[:3] + ["SPILL"] + cases.MONO[3:], variant(1, 1, 0), "nf40"),
    "d": (cases.MONO[:5] + ["WIDE"] + cases.MONO[5:], variant(1, 0, 0), "small"),
    "e": (["BIG"] + cases.MONO + ["SPILL"], variant(0, 1, 0), "nf5"),
}
_RESULTS = {}


def run_case(lib, oracle_mod, case, hooks=True):
    """solo, upload, batch, download, solo bits, variant, one bystander against the oracle; the batch's results, kept per
    (case, library) so that the comparison of the two libraries runs nothing twice"""
    if (case, hooks) in _RESULTS:
        return _RESULTS[case, hooks]
    names, expect, bystander = CASES[case]
    with Batch(lib, names, hooks=hooks) as b:
        solo = b.solo()
        for n, r in zip(names, solo):
            assert (r["n_band"] > 0) == n.startswith("band") or n.startswith(("BIG", "WIDE")), (n, r["n_band"])
            if n == "SPILL":
                assert r["pcg_iters"] > 0 and r["n_band"] == 0
        b.upload()
        res = b.run(expect)
        check_against(b.result_of(res, bystander), _oracle(oracle_mod, bystander), cases.window(bystander))
    _RESULTS[case, hooks] = res
    return res


@pytest.mark.parametrize("case", ["a", "a-stereo"])
def test_a_batch_of_bystanders_runs_the_padded_lds_variant(built_lib, oracle_mod, case):
    """The baseline, and the proof that the record works: <ldsp=1, overflow=0, padded=1>, two groups."""
    run_case(built_lib, oracle_mod, case)


@pytest.mark.parametrize("case", ["b-first", "b-last", "b-stereo"])
def test_b_one_window_beyond_the_lds_image_takes_every_window_through_l2(built_lib, oracle_mod, case):
    """BIG forces LDSP=false on k_point_b, forward and back-substitution, for the windows of BOTH groups, whichever group it
    sits in; monocular and stereo."""
    run_case(built_lib, oracle_mod, case)


def test_c_one_spilling_window_takes_every_pcg_window_through_the_overflow_kernel(built_lib, oracle_mod):
    """SPILL on a pcg_spill handle: k_pcg_rows_b<OVERFLOW=true, PADDED=false> for all; the bystanders' tail loop runs over
    nothing and every off-diagonal block of theirs is summed from the partials instead of read from the image."""
    run_case(built_lib, oracle_mod, "c")


def test_d_one_long_block_row_takes_every_padded_window_onto_the_packed_pair_sums(built_lib, oracle_mod):
    """WIDE: k_pcg_rows_b<false, false>.  The bystanders' bits are also those of a solo run forced onto the packed layout."""
    names = CASES["d"][0]
    res = run_case(built_lib, oracle_mod, "d")
    packed = built_lib.Solver(solver=3, hooks=True)
    try:
        packed.hook("pcg_packed", 1)
        for n, r in zip(names, res):
            if n.startswith(("band", "WIDE")):
                continue
            assert_same_bits(packed.solve(cases.window(n)), r, n + " solo, packed")
    finally:
        packed.close()


def test_e_lds_limit_and_overflow_forced_together(built_lib, oracle_mod):
    run_case(built_lib, oracle_mod, "e")


def test_f_the_variant_changes_between_batches_on_the_same_handles(built_lib):
    """b, then the bystanders alone without a new upload (LDS image again), then b again (through L2 again): the copies of
    the windows a batch overwrites (lds_poses) leave nothing behind on the handles."""
    names = CASES["b-first"][0]
    with Batch(built_lib, names) as b:
        b.solo()
        b.upload()
        b.run(variant(0, 0, 1))
        b.run(variant(1, 0, 1), names=cases.MONO)
        b.run(variant(0, 0, 1))
        b.run(variant(1, 0, 1), names=cases.MONO[::-1])


@pytest.mark.parametrize("names,default_solver,groups,band", [
    (["nf40"], False, 1, 0),                                   # one window of the PCG: no k_band_b launch, one group
    (["band"], False, 1, 1),                                   # one banded window: no k_pcg_rows_b launch
    (["cfg2", "band"], False, 2, None),                        # two: one window per group, each group one solver only
    (["small", "nf5", "cfg2", "band"], True, 2, 1),            # banded windows only
    ([n for n in cases.MONO if n != "band"], False, 2, 0),     # PCG windows only
], ids=["one-pcg", "one-banded", "two", "banded-only", "pcg-only"])
def test_g_batch_sizes_and_suppressed_launches(built_lib, names, default_solver, groups, band):
    with Batch(built_lib, names, default_solver=default_solver) as b:
        solo = b.solo()
        if band is not None:
            assert all((r["n_band"] > 0) == bool(band) for r in solo), [r["n_band"] for r in solo]
        b.upload()
        b.run(variant(1, 0, 1, groups=groups))


def test_g_a_window_that_leaves_the_batch_does_not_enter_the_fold(built_lib):
    """SPILL on a handle WITHOUT pcg_spill: the direct solver takes it from the first trial, behind the batched launches
    (recorded: not batched, ran on its own), and its overflow does not move the others off the padded kernel."""
    with Batch(built_lib, cases.MONO[:4] + ["SPILL"] + cases.MONO[4:6], leaves=("SPILL",)) as b:
        b.solo()
        b.upload()
        b.run(variant(1, 0, 1))


def test_h_a_batch_of_monocular_and_stereo_windows_is_refused_and_harms_nothing(built_lib):
    names = ["cfg2", "nf9", "small-st", "nf17", "band"]
    mono = [n for n in names if not n.endswith("-st")]
    with Batch(built_lib, names) as b:
        solo = b.solo()
        b.upload()
        with pytest.raises(built_lib.MovbaError, match="invalid argument"):
            built_lib.run_batch(b.solvers)
        for n, s, a in zip(names, b.solvers, solo):                 # the uploads are still good: each runs on its own
            assert s.run() == 0
            assert_same_bits(a, s.download(), n + " run() after the refusal")
        b.run(variant(1, 0, 1), names=mono)
        # (and the other way round: the stereo window first decides what the batch holds)
        with pytest.raises(built_lib.MovbaError, match="invalid argument"):
            built_lib.run_batch(b.solvers[2:] + b.solvers[:2])
        b.run(variant(1, 0, 1, stereo=1, groups=1), names=["small-st"])


CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "batch_groups_child.py")


def test_i_group_counts_other_than_the_default(built_lib):
    """MOVBA_BATCH_GROUPS is read once per process: 1 (one stream), 3 and 4 (streams of their own, the phase-event ring) each
    in a fresh child, one after the other; the child holds the eight windows of case a to their solo bits and asserts the
    recorded number of groups.  A child that fails or runs out of time fails the test and no further one is started."""
    assert os.path.exists(built_lib.HOOKS_LIB_PATH)
    for groups in (1, 3, 4):
        env = dict(os.environ, MOVBA_BATCH_GROUPS=str(groups))
        flags = ["-s"] if sys.flags.no_user_site else []
        p = subprocess.run([sys.executable] + flags + [CHILD, str(groups)], env=env, timeout=120, capture_output=True, text=True)
        assert p.returncode == 0, (groups, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        assert f"groups {groups}: 8 windows equal their solo bits" in p.stdout, p.stdout[-2000:]


@pytest.mark.parametrize("case", ["a", "b-first", "c"])
def test_the_product_library_computes_what_the_test_build_computes(built_lib, oracle_mod, case):
    """The record lives in the test build only; the library that ships must take the same path: same bits, window by window."""
    names = CASES[case][0]
    ref = run_case(built_lib, oracle_mod, case, hooks=True)
    res = run_case(built_lib, oracle_mod, case, hooks=False)
    for n, a, b in zip(names, ref, res):
        assert_same_bits(a, b, n + ": product library against test build")
