"""The windows of tests/test_gpu_batch_variants.py, chosen on the host.

movba_lba_run_batch folds four properties over the windows of a call (api.cpp: stereo, ldsp, overflow, padded) and every batched
launch takes its template arguments from that fold, so ONE window moves all the others onto a kernel variant none of them runs
solo.  The GPU test needs windows that flip exactly one property each (BIG, SPILL, WIDE) and bystanders that flip none; which
window does what is a property of its structure alone, so it is asserted here, without a GPU, from movba_structure_probe and
from the conditions of the sources restated in numpy.  The GPU test imports the windows from this module."""
import functools
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from movba import synth

CSRC = os.path.join(ROOT, "mov-slam_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def constants():
    """kPointLdsLimit, kPointRed and kPcgPlanOwnBatch as the headers state them (so the cases follow the sources)"""
    k, d = _src("kernels.h"), _src("device_types.h")
    a, b = re.search(r"constexpr size_t kPointLdsLimit = (\d+) \* (\d+);", k).groups()
    block = int(re.search(r"#define MOVBA_POINT_BLOCK (\d+)", d).group(1))
    m = re.search(r"constexpr int kPointRed = (\d+) \* \(kPointBlock / (\d+)\) > (\d+) \? (\d+) \* \(kPointBlock / (\d+)\) : (\d+);", d)
    f, q, lim, f2, q2, lo = (int(v) for v in m.groups())
    assert (f, q, lim) == (f2, q2, lo)
    own = int(re.search(r"kPcgPlanOwnBatch = (\d+);", k).group(1))
    return dict(point_lds_limit=int(a) * int(b), point_red=max(f * (block // q), lo), own_batch=own)


def point_lds_need(NP, nfree):
    """kernels.hip, point_lds_need: the back-substitution pass's LDS image of NP keyframes, nfree of them free"""
    return (24 * NP + 6 * nfree + constants()["point_red"]) * 8 + 4 * NP + 16


def smallest_np_beyond_the_lds_limit(nfree):
    NP = nfree + 1
    while point_lds_need(NP, nfree) <= constants()["point_lds_limit"]:
        NP += 1
    return NP


def covisibility(w):
    """free keyframes with an edge (the reduced system's block rows, ascending id) and which of them share a point"""
    free = w.pose_fixed == 0
    active = np.zeros(w.n_poses, bool); active[w.edge_pose] = True
    idx = np.flatnonzero(free & active)
    h = -np.ones(w.n_poses, int); h[idx] = np.arange(len(idx))
    m = h[w.edge_pose] >= 0
    A = np.zeros((w.n_points, len(idx)), np.int32); A[w.edge_point[m], h[w.edge_pose[m]]] = 1
    C = (A.T @ A) > 0
    np.fill_diagonal(C, True)
    return C


def row_lengths(w):
    """entries per block row of the PCG's gather lists (structure.cpp: the diagonal block and one entry per covisible free
    keyframe, rounded up to whole entry PAIRS); pcg_plan.cpp pads the pair sums iff none exceeds 2 * kPcgPlanOwnBatch"""
    return (covisibility(w).sum(1) + 1) & ~1


def band_estimate(w):
    """upload.cpp, choose_solver: k_band's estimated cycles for the window in ascending-id numbering (callers assert that the
    upload keeps that numbering); the default choice takes k_band iff this is at most the PCG's 130 000"""
    C = covisibility(w)
    nf = len(C)
    i, j = np.nonzero(C)
    bw = int(np.abs(i - j).max())
    m_avg = sum(min(bw, nf - 1 - k) for k in range(nf)) / nf
    rt = math.ceil((m_avg * (m_avg + 1.0) * 18.0 + 6.0 * m_avg) / 512.0)
    rp = max(1.0, math.ceil(m_avg * 36.0 / 512.0))
    return nf * (1970.0 + 780.0 * rp + 420.0 * rt) + 54.0 * nf * (bw + 1) + 360.0 * nf + 5000.0


# name -> (free, fixed, points, seed, run_lo, run_hi); "-st": the same kind with half of its edges stereo
_KINDS = {
    "small": (8, 2, 200, 11, 2, 6),             # synth.cfg("small"): eight free keyframes, one per wave
    "cfg2": (10, 2, 2000, 1002, 2, 6),          # synth.cfg("cfg2")
    "nf5": (5, 2, 400, 4105, 2, 5),             # fewer keyframes than waves
    "nf9": (9, 2, 600, 4109, 2, 6),             # the first aggregated coarse level
    "cut": (6, 2, 6000, 17, 8, 8),              # pairs cut into several work items
    "band": (16, 3, 1500, 4116, 2, 6),          # the default choice gives it to k_band
    "nf17": (17, 2, 900, 4117, 3, 7),
    "nf40": (40, 4, 3000, 4140, 2, 8),          # the default choice gives it to the PCG
}
MONO = list(_KINDS)
STEREO = [n + "-st" for n in _KINDS]
MAX_ITERS = {"BIG": 3, "BIG-st": 3}


@functools.lru_cache(maxsize=None)
def window(name):
    """The case windows, built once per process and never changed."""
    if name in ("BIG", "BIG-st"):
        NP = smallest_np_beyond_the_lds_limit(12)
        return synth.make_window(12, NP - 12, 1000, seed=4312, run_lo=2, run_hi=6, stereo_frac=0.5 if name == "BIG-st" else 0.0)
    if name == "SPILL":
        return synth.make_window(40, 4, 3000, seed=5, run_lo=10, run_hi=30)
    if name == "WIDE":
        return synth.make_window(30, 3, 2500, seed=4201, run_lo=8, run_hi=12)
    st = name.endswith("-st")
    K, F, P, seed, lo, hi = _KINDS[name[:-3] if st else name]
    return synth.make_window(K, F, P, seed=seed + (500 if st else 0), run_lo=lo, run_hi=hi, stereo_frac=0.5 if st else 0.0)


def is_stereo(w):
    return w.obs_right is not None and bool((w.obs_right >= 0).any())


def test_constants_are_read_from_the_headers():
    c = constants()
    assert c["point_lds_limit"] >= 64 * 1024 and c["point_red"] >= 8 and c["own_batch"] >= 1
    # (the limit the issue speaks of: about 780 keyframes in all)
    assert 700 <= smallest_np_beyond_the_lds_limit(12) <= 900


def test_named_windows_are_the_configurations_they_stand_for():
    for name in ("small", "cfg2"):
        a, b = window(name), synth.cfg(name)
        for f in ("poses", "pose_fixed", "points", "edge_pose", "edge_point", "obs"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (name, f)


@pytest.mark.parametrize("name", MONO + STEREO)
def test_bystanders_flip_no_property_of_the_fold(built_lib, name):
    """on chip, no overflow, padded, staged in LDS: a batch of bystanders alone runs <ldsp=1, overflow=0, padded=1>"""
    w = window(name)
    plan = built_lib.structure_probe(w)
    assert plan["pcg_on_chip"] and not plan["pcg_overflow"] and plan["pcg_max_wave_entries"] <= 128
    rows = row_lengths(w)
    assert rows.sum() == plan["n_row_entries"] and rows.max() <= 2 * constants()["own_batch"]
    assert point_lds_need(w.n_poses, plan["n_free"]) <= constants()["point_lds_limit"]
    assert is_stereo(w) == name.endswith("-st") and w.n_points <= 6000 and w.max_iters <= 10
    assert plan["n_free"] == _KINDS[name[:-3] if name.endswith("-st") else name][0]


def test_bystanders_cover_the_kinds_the_batch_treats_differently(built_lib):
    for sfx in ("", "-st"):
        nf = {n: built_lib.structure_probe(window(n + sfx))["n_free"] for n in _KINDS}
        assert nf["small"] == 8 and nf["nf5"] < 8 and nf["nf9"] == 9 and nf["nf17"] > 16       # one keyframe per wave / first aggregates / three rows in a wave
        plan = built_lib.structure_probe(window("cut" + sfx))
        assert plan["n_items"] >= plan["n_pairs"] + 2 * (plan["n_pairs"] - plan["n_free"])     # pairs cut into several work items
        # the default solver choice: k_band for "band", the PCG for "nf40" (numbering as given, so the band is the one computed here)
        for n in ("band", "nf40"):
            assert not built_lib.structure_probe(window(n + sfx))["reordered"]
        assert band_estimate(window("band" + sfx)) <= 0.8 * 130000.0 and band_estimate(window("nf40" + sfx)) >= 1.2 * 130000.0


@pytest.mark.parametrize("name", ["BIG", "BIG-st"])
def test_big_is_the_smallest_window_beyond_the_point_kernels_lds_image(built_lib, name):
    w = window(name)
    plan = built_lib.structure_probe(w)
    lim = constants()["point_lds_limit"]
    assert plan["n_free"] == 12 and w.n_free == 12
    assert point_lds_need(w.n_poses, 12) > lim >= point_lds_need(w.n_poses - 1, 12)
    # flips nothing else: on chip, no overflow, padded
    assert plan["pcg_on_chip"] and not plan["pcg_overflow"] and row_lengths(w).max() <= 2 * constants()["own_batch"]
    assert w.n_points == 1000 and MAX_ITERS[name] == 3 and is_stereo(w) == (name == "BIG-st")


def test_spill_overflows_the_pcg_workgroups_registers(built_lib):
    w = window("SPILL")
    plan = built_lib.structure_probe(w)
    assert plan["pcg_on_chip"] and plan["pcg_overflow"] and plan["pcg_max_wave_entries"] > 128
    assert point_lds_need(w.n_poses, plan["n_free"]) <= constants()["point_lds_limit"] and not is_stereo(w)


def test_wide_has_a_long_block_row_and_no_overflow(built_lib):
    w = window("WIDE")
    plan = built_lib.structure_probe(w)
    rows = row_lengths(w)
    assert plan["pcg_on_chip"] and not plan["pcg_overflow"] and plan["pcg_max_wave_entries"] <= 128
    assert rows.sum() == plan["n_row_entries"] and rows.max() > 2 * constants()["own_batch"]
    assert point_lds_need(w.n_poses, plan["n_free"]) <= constants()["point_lds_limit"] and not is_stereo(w)
    assert band_estimate(w) >= 1.2 * 130000.0 and not plan["reordered"]      # the PCG by default: the packed kernel solves it
