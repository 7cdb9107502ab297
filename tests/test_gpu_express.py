"""movba_express on the device against the literal restatement of tests/express_ref.py, every comparison exact equality: the mixed
call array by array, 1 024 images (k_express_counts over four workgroups), item counts that leave workgroups partly filled, the
grid of a 240 x 320 frame, independence of an item
from everything but its own rect, mode, reference and image (reordered, split over calls, a pixel changed elsewhere), pinned
results, a solved window on the same handle left as it was, a refusal on a live handle, and the distance against an item's own
descriptor and its complement.  Every rect handed to the device is inside its image by the reference's own test or carries a
code that keeps the kernel from reading it."""
import ctypes as C

import numpy as np
import pytest

import express_ref as R
from movba import capi, synth

pytestmark = pytest.mark.gpu


def test_parity_with_the_restatement_on_a_mixed_call(solver):
    """5 images with items, 17 x 17 to 64 x 80, one with padded rows whose padding is poisoned, one image without items; both
    modes, all four shapes, odd and even x0, rects at (0, 0), rects that end one column before the last (accepted) and on it
    (code 16), negative x, 4 x 4 and 16 x 32 (code 17), thresholds 0, 25 and 255, with and without references: every array
    equals the literal restatement's, and the same call twice gives the same bits."""
    images, items, thr = R.mixed_case()
    got = solver.express(images, items, thr, R.mixed_refs())
    assert got["status"] == 0
    R.compare(got, R.mixed_ref(), "mixed")
    R.compare(solver.express(images, items, thr, R.mixed_refs()), got, "the same call twice")
    bare = solver.express(images, items, thr)
    R.compare(bare, R.mixed_ref(False), "no references")
    # an image without items may come as a NULL pointer; the distance array may be left out
    with_null = list(images)
    with_null[2] = None
    R.compare(solver.express(with_null, items, thr, R.mixed_refs()), R.mixed_ref(), "a NULL image without items")
    d, keep = capi.express_desc(images, items, thr, R.mixed_refs())
    r, out = capi.express_result(len(keep["item_rect"]), d.n_images, distance=False)
    assert solver._L.movba_express(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    for key in ("code", "desc", "count", "n_features"):
        assert np.array_equal(out[key], R.mixed_ref()[key]), key


def test_1024_images_take_the_counts_over_four_workgroups(solver):
    """MOVBA_MAX_EXPRESS_IMAGES images of 17 x 17 to 24 x 40 with 0 to 3 items each, the ones without items NULL - the first, the
    last and a run in the middle among them: k_express_counts, which only the device runs, over four workgroups.  n_features
    in full, and every item's row."""
    images, items, thr = R.many_case()
    ref = R.many_ref()
    got = solver.express(images, items, thr)
    assert got["status"] == 0 and got["n_features"].shape == (R.MANY_IMAGES,)
    assert np.array_equal(got["n_features"], ref["n_features"]), np.flatnonzero(got["n_features"] != ref["n_features"])[:8].tolist()
    R.compare(got, ref, "many")
    assert got["n_features"][256:512].any() and got["n_features"][512:768].any() and got["n_features"][768:].any()
    R.compare(solver.express(images, items, thr, pinned=True), ref, "many, pinned")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_item_counts_that_leave_a_workgroup_partly_filled(solver, n):
    images, items, thr, _ = R.coverage_case()
    image = images[0]
    rng = np.random.default_rng(n)
    rects = np.concatenate([R.random_rects(rng, *image.shape, R.SHAPES[k % 4], 1) for k in range(n)])
    modes = (np.arange(n) % 5 == 2).astype(np.int32)
    got = solver.express([image], [(rects, modes)], thr)
    R.compare(got, R.ref_express([image], [(rects, modes)], thr), f"{n} items")
    assert len(got["code"]) == n


def test_the_grid_of_a_frame(solver):
    """movba_express_grid of a 240 x 320 frame through the device: 14 x 19 rects, the last of which end one pixel short of the
    image's last row and column, so every one passes the bounds test."""
    rng = np.random.default_rng(9)
    frame = R.edge_image(rng, 240, 320)
    frame[60:180, 80:240] = R.edge_image(rng, 120, 160)
    frame[0:48, 0:64] = R.noise_image(rng, 48, 64)
    rects = capi.express_grid(240, 320)
    assert rects.shape == (14 * 19, 4) and rects[-1].tolist() == [288, 208, 16, 16]
    got = solver.express([frame], [(rects, R.EX_DETECT)], 25)
    ref = R.ref_express([frame], [(rects, R.EX_DETECT)], 25)
    R.compare(got, ref, "grid")
    assert set(ref["code"].tolist()) == {R.EX_FEATURE, R.EX_REJ_FLAT, R.EX_REJ_NO_EDGE} and ref["n_features"][0] >= 5


def test_an_item_depends_on_its_own_data_alone(built_lib):
    images, items, thr = R.mixed_case()
    refs = R.mixed_refs()
    ni = len(images)
    s = built_lib.Solver()
    try:
        whole = s.express(images, items, thr, refs)
        R.compare(whole, R.mixed_ref(), "whole")
        ptr = whole["item_ptr"]
        want = [R.rows(whole, range(ptr[i], ptr[i + 1])) for i in range(ni)]
        # images and items reversed
        order = list(range(ni - 1, -1, -1))
        rev = s.express([images[i] for i in order], [(items[i][0][::-1], items[i][1][::-1]) for i in order], [thr[i] for i in order],
                        [refs[i][::-1] for i in order])
        for pos, i in enumerate(order):
            assert R.rows(rev, range(rev["item_ptr"][pos], rev["item_ptr"][pos + 1])) == want[i][::-1], i
            assert rev["n_features"][pos] == whole["n_features"][i]
        # one call per image
        for i in range(ni):
            if not len(items[i][0]):
                continue
            one = s.express([images[i]], [items[i]], [thr[i]], [refs[i]])
            assert R.rows(one, range(len(items[i][0]))) == want[i], i
            assert one["n_features"][0] == whole["n_features"][i]
        # a pixel outside every pixel an item reads leaves the item's row as it was
        i = 5
        image, (rects, modes) = images[i], items[i]
        codes = whole["code"][ptr[i]:ptr[i + 1]]
        k = int(np.flatnonzero((codes == R.EX_FEATURE) & (rects[:, 2] == 8) & (rects[:, 3] == 8))[0])
        read = R.read_pixels(rects[k], image.shape[1])
        x0, y0, w, h = (int(v) for v in rects[k])
        near = [(y0 - 1, x0), (y0, x0 - 1), (y0 + h, x0), (y0, x0 + w + 1), (y0 + h - 1, x0 + w + 1)]
        near = [(y, x) for y, x in near if 0 <= y < image.shape[0] and 0 <= x < image.shape[1] and (y, x) not in read]
        assert len(near) >= 2
        changed = image.copy()
        for y, x in near:
            changed[y, x] ^= 0xFF
        after = s.express([changed], [(rects, modes)], [thr[i]], [refs[i]])
        assert R.rows(after, [k]) == [want[i][k]]
        R.compare(after, R.ref_express([changed], [(rects, modes)], [thr[i]], [refs[i]]), "changed image")
        # ... and a pixel it does read does not (the shifted column belongs to the block)
        changed = image.copy()
        changed[y0:y0 + h, x0 + w] ^= 0xFF
        after = s.express([changed], [(rects, modes)], [thr[i]], [refs[i]])
        assert R.rows(after, [k]) != [want[i][k]]
        R.compare(after, R.ref_express([changed], [(rects, modes)], [thr[i]], [refs[i]]), "changed shifted column")
    finally:
        s.close()


def test_pinned_results_equal_ordinary_results(built_lib):
    s = built_lib.Solver()
    try:
        images, items, thr = R.mixed_case()
        R.compare(s.express(images, items, thr, R.mixed_refs(), pinned=True), s.express(images, items, thr, R.mixed_refs()), "pinned")
        R.compare(s.express(images, items, thr, R.mixed_refs(), pinned=True), R.mixed_ref(), "pinned against the restatement")
        images, items, thr, _ = R.coverage_case()
        R.compare(s.express(images, items, thr, pinned=True), R.coverage_ref(), "coverage, pinned")
        R.compare(s.express(images, items, thr), R.coverage_ref(), "coverage")
    finally:
        s.close()


def test_a_window_on_the_same_handle_is_left_as_it_was(built_lib):
    """A solved window's download before and after an express call is bit-identical, later runs too; and the call gives on the
    handle of a solved window what it gives on a fresh one."""
    w = synth.cfg("small")
    images, items, thr = R.mixed_case()
    keys = ("poses", "points", "chi2", "outlier", "n_solves", "cost", "lam")
    s = built_lib.Solver()
    try:
        first = s.solve(w)
        before = s.download()
        R.compare(s.express(images, items, thr, R.mixed_refs()), R.mixed_ref(), "after the solve")
        after = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(first[k]), np.asarray(before[k])) and np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
        assert s._L.movba_lba_reset(s._h) == 0
        R.compare(s.express(images, items, thr, R.mixed_refs(), pinned=True), R.mixed_ref(), "after the reset, pinned")
        s.run()
        again = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(again[k]), np.asarray(first[k])), k
        s.upload(w)
        R.compare(s.express(images, items, thr), R.mixed_ref(False), "between upload and run")
        s.run()
        fresh = s.download()
        for k in keys:
            assert np.array_equal(np.asarray(fresh[k]), np.asarray(first[k])), k
    finally:
        s.close()


def test_a_refusal_and_a_call_without_items_on_a_live_handle(solver):
    images, items, thr = R.mixed_case()
    d, keep = capi.express_desc(images, items, thr, R.mixed_refs())
    keep["item_mode"][7] = 2                                    # one unknown mode
    r, out = capi.express_result(len(keep["item_rect"]), d.n_images, alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
    r.status = 99
    assert solver._L.movba_express(solver._h, C.byref(d), C.byref(r)) == capi.ERR_ARG
    assert r.status == capi.ERR_ARG and all((a == 0x77).all() for a in out.values())
    with pytest.raises(capi.MovbaError, match="argument"):
        solver.express(images, items, [25, 25, 256, 25, 25, 25])
    # no items: MOVBA_OK, and not one result entry is written
    empty = [(np.zeros((0, 4), np.int32), 0)] * len(images)
    d, keep = capi.express_desc(images, empty, thr)
    r, out = capi.express_result(3, len(images), alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
    r.status = 99
    assert solver._L.movba_express(solver._h, C.byref(d), C.byref(r)) == 0 and r.status == 0
    assert all((a == 0x77).all() for a in out.values())
    assert solver.express([], [], [])["status"] == 0
    R.compare(solver.express(images, items, thr, R.mixed_refs()), R.mixed_ref(), "after the refusal")


def test_distance_against_the_items_own_descriptor_and_its_complement(solver):
    """item_ref equal to the item's own descriptor gives 0; against its complement on the bits the shape uses it gives the
    number of those bits - count of the union."""
    images, items, thr, shape_of = R.coverage_case()
    ref = R.coverage_ref()
    ptr = ref["item_ptr"]
    own = [ref["desc"][ptr[i]:ptr[i + 1]] for i in range(len(images))]
    got = solver.express(images, items, thr, own)
    have = ref["code"] == R.EX_FEATURE
    assert have.sum() > 300 and (got["distance"][have] == 0).all() and (got["distance"][~have] == -1).all()
    # the bits a shape can set: y * h + x over the block
    used = []
    for w, h in R.SHAPES:
        bits = 0
        for y in range(h):
            for x in range(w):
                bits |= 1 << (y * h + x)
        used.append(R.words(bits))
    used = np.array(used, np.uint64)[shape_of]
    flipped = ref["desc"] ^ used
    got = solver.express(images, items, thr, [flipped[ptr[i]:ptr[i + 1]] for i in range(len(images))])
    union = np.array([sum(bin(int(v)).count("1") for v in row) for row in (ref["desc"] | flipped)], np.int32)
    assert (union[have] == np.array([[64, 72, 128, 256][s] for s in shape_of])[have]).all()
    assert np.array_equal(got["distance"][have], union[have]) and (got["distance"][~have] == -1).all()
    assert np.array_equal(got["desc"], ref["desc"]) and np.array_equal(got["count"], ref["count"])
