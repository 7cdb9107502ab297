"""movba_express without a GPU: the two restatements the GPU tests compare against (tests/express_ref.py) held equal on every
case, and the coverage the cases must have before any device comparison; the symbols, the struct layouts, movba_express_grid and
every refusal of the header through the built library (the checks run before the handle is touched); the library's own steps
on the CPU (tests/express/ex_main.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement; and the host
side of the call - checks, packing, copy-out, pinned and ordinary results, a handle shared with a window, two handles on two
threads - under the sanitizers (tests/express: a stand-alone driver against the stand-in runtime of tests/hipstub and a fake
launch of its own).  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import express_ref as R
from conftest import ROOT

EX_DIR = os.path.join(ROOT, "tests", "express")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")


# ---- the restatements and their cases ------------------------------------------------------------------------------------------

def test_the_two_restatements_agree_on_every_case():
    images, items, thr, _ = R.coverage_case()
    fast = R.ref_express(images, items, thr, literal=False)
    R.compare(fast, R.coverage_ref(), "coverage")
    assert np.array_equal(fast["passes"], R.coverage_ref()["passes"])
    images, items, thr = R.mixed_case()
    fast = R.ref_express(images, items, thr, R.mixed_refs(), literal=False)
    R.compare(fast, R.mixed_ref(), "mixed")
    assert np.array_equal(fast["passes"], R.mixed_ref()["passes"])
    R.compare(R.ref_express(images, items, thr, None, literal=False), R.mixed_ref(False), "mixed, no references")
    fast = R.ref_express(*R.many_case(), literal=False)
    R.compare(fast, R.many_ref(), "many")
    assert np.array_equal(fast["passes"], R.many_ref()["passes"])


def test_many_case_is_what_the_gpu_test_asks_for():
    """what takes k_express_counts to its second, third and fourth workgroup: features in images above 255, 511 and 767"""
    images, items, thr = R.many_case()
    ref = R.many_ref()
    assert len(images) == len(items) == R.MANY_IMAGES == 1024 and thr == 25
    counts = np.array([len(r) for r, _ in items])
    assert counts.min() == 0 and counts.max() == 3 and set(counts.tolist()) == {0, 1, 2, 3}
    assert all((im is None) == (n == 0) for im, n in zip(images, counts))
    shapes = [im.shape for im in images if im is not None]
    assert all(17 <= r <= 24 and 17 <= c <= 40 for r, c in shapes) and len(set(shapes)) > 100
    # images without items first, last and in a run in the middle
    assert counts[0] == 0 and counts[-1] == 0 and (counts[300:304] == 0).all() and counts[1:300].any() and counts[304:-1].any()
    assert np.array_equal(np.diff(ref["item_ptr"]), counts)
    feats = ref["n_features"]
    assert feats.shape == (1024,) and feats.sum() == (ref["code"] == R.EX_FEATURE).sum()
    for block in range(4):                  # (one workgroup of k_express_counts per 256 images)
        part = feats[256 * block:256 * (block + 1)]
        assert (part > 0).sum() >= 20 and (part == 0).sum() >= 20, block
    assert feats[256:].any() and feats[512:].any() and feats[768:].any() and set(feats.tolist()) >= {0, 1, 2}
    assert (feats[counts == 0] == 0).all() and (feats < counts).any()


def test_coverage_case_meets_the_input_conditions():
    """Per shape at least 10 items each of code 1 from pass 0, code 1 from pass 1, code 18 and code 19; a block whose `low`
    wrapped, one whose `high` wrapped, one with all pixels outside; noise gives only code 19; images of 48 x 56 and smaller."""
    images, items, thr, shape_of = R.coverage_case()
    ref = R.coverage_ref()
    assert thr == 25 and all(im.shape[0] <= 48 and im.shape[1] <= 56 for im in images)
    assert len(shape_of) == len(ref["code"]) and set(ref["code"].tolist()) == {R.EX_FEATURE, R.EX_REJ_FLAT, R.EX_REJ_NO_EDGE}
    for s, shape in enumerate(R.SHAPES):
        m = shape_of == s
        tally = dict(pass0=int(((ref["code"] == 1) & (ref["passes"] == 1) & m).sum()), pass1=int(((ref["code"] == 1) & (ref["passes"] == 2) & m).sum()),
                     flat=int(((ref["code"] == 18) & m).sum()), no_edge=int(((ref["code"] == 19) & m).sum()))
        assert min(tally.values()) >= 10, (shape, tally)
    assert ((ref["passes"] > 0) == (ref["code"] == 1)).all()
    low_wrapped = high_wrapped = all_outside = 0
    for i, (image, (rects, _)) in enumerate(zip(images, items)):
        for k, rect in enumerate(rects):
            x0, y0, w, h = (int(v) for v in rect)
            center = R.compute_center(R.Block(image, rect))
            low_wrapped += center - thr < 0
            high_wrapped += center + thr > 255
            low, high = (center - thr) & 255, (center + thr) & 255
            blk = image[y0:y0 + h, x0 + 1:x0 + w + 1].astype(int)
            all_outside += bool(((blk < low) | (blk > high)).all())
    assert low_wrapped >= 1 and high_wrapped >= 1 and all_outside >= 1
    # the last two images are noise, the three before them flat
    ptr = ref["item_ptr"]
    assert (ref["code"][ptr[-3]:] == R.EX_REJ_NO_EDGE).all()
    assert (ref["code"][ptr[-6]:ptr[-5]] == R.EX_REJ_FLAT).all()                # mid-grey: nothing is outside
    assert (ref["code"][ptr[-5]:ptr[-3]] == R.EX_REJ_NO_EDGE).all()             # dark and bright: the bounds wrap, everything is
    assert ref["n_features"].sum() == (ref["code"] == 1).sum() and (ref["n_features"][-5:] == 0).all()


def test_mixed_case_is_what_the_gpu_test_asks_for():
    images, items, thr = R.mixed_case()
    ref = R.mixed_ref()
    shapes = [im.shape for im in images]
    assert shapes[0] == (17, 17) and shapes[3] == (64, 80) and len(set(shapes)) == 6 and len(items[2][0]) == 0
    assert images[3].strides[0] > images[3].shape[1] and (images[3].base[:, 80:] == 0xA5).all()
    assert sorted(set(thr)) == [0, 25, 255]
    assert set(ref["code"].tolist()) == {1, 2, 16, 17, 18, 19}
    rects = np.concatenate([r for r, _ in items])
    modes = np.concatenate([m for _, m in items])
    read = ref["code"] < 16
    assert set(map(tuple, rects[read][:, 2:].tolist())) == set(R.SHAPES)
    assert (rects[read][:, 0] % 2 == 0).any() and (rects[read][:, 0] % 2 == 1).any()
    assert ((rects[:, 0] == 0) & (rects[:, 1] == 0) & read).any()
    assert set(modes.tolist()) == {0, 1} and {2} == set(ref["code"][(modes == 1) & read].tolist())
    for i, (im, (r, _)) in enumerate(zip(images, items)):
        a, b = ref["item_ptr"][i], ref["item_ptr"][i + 1]
        if not len(r):
            continue
        last_col = r[:, 0].astype(np.int64) + r[:, 2] == im.shape[1] - 1
        touches = r[:, 0].astype(np.int64) + r[:, 2] == im.shape[1]
        assert (ref["code"][a:b][last_col & (r[:, 1] >= 0)] < 16).any() and (ref["code"][a:b][touches] == 16).all() and touches.any()
        assert (ref["code"][a:b][r[:, 0] < 0] == 16).all() and (r[:, 0] < 0).any()
    assert (ref["code"][(rects[:, 2] == 4) & (rects[:, 0] == 0)] == 17).all() and (ref["code"][rects[:, 3] == 32] >= 16).all()
    assert (ref["distance"][read] >= 0).all() and (ref["distance"][~read] == -1).all() and (R.mixed_ref(False)["distance"] == -1).all()
    assert (ref["count"][~read] == -1).all() and (ref["desc"][~read] == 0).all()


def test_descriptor_bit_order_and_overlap():
    """One outside pixel at shifted (y, x) sets bit y * h + x: on a 16 x 8 block (w = 16, h = 8) two pixels share a bit."""
    for w, h in R.SHAPES:
        for y, x in ((0, 0), (1, 0), (h - 1, w - 1), (3, 5)):
            img = np.full((40, 40), 100, np.uint8)
            img[4 + y, 6 + x + 1] = 200
            for one in (R.literal_item, R.fast_item):
                code, desc, count, _, _ = one(img, (6, 4, w, h), R.EX_DESCRIBE, 25)
                assert code == R.EX_DESCRIBED and count == 1 and desc == 1 << (y * h + x), (w, h, y, x)
    img = np.full((40, 40), 100, np.uint8)
    img[4, 6 + 8 + 1] = 200; img[5, 6 + 0 + 1] = 200          # (0, 8) and (1, 0) of a 16 x 8 block: both bit 8
    assert R.literal_item(img, (6, 4, 16, 8), R.EX_DESCRIBE, 25)[1:3] == (1 << 8, 1)


# ---- C-ABI without a device ------------------------------------------------------------------------------------------------

def test_symbols_and_struct_layouts(built_lib, tmp_path):
    for hooks in (False, True):
        assert hasattr(built_lib.lib(hooks), "movba_express") and hasattr(built_lib.lib(hooks), "movba_express_grid")
    assert "movba_express" in built_lib.EXPORTS and "movba_express_grid" in built_lib.EXPORTS and built_lib.lib().movba_version() == 5
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "movba.h"', 'int main(void) {']
    for st, cls in (("movba_express_desc", built_lib.ExpressDesc), ("movba_express_result", built_lib.ExpressResult)):
        src.append(f'printf("%zu", sizeof({st}));')
        src += [f'printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        src.append('printf("\\n");')
    src += ['printf("%d %d %d %d %d %d %d %d %d %d\\n", MOVBA_MAX_EXPRESS_IMAGES, MOVBA_MAX_EXPRESS_ITEMS, MOVBA_EX_DETECT, MOVBA_EX_DESCRIBE, '
            'MOVBA_EX_FEATURE, MOVBA_EX_DESCRIBED, MOVBA_EX_REJ_BOUNDS, MOVBA_EX_REJ_SHAPE, MOVBA_EX_REJ_FLAT, MOVBA_EX_REJ_NO_EDGE);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    for row, cls in zip(rows, (built_lib.ExpressDesc, built_lib.ExpressResult)):
        assert row[0] == C.sizeof(cls) and row[0] % 8 == 0
        assert row[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert C.sizeof(built_lib.ExpressDesc) == 80 and C.sizeof(built_lib.ExpressResult) == 48
    assert rows[2] == [1024, 1 << 22, 0, 1, 1, 2, 16, 17, 18, 19]
    assert rows[2] == [built_lib.MAX_EXPRESS_IMAGES, built_lib.MAX_EXPRESS_ITEMS, built_lib.EX_DETECT, built_lib.EX_DESCRIBE, built_lib.EX_FEATURE,
                       built_lib.EX_DESCRIBED, built_lib.EX_REJ_BOUNDS, built_lib.EX_REJ_SHAPE, built_lib.EX_REJ_FLAT, built_lib.EX_REJ_NO_EDGE]


@pytest.mark.parametrize("rows,cols", [(16, 16), (17, 17), (24, 24), (25, 40), (240, 320), (16, 400), (400, 16), (1, 1)])
def test_grid_is_the_lattice_of_extract_moves(built_lib, rows, cols):
    want = np.array([(x - 8, y - 8, 16, 16) for y in range(8, rows - 8, 16) for x in range(8, cols - 8, 16)], np.int32).reshape(-1, 4)
    got = built_lib.express_grid(rows, cols)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if rows <= 16 or cols <= 16:
        assert len(got) == 0
    else:
        assert len(got) == ((rows - 1) // 16) * ((cols - 1) // 16) > 0
    # up to cap: the first rects and no more, the lattice's size all the same
    if len(want) > 1:
        part = np.full((len(want), 4), -7, np.int32)
        assert built_lib.lib().movba_express_grid(rows, cols, part.ctypes.data_as(C.POINTER(C.c_int32)), len(want) - 1) == len(want)
        assert np.array_equal(part[:-1], want[:-1]) and (part[-1] == -7).all()


def test_grid_of_a_1080p_frame_and_its_refusals(built_lib):
    L_ = built_lib.lib()
    assert len(built_lib.express_grid(1080, 1920)) == 7973
    assert L_.movba_express_grid(100, 100, None, -1) == built_lib.ERR_ARG and L_.movba_express_grid(100, 100, None, 2) == built_lib.ERR_ARG
    assert L_.movba_express_grid(2 ** 31 - 1, 2 ** 31 - 1, None, 0) == built_lib.ERR_ARG


def _small_case():
    rng = np.random.default_rng(4)
    images = [R.edge_image(rng, 30, 34), R.edge_image(rng, 20, 52), R.noise_image(rng, 25, 25), R.edge_image(rng, 40, 40)]
    items = [(R.random_rects(rng, 30, 34, (8, 8), 5), 0), (R.random_rects(rng, 20, 52, (16, 8), 4), 1), (np.zeros((0, 4), np.int32), 0),
             (R.random_rects(rng, 40, 40, (16, 16), 3), 0)]
    refs = [rng.integers(0, 2 ** 64, (len(r), 4), dtype=np.uint64) for r, _ in items]
    return images, items, [25, 40, 25, 0], refs


def test_every_refusal_of_the_header_writes_nothing_but_status(built_lib):
    """The checks run before the handle is used for anything, so a handle that is merely not NULL serves: no device is needed
    (the calls that go on to the device are the GPU tests' and the sanitizer driver's)."""
    L_ = built_lib.lib()
    dummy = C.create_string_buffer(64)
    h = C.cast(dummy, C.c_void_p)

    def call(mutate=None, handle=h, desc=True, result=True):
        d, keep = built_lib.express_desc(*_small_case())
        r, out = built_lib.express_result(len(keep["item_rect"]), d.n_images, alloc=lambda shape, dtype: np.full(shape, 0x77, dtype))
        r.status = 99
        if mutate:
            mutate(d, keep, r)
        rc = L_.movba_express(handle, C.byref(d) if desc else None, C.byref(r) if result else None)
        clean = all((a == 0x77).all() for a in out.values())
        return rc, r.status, clean

    def null(field, res=False):
        return lambda d, keep, r: setattr(r if res else d, field, None)

    def put(key, index, value):
        return lambda d, keep, r: keep[key].__setitem__(index, value)

    refusals = {
        "negative n_images": lambda d, keep, r: setattr(d, "n_images", -1), "n_images above the bound": lambda d, keep, r: setattr(d, "n_images", 1025),
        "item_ptr not starting at 0": put("item_ptr", 0, 1), "item_ptr descending": put("item_ptr", 2, 3), "item_ptr negative": put("item_ptr", 0, -2),
        "n_items above the bound": put("item_ptr", slice(1, None), (1 << 22) + 1),
        "a NULL image that has items": lambda d, keep, r: keep["image"].__setitem__(1, None),
        "rows 0": put("rows", 0, 0), "cols 0": put("cols", 3, 0), "rows negative, no items": put("rows", 2, -1), "stride below cols": put("stride", 1, 51),
        "stride 0": put("stride", 0, 0), "threshold -1": put("threshold", 0, -1), "threshold 256": put("threshold", 2, 256),
        "unknown mode": put("item_mode", 4, 2), "negative mode": put("item_mode", 0, -1), "unknown mode, last item": put("item_mode", -1, 9),
        "more than 2^28 pixels": lambda d, keep, r: (keep["rows"].__setitem__(slice(None), 16384), keep["cols"].__setitem__(slice(None), 16384),
                                                     keep["stride"].__setitem__(slice(None), 16384)),
    }
    for field in ("image", "rows", "cols", "stride", "threshold", "item_ptr", "item_rect", "item_mode"):
        refusals["NULL " + field] = null(field)
    for field in ("code", "desc", "count", "n_features"):
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
    # no images, or no items at all: MOVBA_OK, the status and nothing else - whatever else the descriptor holds
    rc, status, clean = call(lambda d, keep, r: setattr(d, "n_images", 0))
    assert rc == 0 and status == 0 and clean
    rc, status, clean = call(lambda d, keep, r: (keep["item_ptr"].__setitem__(slice(None), 0), setattr(d, "rows", None), setattr(r, "code", None)))
    assert rc == 0 and status == 0 and clean


# ---- the library's own steps on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ex_main():
    subprocess.check_call(["make", "-C", EX_DIR, "-s", "ex_main_asan"])
    return os.path.join(EX_DIR, "ex_main_asan")


def run_ex_main(exe, images, items, thresholds, refs, tmp_path):
    """tests/express/ex_main.cpp on one call -> the fields of Solver.express's dict, plus `passes`"""
    from movba import capi
    d, keep = capi.express_desc(images, items, thresholds, refs)
    n, ni = len(keep["item_rect"]), d.n_images
    src, dst = os.path.join(str(tmp_path), "call.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([ni, n, int(refs is not None)], np.int32).tobytes())
        for key in ("rows", "cols", "threshold", "item_ptr", "item_rect", "item_mode"):
            f.write(keep[key].tobytes())
        if refs is not None:
            f.write(keep["item_ref"].tobytes())
        for im in images:
            f.write(b"\0" if im is None else np.ascontiguousarray(im).tobytes())        # (None: 1 x 1 in the descriptor, never read)
    r = subprocess.run([exe, src, dst], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ex_main: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    blob = open(dst, "rb").read()
    at = 0

    def take(count, dtype):
        nonlocal at
        a = np.frombuffer(blob, dtype, count, at)
        at += a.nbytes
        return a

    out = dict(count=take(n, np.int32), distance=take(n, np.int32), n_features=take(ni, np.int32), passes=take(n, np.int32),
               desc=take(4 * n, np.uint64).reshape(n, 4), code=take(n, np.uint8), item_ptr=keep["item_ptr"])
    assert at == len(blob)
    return out


def test_the_librarys_steps_on_the_coverage_case(ex_main, tmp_path):
    images, items, thr, _ = R.coverage_case()
    got = run_ex_main(ex_main, images, items, thr, None, tmp_path)
    R.compare(got, R.coverage_ref(), "coverage")
    assert np.array_equal(got["passes"], R.coverage_ref()["passes"])


def test_the_librarys_steps_on_the_mixed_case(ex_main, tmp_path):
    images, items, thr = R.mixed_case()
    got = run_ex_main(ex_main, images, items, thr, R.mixed_refs(), tmp_path)
    R.compare(got, R.mixed_ref(), "mixed")
    assert np.array_equal(got["passes"], R.mixed_ref()["passes"])
    R.compare(run_ex_main(ex_main, images, items, thr, None, tmp_path), R.mixed_ref(False), "mixed, no references")


def test_the_librarys_steps_on_the_many_case(ex_main, tmp_path):
    got = run_ex_main(ex_main, *R.many_case(), None, tmp_path)
    R.compare(got, R.many_ref(), "many")
    assert np.array_equal(got["passes"], R.many_ref()["passes"])


def test_the_librarys_diagonals_are_the_rules(ex_main, tmp_path):
    """Blocks cut along one diagonal of pass 0 - the last `rounds` diagonals on one side of the bounds, the others on the other -
    and their mirror images, whose cut runs along a diagonal of pass 1: on the square shapes the first passes pass 0, the mirror
    image only pass 1."""
    imgs, items = [], []
    for w, h in R.SHAPES:
        slices = w + h - 1
        rounds = {15: 4, 23: 6, 31: 8}[slices]
        img = np.full((h + 2, w + 4), 100, np.uint8)
        Y, X = np.mgrid[0:h, 0:w]
        img[:h, 2:2 + w][(X - Y + h - 1) < slices - rounds] = 200
        imgs += [img, np.ascontiguousarray(img[:, ::-1])]
        items += [(np.array([[2, 0, w, h]], np.int32), 0)] * 2
    ref = R.ref_express(imgs, items, 25)
    got = run_ex_main(ex_main, imgs, items, 25, None, tmp_path)
    R.compare(got, ref, "cut along a diagonal")
    assert np.array_equal(got["passes"], ref["passes"])
    assert ref["passes"][[0, 1, 6, 7]].tolist() == [1, 2, 1, 2]


# ---- the host side under the sanitizers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["express_asan", "express_tsan"])
def test_host_side_under_sanitizers(target):
    """tests/express/express_driver.cpp: every refusal of the header with nothing written, calls without images or items, padded
    rows, images without items, the optional arrays left out, pinned against ordinary result memory, calls of growing and
    shrinking size up to a 1080p frame, the call between upload, run, download and reset of a window on the same handle,
    movba_express_grid, and two handles on two threads - with the library's host sources, the stand-in runtime and fakes of
    tests/hipstub and the fake launch of tests/express linked into one program."""
    subprocess.check_call(["make", "-C", EX_DIR, "-s", target])
    r = subprocess.run([os.path.join(EX_DIR, target)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "express driver: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
