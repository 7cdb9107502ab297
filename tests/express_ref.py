"""movba_express restated from the rules of include/movba.h (what the CPU and GPU tests compare against), twice: literally - loop
by loop as EXPRESS.h:79-192 runs, uint8 counters, the row-wise `break` of the precheck and the `p++` in front of the read
included - and with numpy over whole blocks, written independently (tests/test_express_cpu.py holds the two equal on every
case); and the committed cases: the coverage set, the mixed call, the grid frame.  Everything is integer: every comparison is
exact equality.  Helper module: no tests here (tests/test_express_cpu.py, tests/test_gpu_express.py).

A call is (images, items, thresholds, refs) as movba.capi.express_desc takes them: images is a list of 2-D uint8 arrays (None for
an image without items), items a list of (rects (n, 4) x y w h, modes (n,)) per image, refs None or a list of (n, 4) uint64."""
import functools

import numpy as np

EX_DETECT, EX_DESCRIBE = 0, 1
EX_FEATURE, EX_DESCRIBED = 1, 2
EX_REJ_BOUNDS, EX_REJ_SHAPE, EX_REJ_FLAT, EX_REJ_NO_EDGE = 16, 17, 18, 19
SHAPES = ((8, 8), (16, 8), (8, 16), (16, 16))           # (w, h)
KEYS = ("code", "desc", "count", "distance")
ALL_BITS = (1 << 64) - 1


def words(bits: int) -> list:
    """a bitset<256> held in a Python int -> its four 64-bit words, bit k in bit k & 63 of word k >> 6"""
    return [(bits >> (64 * k)) & ALL_BITS for k in range(4)]


def rejected(rect, rows, cols):
    """the reference's `if`, strict as written, then the four shapes diagonal() knows"""
    x, y, w, h = (int(v) for v in rect)
    if not (x >= 0 and y >= 0 and x + w < cols and y + h < rows):
        return EX_REJ_BOUNDS
    if (w, h) not in SHAPES:
        return EX_REJ_SHAPE
    return 0


# ---- the literal restatement ------------------------------------------------------------------------------------------------

class Block:
    """cv::Mat img = imGray(rect): at(row, col) with rows = h, cols = w; nothing keeps an index inside the block"""

    def __init__(self, image, rect):
        self.image = image
        self.x0, self.y0, self.cols, self.rows = (int(v) for v in rect)

    def at(self, row, col):
        return int(self.image[self.y0 + row, self.x0 + col])


def compute_center(img):
    center_row = (img.rows // 2) & 255
    center_col = (img.cols // 2) & 255
    # (at<uint8_t>(center_col, center_row): the first argument of at<>() is the row)
    return (img.at(center_col, center_row) + img.at(center_col - 1, center_row - 1) + img.at(center_col, center_row - 1)
            + img.at(center_col - 1, center_row)) // 4


def compute_descriptor(img, threshold):
    center = compute_center(img)
    low_bounds = (center - threshold) & 255
    high_bounds = (center + threshold) & 255
    desc = 0
    for y in range(img.rows):
        p = 0
        for x in range(img.cols):
            p += 1
            v = img.at(y, p)
            if low_bounds > v or high_bounds < v:
                desc |= 1 << ((y * img.rows) + x)
    return desc


def diagonal(img, d, direction):
    """the pixels of diagonal d: direction true (pass 0) {(y, x): x - y = d - (rows - 1)}, false (pass 1) {(y, x): (cols - 1 -
    x) - y = d - (rows - 1)} - the rule, not the tables"""
    out = []
    for y in range(img.rows):
        a = y + d - (img.rows - 1)
        if 0 <= a < img.cols:
            out.append(img.at(y, a if direction else img.cols - 1 - a))
    return out


def compute_express(img, threshold):
    """-> (true / false, the precheck passed, the pass that succeeded or -1)"""
    center = compute_center(img)
    low_bounds = (center - threshold) & 255
    high_bounds = (center + threshold) & 255
    precheck = int(img.rows * img.cols * .125) & 255
    f = 0
    for row in range(img.rows):
        p = 0
        for col in range(img.cols):
            p += 1
            v = img.at(row, p)
            if low_bounds > v or high_bounds < v:
                f = (f + 1) & 255
        if f >= precheck:
            break
    if f < precheck:
        return False, False, -1
    slices = (img.rows + img.cols - 1) & 255
    rounds = int(np.floor(slices * .25 + .5)) & 255             # round(): halves away from zero, positive here
    u_rounds = (slices - rounds) & 255
    for a in range(2):
        wins = losses = 0
        for i in range(slices):
            win = loss = 0
            for v in diagonal(img, i, a == 0):
                if low_bounds > v or high_bounds < v:
                    win += 1
                else:
                    loss += 1
            if wins < rounds:
                wins = wins + 1 if win >= loss else 0
            if losses < rounds:
                losses = losses + 1 if loss > win else 0
            if i > u_rounds and (wins == 0 or losses == 0):
                break
        if wins >= rounds and losses >= rounds:
            return True, True, a
    return False, True, -1


def literal_item(image, rect, mode, threshold, ref=None):
    """-> (code, desc as an int, count, distance, pass: 0 none, 1 pass 0, 2 pass 1)"""
    code = rejected(rect, *image.shape) if image is not None else EX_REJ_BOUNDS
    if code:
        return code, 0, -1, -1, 0
    img = Block(image, rect)
    which = 0
    if mode == EX_DETECT:
        ok, pre, a = compute_express(img, threshold)
        if not ok:
            return (EX_REJ_NO_EDGE if pre else EX_REJ_FLAT), 0, -1, -1, 0
        which = a + 1
    desc = compute_descriptor(img, threshold)
    dist = -1 if ref is None else bin(desc ^ ref).count("1")
    return (EX_FEATURE if mode == EX_DETECT else EX_DESCRIBED), desc, bin(desc).count("1"), dist, which


# ---- the same with numpy over whole blocks ----------------------------------------------------------------------------------

def fast_item(image, rect, mode, threshold, ref=None):
    code = rejected(rect, *image.shape)
    if code:
        return code, 0, -1, -1, 0
    x0, y0, w, h = (int(v) for v in rect)
    I = image.astype(np.int64)
    r, c = w // 2, h // 2
    center = int(I[y0 + r - 1:y0 + r + 1, x0 + c - 1:x0 + c + 1].sum()) // 4
    low, high = (center - threshold) % 256, (center + threshold) % 256
    true = I[y0:y0 + h, x0:x0 + w]
    shifted = I[y0:y0 + h, x0 + 1:x0 + w + 1]
    out_t, out_s = (true < low) | (true > high), (shifted < low) | (shifted > high)
    Y, X = np.mgrid[0:h, 0:w]
    which = 0
    if mode == EX_DETECT:
        if int(out_s.sum()) < (h * w) // 8:
            return EX_REJ_FLAT, 0, -1, -1, 0
        slices = h + w - 1
        rounds = {15: 4, 23: 6, 31: 8}[slices]
        for a, index in enumerate((X - Y + h - 1, (w - 1 - X) - Y + h - 1)):
            length = np.bincount(index.ravel(), minlength=slices)
            win = np.bincount(index.ravel(), weights=out_t.ravel(), minlength=slices).astype(np.int64)
            loss = length - win
            wins = losses = 0
            for i in range(slices):
                if wins < rounds:
                    wins = wins + 1 if win[i] >= loss[i] else 0
                if losses < rounds:
                    losses = losses + 1 if loss[i] > win[i] else 0
                if i > slices - rounds and (wins == 0 or losses == 0):
                    break
            if wins >= rounds and losses >= rounds:
                which = a + 1
                break
        if not which:
            return EX_REJ_NO_EDGE, 0, -1, -1, 0
    bits = np.zeros(256, np.uint8)
    bits[(Y * h + X)[out_s]] = 1
    desc = int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")
    dist = -1 if ref is None else bin(desc ^ ref).count("1")
    return (EX_FEATURE if mode == EX_DETECT else EX_DESCRIBED), desc, bin(desc).count("1"), dist, which


# ---- a whole call -----------------------------------------------------------------------------------------------------------

def as_int(ref_words):
    return sum(int(v) << (64 * k) for k, v in enumerate(ref_words))


def ref_express(images, items, thresholds, refs=None, literal=True):
    """-> the fields of Solver.express's dict, plus `passes` (per item 0: no pass succeeded or none ran, 1: pass 0, 2: pass 1)"""
    thresholds = np.broadcast_to(np.asarray(thresholds, np.int32), (len(images),))
    one = literal_item if literal else fast_item
    code, desc, count, dist, passes, feats, ptr = [], [], [], [], [], [], [0]
    for i, (image, (rects, modes)) in enumerate(zip(images, items)):
        rects = np.asarray(rects, np.int32).reshape(-1, 4)
        modes = np.broadcast_to(np.asarray(modes, np.int32), (len(rects),))
        n = 0
        for k, (rect, mode) in enumerate(zip(rects, modes)):
            ref = None if refs is None else as_int(np.asarray(refs[i], np.uint64).reshape(-1, 4)[k])
            cd, ds, ct, di, ps = one(image, rect, int(mode), int(thresholds[i]), ref)
            code.append(cd); desc.append(words(ds)); count.append(ct); dist.append(di); passes.append(ps)
            n += cd == EX_FEATURE
        feats.append(n)
        ptr.append(len(code))
    return dict(status=0, code=np.array(code, np.uint8), desc=np.array(desc, np.uint64).reshape(-1, 4), count=np.array(count, np.int32),
                distance=np.array(dist, np.int32), n_features=np.array(feats, np.int32), item_ptr=np.array(ptr, np.int32),
                passes=np.array(passes, np.int32))


def rows(res, ks):
    """the per-item rows of a result, as tuples that compare"""
    return [(int(res["code"][k]), tuple(int(v) for v in res["desc"][k]), int(res["count"][k]), int(res["distance"][k])) for k in ks]


def compare(got, ref, label=""):
    for key in KEYS:
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (label, key)
        bad = np.flatnonzero((got[key] != ref[key]).reshape(len(ref[key]), -1).any(axis=1))
        assert not len(bad), (label, key, bad[:8].tolist(), got[key][bad[:3]].tolist(), ref[key][bad[:3]].tolist())
    assert np.array_equal(got["n_features"], ref["n_features"]), (label, got["n_features"].tolist(), ref["n_features"].tolist())
    assert np.array_equal(got["item_ptr"], ref["item_ptr"]), label


# ---- images -------------------------------------------------------------------------------------------------------------------

def edge_image(rng, rows_, cols):
    """a noisy step edge at a random angle through a random point of the middle of the image"""
    a, b = 0, 0
    while abs(a - b) < 60:
        a, b = (int(v) for v in rng.integers(30, 226, 2))
    angle = rng.uniform(0.0, np.pi)
    py, px = rng.uniform(0.25, 0.75) * rows_, rng.uniform(0.25, 0.75) * cols
    Y, X = np.mgrid[0:rows_, 0:cols]
    side = (X - px) * np.cos(angle) + (Y - py) * np.sin(angle) < 0
    img = np.where(side, a, b) + rng.integers(-8, 9, (rows_, cols))
    return np.clip(img, 0, 255).astype(np.uint8)


def flat_image(rows_, cols, value):
    return np.full((rows_, cols), value, np.uint8)


def noise_image(rng, rows_, cols):
    return rng.integers(0, 256, (rows_, cols)).astype(np.uint8)


def random_rects(rng, rows_, cols, shape, n):
    """n rects of one shape (w, h) that pass the reference's bounds test"""
    w, h = shape
    return np.stack([rng.integers(0, cols - w, n), rng.integers(0, rows_ - h, n), np.full(n, w), np.full(n, h)], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def coverage_case():
    """The set the CPU tests hold the restatements and the library's steps to: 40 step-edge images, 3 flat ones (mid-grey, dark -
    `low` wraps - and bright - `high` wraps) and 2 of uniform noise, 48 x 56 and
    smaller, threshold 25, every item DETECT; per step-edge image 10 random rects of every shape (400 blocks per shape).
    -> (images, items, thresholds, shape index per item)"""
    rng = np.random.default_rng(20221)
    images, items, shape_of = [], [], []

    def add(img, per_shape):
        rects = []
        for s, shape in enumerate(SHAPES):
            rects.append(random_rects(rng, img.shape[0], img.shape[1], shape, per_shape))
            shape_of.extend([s] * per_shape)
        images.append(img)
        items.append((np.concatenate(rects), np.zeros(4 * per_shape, np.int32)))

    for k in range(40):
        add(edge_image(rng, int(rng.integers(24, 49)), int(rng.integers(24, 57))), 10)
    for value in (128, 10, 245):
        add(flat_image(40, 44, value), 12)
    for k in range(2):
        add(noise_image(rng, 48, 56), 12)
    return images, items, 25, np.array(shape_of, np.int32)


@functools.lru_cache(maxsize=None)
def coverage_ref():
    images, items, thr, _ = coverage_case()
    return ref_express(images, items, thr)


MIXED_SIZES = ((17, 17), (33, 47), (40, 40), (64, 80), (25, 31), (48, 56))       # (rows, cols); [2] has no items, [3] a padded stride


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The mixed call of the GPU test: 5 images with items, 17 x 17 to 64 x 80, and one without; image 3 is a view into a wider
    array whose padding holds a poison value; thresholds 0, 25 and 255; both modes, all four shapes, odd and even x0, rects at
    (0, 0), rects with x + w == cols - 1 (accepted) and == cols (code 16), negative x, shapes 4 x 4 and 16 x 32 (code 17); every
    second image's items carry a reference.  -> (images, items, thresholds, refs)"""
    rng = np.random.default_rng(77)
    images, items = [], []
    thresholds = [25, 0, 25, 25, 255, 25]
    for i, (r, c) in enumerate(MIXED_SIZES):
        if i == 2:
            images.append(edge_image(rng, r, c)); items.append((np.zeros((0, 4), np.int32), np.zeros(0, np.int32)))
            continue
        img = edge_image(rng, r, c) if i != 4 else noise_image(rng, r, c)
        if i == 3:
            wide = np.full((r, c + 13), 0xA5, np.uint8)
            wide[:, :c] = img
            img = wide[:, :c]
        images.append(img)
        rects = [(0, 0, 8, 8), (0, 0, 16, 16), (c - 9, 0, 8, 8), (c - 8, 0, 8, 8), (0, r - 9, 8, 8), (0, r - 8, 8, 8), (-1, 0, 8, 8), (0, -3, 16, 8),
                 (0, 0, 4, 4), (1, 1, 16, 32), (c, r, 8, 8), (0, 0, 0, 0), (2, 2, -8, 8), (2 ** 31 - 1, 0, 16, 16), (0, 2 ** 31 - 8, 8, 16)]
        if r > 17:
            for shape in SHAPES:
                rects += random_rects(rng, r, c, shape, 12).tolist()
            rects += [(c - 17, r - 17, 16, 16), (c - 17, 1, 16, 8), (1, r - 17, 8, 16), (3, 5, 16, 8), (4, 5, 8, 16)]
        rects = np.array(rects, np.int64).astype(np.int32)
        modes = (np.arange(len(rects)) % 3 == 1).astype(np.int32)         # every third item DESCRIBE
        items.append((rects, modes))
    return images, items, thresholds


@functools.lru_cache(maxsize=None)
def mixed_refs():
    """the references of the mixed call: per item four random words"""
    images, items, _ = mixed_case()
    rng = np.random.default_rng(78)
    return [rng.integers(0, 2 ** 64, (len(r), 4), dtype=np.uint64) for r, _ in items]


@functools.lru_cache(maxsize=None)
def mixed_ref(with_refs=True):
    images, items, thr = mixed_case()
    return ref_express(images, items, thr, mixed_refs() if with_refs else None)


MANY_IMAGES = 1024


@functools.lru_cache(maxsize=None)
def many_case():
    """MOVBA_MAX_EXPRESS_IMAGES images of 17 x 17 up to 24 x 40 with 0 to 3 DETECT items each: k_express_counts runs four
    workgroups.  An image without items is None (a NULL pointer): the first, the last, images 300 to 303 and a sixth of the
    others.  -> (images, items, threshold)"""
    rng = np.random.default_rng(20222)
    images, items = [], []
    for i in range(MANY_IMAGES):
        n = 0 if i in (0, MANY_IMAGES - 1, 300, 301, 302, 303) else int(rng.integers(0, 4)) if rng.random() < 0.8 else 0
        rows_, cols = int(rng.integers(17, 25)), int(rng.integers(17, 41))
        image = edge_image(rng, rows_, cols)
        rects = [random_rects(rng, rows_, cols, SHAPES[int(rng.integers(0, 4))], 1) for _ in range(n)]
        images.append(image if n else None)
        items.append((np.concatenate(rects) if n else np.zeros((0, 4), np.int32), np.zeros(n, np.int32)))
    return images, items, 25


@functools.lru_cache(maxsize=None)
def many_ref():
    return ref_express(*many_case())


def read_pixels(rect, cols):
    """the flat indices of every pixel an accepted item reads: the block, the column to its right, and the centre's four"""
    x0, y0, w, h = (int(v) for v in rect)
    px = {(y0 + y, x0 + x) for y in range(h) for x in range(w + 1)}
    r, c = w // 2, h // 2
    px |= {(y0 + r, x0 + c), (y0 + r - 1, x0 + c - 1), (y0 + r, x0 + c - 1), (y0 + r - 1, x0 + c)}
    return px
