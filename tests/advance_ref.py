"""movba_advance restated from the rules of include/movba.h (what the CPU and GPU tests compare against), twice: literally - a
serial walk in sorted order with a real lbFound list, np.float32 arithmetic and int() truncation, on express_ref's literal block
functions - and vectorised, written independently - stable argsort, minimum position per macroblock, cumulative sums, on
express_ref's numpy block function (tests/test_advance_cpu.py holds the two equal on every case); and the committed cases: the
mixed call, the counts that leave waves partly filled, the bound, the mov_cnt trio, and the three that take the device's own sums
and scans past their first pass (1 024 frames, the bound's frame behind others, 300 macroblocks and 266 lattice rects).
Everything is integer except one fp32 add
and one fp32 subtract per rectangle: every comparison is exact equality.  Helper module: no tests here.

A call is a list of frames as movba.capi.advance_desc takes them: dicts with image, threshold, force_grid, first_id, prev_pt,
prev_mb, prev_age, prev_track, prev_desc, prev_coverage, prev_cand, mv_pt, mv_dindx, kp_rect, grid_covered."""
import functools

import numpy as np

import express_ref as R

ADV_KEPT, ADV_COVERAGE = 1, 2
ADV_NO_MV, ADV_REJ_BOUNDS, ADV_LOST_CLAIM, ADV_FAR = 16, 17, 18, 19
FATES = (ADV_KEPT, ADV_COVERAGE, ADV_NO_MV, ADV_REJ_BOUNDS, ADV_LOST_CLAIM, ADV_FAR)
PER_PREV = ("order", "fate", "chosen_mv", "distance")
PER_KP = ("kp_found", "kp_code")
PER_FRAME = ("mov_cnt", "grid_ran", "next_id")
FEAT = ("feat_src", "feat_track", "feat_pt", "feat_rect", "feat_age", "feat_desc")
KEYS = PER_PREV + PER_KP + PER_FRAME + ("seg_ptr",) + FEAT


def popcount(v: int) -> int:
    return bin(v).count("1")


def lattice(rows, cols):
    """the rects of extract_moves, in its order"""
    return [(x - 8, y - 8, 16, 16) for y in range(8, rows - 8, 16) for x in range(8, cols - 8, 16)]


def shape_of(fr):
    return (1, 1) if fr["image"] is None else fr["image"].shape


def rect_of(pt, mv, w, h):
    """-> (pt + mv in fp32, the cv::Rect): one fp32 add per component, w / 2 the integer quotient, the subtraction in fp32, the
    conversion truncating toward zero"""
    qx = np.float32(pt[0]) + np.float32(mv[0])
    qy = np.float32(pt[1]) + np.float32(mv[1])
    x = int(np.float32(qx - np.float32(w // 2)))
    y = int(np.float32(qy - np.float32(h // 2)))
    return (qx, qy), (x, y, int(w), int(h))


# ---- the literal restatement ------------------------------------------------------------------------------------------------

def literal_frame(fr):
    """MOVExtractor.cc:245-335, :380-451 on one frame -> dict(order, fate, chosen_mv, distance, kp_found, kp_code, mov_cnt,
    grid_ran, next_id, kept, new, grid: lists of (src, track, (ptx, pty), rect, age, desc as an int))"""
    image, thr = fr["image"], int(fr["threshold"])
    rows, cols = shape_of(fr)
    n, nk = len(fr["prev_age"]), len(fr["kp_rect"])
    descs = [R.as_int(w) for w in np.asarray(fr["prev_desc"], np.uint64).reshape(-1, 4)]
    age = [int(a) for a in fr["prev_age"]]
    # sort: age descending, then count descending; Python's sort is stable, so ties stand in ascending input index
    order = sorted(range(n), key=lambda i: (-age[i], -popcount(descs[i])))
    fate, chosen, distance = [0] * n, [-1] * n, [-1] * n
    lbFound = [False] * nk
    kept = []
    for i, idx in enumerate(order):
        if fr["prev_coverage"][idx]:
            fate[idx] = ADV_COVERAGE
            continue
        cand = [int(c) for c in fr["prev_cand"][idx]]
        if cand[0] == -1:
            fate[idx] = ADV_NO_MV
            continue
        w, h = (int(v) for v in fr["prev_mb"][idx])
        pt = fr["prev_pt"][idx]
        indx = cand[0]
        if cand[1] >= 0:
            bestDesc = 256
            for j in range(4):
                if cand[j] == -1:
                    break
                _, mb = rect_of(pt, fr["mv_pt"][cand[j]], w, h)
                if R.rejected(mb, rows, cols) == 0:
                    dist = popcount(descs[idx] ^ R.compute_descriptor(R.Block(image, mb), thr))
                    if dist < bestDesc:
                        bestDesc = dist
                        indx = cand[j]
        q, mb = rect_of(pt, fr["mv_pt"][indx], w, h)
        d = int(fr["mv_dindx"][indx])
        chosen[idx] = indx
        if R.rejected(mb, rows, cols) != 0:
            fate[idx] = ADV_REJ_BOUNDS
            continue
        desc = R.compute_descriptor(R.Block(image, mb), thr)
        distance[idx] = popcount(descs[idx] ^ desc)
        if d >= 0 and lbFound[d]:
            fate[idx] = ADV_LOST_CLAIM
            continue
        if d >= 0:
            lbFound[d] = True
        if distance[idx] <= 40:
            fate[idx] = ADV_KEPT
            kept.append((i, int(fr["prev_track"][idx]), q, mb, age[idx] + 1, desc))
        else:
            fate[idx] = ADV_FAR
    current = int(fr["first_id"])
    kp_code, new = [0] * nk, []
    for m in range(nk):
        if lbFound[m]:
            continue
        mb = tuple(int(v) for v in fr["kp_rect"][m])
        code, desc, _, _, _ = R.literal_item(image, mb, R.EX_DETECT, thr)
        kp_code[m] = code
        if code == R.EX_FEATURE:
            current += 1
            new.append((m, current, (np.float32(mb[0] + mb[2] // 2), np.float32(mb[1] + mb[3] // 2)), mb, 0, desc))
    mov_cnt = len(new)
    grid_ran = bool(fr["force_grid"]) or mov_cnt < 60
    grid = []
    if grid_ran:
        covered = fr.get("grid_covered")
        for g, mb in enumerate(lattice(rows, cols)):
            code, desc, _, _, _ = R.literal_item(image, mb, R.EX_DETECT, thr)
            if code != R.EX_FEATURE or (covered is not None and covered[g]):
                continue
            current += 1
            grid.append((g, current, (np.float32(mb[0] + 8), np.float32(mb[1] + 8)), mb, 0, desc))
    return dict(order=order, fate=fate, chosen_mv=chosen, distance=distance, kp_found=[int(v) for v in lbFound], kp_code=kp_code,
                mov_cnt=mov_cnt, grid_ran=int(grid_ran), next_id=current, kept=kept, new=new, grid=grid)


# ---- the same, vectorised ---------------------------------------------------------------------------------------------------

def fast_frame(fr):
    image, thr = fr["image"], int(fr["threshold"])
    rows, cols = shape_of(fr)
    n, nk = len(fr["prev_age"]), len(fr["kp_rect"])
    words = np.asarray(fr["prev_desc"], np.uint64).reshape(-1, 4)
    descs = [R.as_int(w) for w in words]
    count = np.array([popcount(v) for v in descs], np.int64)
    age = np.asarray(fr["prev_age"], np.int64).reshape(-1)
    order = np.lexsort((np.arange(n), -count, -age)) if n else np.zeros(0, np.int64)
    position = np.empty(n, np.int64)
    position[order] = np.arange(n)
    cache = {}

    def describe(mb):
        """the descriptor of an in-bounds rect, or None"""
        if mb not in cache:
            code, desc, _, _, _ = R.fast_item(image, mb, R.EX_DESCRIBE, thr)
            cache[mb] = desc if code == R.EX_DESCRIBED else None
        return cache[mb]

    pt = np.asarray(fr["prev_pt"], np.float32).reshape(-1, 2)
    mvp = np.asarray(fr["mv_pt"], np.float32).reshape(-1, 2)
    mb_wh = np.asarray(fr["prev_mb"], np.int32).reshape(-1, 2)
    cand = np.asarray(fr["prev_cand"], np.int32).reshape(-1, 4)
    half = (mb_wh // 2).astype(np.float32)
    fate, chosen, distance = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    final = {}
    cov = np.asarray(fr["prev_coverage"]).reshape(-1) != 0
    fate[cov] = ADV_COVERAGE
    fate[~cov & (cand[:, 0] == -1)] = ADV_NO_MV
    for idx in np.flatnonzero(fate == 0):
        c = cand[idx]
        stop = np.flatnonzero(c == -1)
        c = c[:stop[0]] if len(stop) else c
        q = (pt[idx][None, :] + mvp[c]).astype(np.float32)                  # (candidates, 2), fp32
        xy = np.trunc((q - half[idx][None, :]).astype(np.float32)).astype(np.int64)
        mbs = [(int(x), int(y), int(mb_wh[idx, 0]), int(mb_wh[idx, 1])) for x, y in xy]
        pick = 0
        if len(c) > 1:
            dists = np.array([256 if describe(mb) is None else popcount(descs[idx] ^ describe(mb)) for mb in mbs])
            pick = int(np.argmin(dists)) if dists.min() < 256 else 0           # (argmin: the first of equals)
        chosen[idx] = c[pick]
        desc = describe(mbs[pick])
        if desc is None:
            fate[idx] = ADV_REJ_BOUNDS
            continue
        distance[idx] = popcount(descs[idx] ^ desc)
        final[idx] = (tuple(q[pick]), mbs[pick], desc)
    arrives = np.array(sorted(final), np.int64)
    dst = np.asarray(fr["mv_dindx"], np.int64).reshape(-1)[chosen[arrives]] if len(arrives) else np.zeros(0, np.int64)
    holder = np.full(nk, n, np.int64)
    claims = dst >= 0
    np.minimum.at(holder, dst[claims], position[arrives[claims]])
    lost = np.zeros(len(arrives), bool)
    lost[claims] = holder[dst[claims]] != position[arrives[claims]]
    fate[arrives] = np.where(lost, ADV_LOST_CLAIM, np.where(distance[arrives] <= 40, ADV_KEPT, ADV_FAR))
    kept_idx = order[fate[order] == ADV_KEPT] if n else []
    kept = [(int(position[idx]), int(fr["prev_track"][idx]), final[idx][0], final[idx][1], int(age[idx]) + 1, final[idx][2]) for idx in kept_idx]
    found = holder < n
    detect = [R.fast_item(image, tuple(int(v) for v in mb), R.EX_DETECT, thr) if not found[m] else (0, 0) for m, mb in enumerate(fr["kp_rect"])]
    kp_code = np.array([t[0] for t in detect], np.int64).reshape(-1)
    is_new = kp_code == R.EX_FEATURE
    first = int(fr["first_id"])
    ids = first + np.cumsum(is_new)
    new = []
    for m in np.flatnonzero(is_new):
        x, y, w, h = (int(v) for v in fr["kp_rect"][m])
        new.append((int(m), int(ids[m]), (np.float32(x + w // 2), np.float32(y + h // 2)), (x, y, w, h), 0, detect[m][1]))
    mov_cnt = int(is_new.sum())
    grid_ran = bool(fr["force_grid"]) or mov_cnt < 60
    grid = []
    if grid_ran:
        rects = lattice(rows, cols)
        got = [R.fast_item(image, mb, R.EX_DETECT, thr) for mb in rects]
        emit = np.array([t[0] == R.EX_FEATURE for t in got], bool).reshape(-1)
        if fr.get("grid_covered") is not None:
            emit &= np.asarray(fr["grid_covered"]).reshape(-1) == 0
        gid = first + mov_cnt + np.cumsum(emit)
        grid = [(int(g), int(gid[g]), (np.float32(rects[g][0] + 8), np.float32(rects[g][1] + 8)), rects[g], 0, got[g][1]) for g in np.flatnonzero(emit)]
    return dict(order=order.tolist(), fate=fate.tolist(), chosen_mv=chosen.tolist(), distance=distance.tolist(), kp_found=found.astype(int).tolist(),
                kp_code=kp_code.tolist(), mov_cnt=mov_cnt, grid_ran=int(grid_ran), next_id=first + mov_cnt + len(grid), kept=kept, new=new, grid=grid)


# ---- a whole call -----------------------------------------------------------------------------------------------------------

def ref_advance(frames, literal=True):
    """-> the fields of Solver.advance's dict"""
    one = literal_frame if literal else fast_frame
    per = [one(fr) for fr in frames]
    cap = sum(len(fr["prev_age"]) + len(fr["kp_rect"]) + len(lattice(*shape_of(fr))) for fr in frames)

    def cat(key, dtype):
        return np.array([v for p in per for v in p[key]], dtype).reshape(-1)

    out = dict(status=0, order=cat("order", np.int32), fate=cat("fate", np.uint8), chosen_mv=cat("chosen_mv", np.int32),
               distance=cat("distance", np.int32), kp_found=cat("kp_found", np.uint8), kp_code=cat("kp_code", np.uint8),
               mov_cnt=np.array([p["mov_cnt"] for p in per], np.int32), grid_ran=np.array([p["grid_ran"] for p in per], np.uint8),
               next_id=np.array([p["next_id"] for p in per], np.int32))
    seg, rows_ = [], []
    for p in per:
        for part in ("kept", "new", "grid"):
            seg.append(len(rows_))
            rows_ += p[part]
        seg.append(len(rows_))
    seg.append(len(rows_))
    out["seg_ptr"] = np.array(seg, np.int32)
    out["feat_src"] = np.full(cap, -1, np.int32); out["feat_track"] = np.full(cap, -1, np.int32); out["feat_age"] = np.full(cap, -1, np.int32)
    out["feat_pt"] = np.full((cap, 2), np.nan, np.float32); out["feat_rect"] = np.full((cap, 4), -1, np.int32)
    out["feat_desc"] = np.zeros((cap, 4), np.uint64)
    for o, (src, track, pt, mb, age, desc) in enumerate(rows_):
        out["feat_src"][o], out["feat_track"][o], out["feat_age"][o] = src, track, age
        out["feat_pt"][o] = pt
        out["feat_rect"][o] = mb
        out["feat_desc"][o] = R.words(desc)
    out["prev_ptr"] = np.concatenate([[0], np.cumsum([len(fr["prev_age"]) for fr in frames])]).astype(np.int32)
    out["kp_ptr"] = np.concatenate([[0], np.cumsum([len(fr["kp_rect"]) for fr in frames])]).astype(np.int32)
    return out


def compare(got, ref, label=""):
    """every array, padding included (feat_pt bit by bit: the padding is NaN)"""
    for key in KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.dtype == r.dtype and g.shape == r.shape, (label, key, g.dtype, r.dtype, g.shape, r.shape)
        if not r.size:
            continue
        if key == "feat_pt":
            assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key, "padding")
            g, r = g.view(np.uint32), r.view(np.uint32)
            bad = np.flatnonzero(((g != r) & ~np.isnan(np.asarray(ref[key]))).reshape(len(r), -1).any(axis=1))
        else:
            bad = np.flatnonzero((g != r).reshape(len(r), -1).any(axis=1))
        assert not len(bad), (label, key, bad[:8].tolist(), np.asarray(got[key])[bad[:3]].tolist(), np.asarray(ref[key])[bad[:3]].tolist())


def frame_rows(res, f):
    """one frame's share of a result, as tuples that compare: per-feature rows, per-macroblock rows, the counts and the feature list
    with places relative to the frame's start"""
    a, b = int(res["prev_ptr"][f]), int(res["prev_ptr"][f + 1])
    ka, kb = int(res["kp_ptr"][f]), int(res["kp_ptr"][f + 1])
    s = [int(v) for v in res["seg_ptr"][4 * f:4 * f + 4]]
    feats = [(int(res["feat_src"][o]), int(res["feat_track"][o]), tuple(res["feat_pt"][o].view(np.uint32).tolist()), tuple(res["feat_rect"][o].tolist()),
              int(res["feat_age"][o]), tuple(res["feat_desc"][o].tolist())) for o in range(s[0], s[3])]
    return (tuple(tuple(res[k][a:b].tolist()) for k in PER_PREV), tuple(tuple(res[k][ka:kb].tolist()) for k in PER_KP),
            tuple(int(res[k][f]) for k in PER_FRAME), tuple(v - s[0] for v in s), tuple(feats))


# ---- building frames ------------------------------------------------------------------------------------------------------------

def true_desc(image, rect, thr):
    code, desc, _, _, _ = R.fast_item(image, tuple(int(v) for v in rect), R.EX_DESCRIBE, thr)
    assert code == R.EX_DESCRIBED, rect
    return desc


def flipped(desc, nbits, rng):
    """desc with exactly nbits of its 256 bits flipped"""
    for b in rng.choice(256, nbits, replace=False):
        desc ^= 1 << int(b)
    return desc


class Builder:
    """One frame, feature by feature.  feat(dest, ...) places a previous feature so that its candidate `via` lands on the rect
    dest = (x, y, w, h) with the fractional part `frac` left over."""

    def __init__(self, image, threshold=25, first_id=0, force_grid=0):
        self.image, self.threshold, self.first_id, self.force_grid = image, threshold, first_id, force_grid
        self.mvs, self.kps, self.prev = [], [], []
        self.grid_covered = None

    def mv(self, dx, dy, dindx=-1):
        self.mvs.append((np.float32(dx), np.float32(dy), dindx))
        return len(self.mvs) - 1

    def kp(self, rect):
        self.kps.append(tuple(int(v) for v in rect))
        return len(self.kps) - 1

    def feat(self, dest, cand, age, desc, coverage=0, via=0, frac=(0.25, 0.5), track=None):
        x, y, w, h = (int(v) for v in dest)
        cand = list(cand) + [-1] * (4 - len(cand))
        dx, dy = (self.mvs[cand[via]][0], self.mvs[cand[via]][1]) if cand[via] >= 0 else (np.float32(0), np.float32(0))
        pt = (np.float32(x + w // 2 + frac[0]) - dx, np.float32(y + h // 2 + frac[1]) - dy)
        self.prev.append(dict(pt=pt, mb=(w, h), age=age, track=1000 + len(self.prev) if track is None else track, desc=desc, coverage=coverage, cand=cand))
        return len(self.prev) - 1

    def frame(self):
        p = self.prev
        return dict(image=self.image, threshold=self.threshold, force_grid=self.force_grid, first_id=self.first_id,
                    prev_pt=np.array([q["pt"] for q in p], np.float32).reshape(-1, 2), prev_mb=np.array([q["mb"] for q in p], np.int32).reshape(-1, 2),
                    prev_age=np.array([q["age"] for q in p], np.int32), prev_track=np.array([q["track"] for q in p], np.int32),
                    prev_desc=np.array([R.words(q["desc"]) for q in p], np.uint64).reshape(-1, 4),
                    prev_coverage=np.array([q["coverage"] for q in p], np.uint8), prev_cand=np.array([q["cand"] for q in p], np.int32).reshape(-1, 4),
                    mv_pt=np.array([(m[0], m[1]) for m in self.mvs], np.float32).reshape(-1, 2), mv_dindx=np.array([m[2] for m in self.mvs], np.int32),
                    kp_rect=np.array(self.kps, np.int32).reshape(-1, 4), grid_covered=self.grid_covered)


def striped_image(rng, rows, cols):
    """diagonal stripes with noise: edges in every 16 x 16 block"""
    Y, X = np.mgrid[0:rows, 0:cols]
    img = np.where(((X + Y) // 12) % 2 == 0, 60, 190) + rng.integers(-8, 9, (rows, cols))
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def classified(key):
    """every rect of the four shapes on a 2-pixel raster of the image `key` names, by DETECT's code -> (image, {code: [rects]})"""
    rng = np.random.default_rng(31)
    if key == "mixed":
        image = striped_image(rng, 64, 96)
        image[0:22, 0:30] = 128                                          # flat
        image[40:64, 60:96] = R.noise_image(rng, 24, 36)                   # noise
    else:
        image = striped_image(rng, 64, 96)
    by = {}
    for w, h in R.SHAPES:
        for y in range(0, 64 - h, 2):
            for x in range(0, 96 - w, 2):
                by.setdefault((R.fast_item(image, (x, y, w, h), R.EX_DETECT, 25)[0], w, h), []).append((x, y, w, h))
    return image, by


def random_features(b, rng, n, ages=(0, 3, 7), near=0.5):
    """n previous features at random places with 0 - 4 candidates among the builder's vectors; about `near` of them carry the
    descriptor of where their first candidate lands with a few bits flipped, so that KEPT occurs; the rest random words"""
    rows, cols = b.image.shape
    n_mv = len(b.mvs)
    for k in range(n):
        w, h = R.SHAPES[int(rng.integers(4))]
        x, y = int(rng.integers(-2, cols - w + 2)), int(rng.integers(-2, rows - h + 2))         # (some over the border)
        nc = int(rng.integers(0, 5)) if n_mv else 0
        cand = [int(c) for c in rng.integers(0, n_mv, nc)]
        if nc and rng.random() < near and R.rejected((x, y, w, h), rows, cols) == 0:
            desc = flipped(true_desc(b.image, (x, y, w, h), b.threshold), int(rng.integers(0, 60)), rng)
        else:
            desc = R.as_int(rng.integers(0, 2 ** 64, 4, dtype=np.uint64))
        b.feat((x, y, w, h), cand, int(rng.choice(ages)), desc, coverage=int(rng.random() < 0.08), frac=(float(rng.random()), float(rng.random())))


def random_frame(image, rng, n_prev, n_mv=40, n_kps=30, first_id=0, force_grid=0, threshold=25):
    """a frame of random features, vectors of up to 12 pixels whose dindx is -1 or any macroblock, macroblocks of the four shapes
    anywhere (some over the border)"""
    b = Builder(image, threshold, first_id, force_grid)
    rows, cols = image.shape
    for m in range(n_kps):
        w, h = R.SHAPES[m % 4]
        b.kp((int(rng.integers(-2, cols - w + 2)), int(rng.integers(-2, rows - h + 2)), w, h))
    for m in range(n_mv):
        b.mv(float(rng.integers(-48, 49)) / 4, float(rng.integers(-48, 49)) / 4, int(rng.integers(-1, n_kps)) if n_kps else -1)
    random_features(b, rng, n_prev)
    return b.frame()


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The mixed call: frame 0 (64 x 96, first_id 0) is built feature by feature for the conditions tests/test_advance_cpu.py
    asserts; frame 1 (40 x 56, a view into a wider array whose padding is poisoned), frame 2 (no previous features) and frame 3
    (first_id 2^30, force_grid) are random.  -> (frames, notes: what the builder meant, by name -> input indices of frame 0)"""
    rng = np.random.default_rng(2024)
    image, by = classified("mixed")
    thr = 25
    b = Builder(image, thr, first_id=0)
    feats = {s: by[(R.EX_FEATURE, *s)] for s in R.SHAPES}
    pick = lambda s, k: feats[s][(k * 7) % len(feats[s])]
    # macroblocks: 0 - 7 features (two of every shape), 8 over the border, 9 of 4 x 4, 10 flat, 11 without an edge, 12 - 15 others
    for k in range(8):
        b.kp(pick(R.SHAPES[k % 4], k))
    b.kp((90, 10, 8, 8)); b.kp((4, 4, 4, 4)); b.kp(by[(R.EX_REJ_FLAT, 16, 16)][0]); b.kp(by[(R.EX_REJ_NO_EDGE, 8, 8)][0])
    for k in range(4):
        b.kp(pick(R.SHAPES[k], 20 + k))
    notes = {}
    inside = lambda k: tuple(int(v) for v in R.random_rects(rng, 64, 96, R.SHAPES[k % 4], 1)[0])
    near = lambda rect, nbits: flipped(true_desc(image, rect, thr), nbits, rng)

    def note(name, idx):
        notes.setdefault(name, []).append(idx)

    # 1 - 4 candidates, three of each; with more than one the best is j = 1, 2, 0
    for nc in (1, 2, 3, 4):
        for k in range(3):
            dest = inside(nc + k)
            best = 0 if nc == 1 else (1, 2, 0)[k] % nc
            cand = [b.mv(3 + j + k, -2 - j, -1) for j in range(nc)]
            note(f"cand{nc}", b.feat(dest, cand, 9, near(dest, 4 + k), via=best))
            if best:
                note("best_later", notes[f"cand{nc}"][-1])
    # two vectors with the same pt: equal distances, the earlier wins
    for k in range(2):
        dest = inside(k)
        cand = [b.mv(5, 1 + k, -1), b.mv(5, 1 + k, -1)]
        note("equal", b.feat(dest, cand, 8, near(dest, 6)))
    # every candidate out of bounds; one candidate, out of bounds
    for k in range(2):
        note("all_out", b.feat((85, 20 + k, 16, 16), [b.mv(40, 0, -1), b.mv(50, 3, -1)], 8, near((70, 20, 16, 16), 3)))
    note("one_out", b.feat((70, 60, 8, 8), [b.mv(0, 60, -1)], 8, near((70, 30, 8, 8), 3)))
    # truncation: pt - w / 2 = -0.5 -> 0 (kept), = -1.0 -> -1 (rejected)
    free = b.mv(2, 3, -1)
    note("trunc_kept", b.feat((0, 24, 16, 16), [free], 7, near((0, 24, 16, 16), 5), frac=(-0.5, 0.25)))
    note("trunc_kept", b.feat((34, 0, 8, 16), [free], 7, near((34, 0, 8, 16), 5), frac=(0.75, -0.25)))
    note("trunc_out", b.feat((0, 30, 8, 8), [free], 7, near((0, 30, 8, 8), 5), frac=(-1.0, 0.5)))
    # claims.  Macroblock 0: the loser comes first in input order (age 1), the winner later (age 6)
    m0 = b.mv(-4, 2, 0)
    dest = inside(0)
    note("claim0_loser", b.feat(dest, [m0], 1, near(dest, 2)))
    note("claim0_winner", b.feat(dest, [m0], 6, near(dest, 2)))
    # macroblock 1: three features
    m1 = b.mv(1, -5, 1)
    for k, a in enumerate((6, 5, 4)):
        dest = inside(1 + k)
        note("claim1", b.feat(dest, [m1], a, near(dest, 3)))
    # macroblock 2: the winner is FAR
    m2 = b.mv(-2, -2, 2)
    dest = inside(2)
    note("claim2_far", b.feat(dest, [m2], 6, near(dest, 90)))
    note("claim2_loser", b.feat(dest, [m2], 5, near(dest, 1)))
    # macroblock 12: the earlier feature is out of bounds, the later one wins
    m12 = b.mv(30, 0, 12)
    note("claim12_out", b.feat((80, 8, 16, 16), [m12], 6, near((60, 8, 16, 16), 1), frac=(0.5, 0.5)))
    dest = inside(3)
    note("claim12_winner", b.feat(dest, [m12], 5, near(dest, 1)))
    # three features on one vector without a macroblock
    for k in range(3):
        dest = inside(k)
        note("shared_free", b.feat(dest, [free], 4, near(dest, 7)))
    # the gate: exactly 40 and exactly 41
    dest = inside(1)
    note("gate40", b.feat(dest, [free], 3, near(dest, 40)))
    note("gate41", b.feat(dest, [free], 3, near(dest, 41)))
    # ties in the sort: three groups equal in age and count (no vector: NO_MV), and coverage features far apart
    for g, (a, size) in enumerate(((2, 3), (9, 2), (0, 2))):
        desc = R.as_int(rng.integers(0, 2 ** 64, 4, dtype=np.uint64))
        for k in range(size):
            note(f"tie{g}", b.feat(inside(k), [], a, desc))
    note("coverage", b.feat(inside(0), [free], 10, near(inside(0), 0), coverage=1))
    note("coverage", b.feat(inside(1), [], 0, 0, coverage=1))
    # bulk: random features on vectors whose dindx is -1 or one of the macroblocks 13 - 15
    for m in range(12):
        b.mv(float(rng.integers(-40, 41)) / 4, float(rng.integers(-40, 41)) / 4, int(rng.choice([-1, 13, 14, 15])))
    bulk = Builder(image, thr)
    bulk.mvs = b.mvs[-12:]
    random_features(bulk, rng, 30)
    for q in bulk.prev:
        q["cand"] = [c + len(b.mvs) - 12 if c >= 0 else -1 for c in q["cand"]]
        q["track"] = 1000 + len(b.prev)
        b.prev.append(q)
    frames = [b.frame()]
    # frame 1: padded, poisoned rows
    img = R.edge_image(rng, 40, 56)
    wide = np.full((40, 56 + 13), 0xA5, np.uint8)
    wide[:, :56] = img
    frames.append(random_frame(wide[:, :56], rng, 40, first_id=17))
    # frame 2: no previous features; frame 3: a large first_id, the grid forced, some of its lattice covered
    frames.append(random_frame(R.edge_image(rng, 33, 47), rng, 0, n_mv=0, first_id=5))
    fr = random_frame(striped_image(rng, 48, 64), rng, 25, first_id=2 ** 30, force_grid=1, threshold=40)
    fr["grid_covered"] = (np.arange(len(lattice(48, 64))) % 3 == 1).astype(np.uint8)
    frames.append(fr)
    return frames, notes


@functools.lru_cache(maxsize=None)
def mixed_ref():
    return ref_advance(mixed_case()[0])


COUNTS = (0, 1, 63, 64, 65, 257, 1000)


@functools.lru_cache(maxsize=None)
def counts_case():
    """one frame per count of COUNTS over one 64 x 96 image; ages from 3 values, so ties are plentiful"""
    rng = np.random.default_rng(55)
    image = classified("plain")[0]
    return [random_frame(image, rng, n, first_id=100 * k) for k, n in enumerate(COUNTS)]


@functools.lru_cache(maxsize=None)
def counts_ref():
    return ref_advance(counts_case())


@functools.lru_cache(maxsize=None)
def bound_case():
    """one frame with 16384 previous features on a 64 x 96 image: 500 distinct features, repeated with other ages and tracks, so
    that the vectorised restatement's descriptor cache serves most of them"""
    rng = np.random.default_rng(56)
    fr = random_frame(classified("plain")[0], rng, 500, n_mv=60, n_kps=40)
    take = rng.integers(0, 500, 16384)
    for key in ("prev_pt", "prev_mb", "prev_desc", "prev_coverage", "prev_cand"):
        fr[key] = np.ascontiguousarray(fr[key][take])
    fr["prev_age"] = rng.choice([0, 3, 7, 11], 16384).astype(np.int32)
    fr["prev_track"] = np.arange(16384, dtype=np.int32)
    return [fr]


@functools.lru_cache(maxsize=None)
def bound_ref():
    return ref_advance(bound_case(), literal=False)


@functools.lru_cache(maxsize=None)
def bound_head():
    """the literal walk over the features at the first 500 positions of the bound case, handed over in that order (what lies
    behind them cannot change them) -> (their input indices, the literal result of that frame of 500)"""
    fr = bound_case()[0]
    head = bound_ref()["order"][:500]
    part = dict(fr)
    for key in ("prev_pt", "prev_mb", "prev_age", "prev_track", "prev_desc", "prev_coverage", "prev_cand"):
        part[key] = fr[key][head]
    return head, ref_advance([part])


def compare_head(res):
    """a result of the bound case against the literal walk over its first 500 positions"""
    head, lit = bound_head()
    assert lit["order"].tolist() == list(range(500)) and np.array_equal(res["order"][:500], head)
    for key in ("fate", "chosen_mv", "distance"):
        assert np.array_equal(lit[key], res[key][head]), key
    n_kept = int((lit["fate"] == ADV_KEPT).sum())
    assert n_kept >= 1
    for key in FEAT:
        assert np.array_equal(lit[key][:n_kept], res[key][:n_kept]), key


@functools.lru_cache(maxsize=None)
def trio_case():
    """three frames over one image whose macroblock lists are cut from blocks the restatement calls features: mov_cnt 59, 60, and
    60 with force_grid; the lattice of the first and the third has two of its features covered"""
    rng = np.random.default_rng(57)
    image, by = classified("plain")
    blocks = [r for s in R.SHAPES for r in by.get((R.EX_FEATURE, *s), [])]
    blocks = [blocks[int(k)] for k in rng.permutation(len(blocks))[:60]]
    lat = lattice(64, 96)
    is_feature = [R.fast_item(image, mb, R.EX_DETECT, 25)[0] == R.EX_FEATURE for mb in lat]
    covered = np.zeros(len(lat), np.uint8)
    covered[np.flatnonzero(is_feature)[:2]] = 1
    covered[np.flatnonzero(~np.array(is_feature))[:1]] = 1          # (and one that is no feature anyway)
    frames = []
    for n, force, first in ((59, 0, 0), (60, 0, 7), (60, 1, 2 ** 30)):
        b = Builder(image, 25, first, force)
        for mb in blocks[:n]:
            b.kp(mb)
        b.grid_covered = covered.copy()
        frames.append(b.frame())
    return frames


@functools.lru_cache(maxsize=None)
def trio_ref():
    return ref_advance(trio_case())


# ---- the cases for what only the device runs: the sums and scans of k_adv_resolve and k_adv_emit ------------------

N_FRAMES = 1024
FRAMES_ALONE = (0, 85, 86, 255, 256, 1023)
FRAMES_EMPTY = (0, 1, 500, 501, 502, 1022, 1023)


def empty_frame(first_id=0):
    """a frame without an image and without items"""
    z = lambda dtype, *shape: np.zeros((0,) + shape, dtype)
    return dict(image=None, threshold=25, force_grid=0, first_id=first_id, prev_pt=z(np.float32, 2), prev_mb=z(np.int32, 2), prev_age=z(np.int32),
                prev_track=z(np.int32), prev_desc=z(np.uint64, 4), prev_coverage=z(np.uint8), prev_cand=z(np.int32, 4), mv_pt=z(np.float32, 2),
                mv_dindx=z(np.int32), kp_rect=z(np.int32, 4), grid_covered=None)


@functools.lru_cache(maxsize=None)
def frames_case():
    """MOVBA_MAX_EXPRESS_IMAGES frames on images of 17 x 17 up to 33 x 47 with 0 to 4 previous features, 0 to 3 macroblocks and 0 to 3
    vectors each: k_adv_emit's sum over the 3 x 1 024 counts takes 12 passes of its stride of 256 (frame 85's three counts lie on
    both sides of the end of the first pass).  FRAMES_EMPTY have no image and no item."""
    rng = np.random.default_rng(58)
    frames = []
    for f in range(N_FRAMES):
        if f in FRAMES_EMPTY:
            frames.append(empty_frame(first_id=f))
            continue
        low = 1 if f in FRAMES_ALONE else 0
        image = R.edge_image(rng, int(rng.integers(17, 34)), int(rng.integers(17, 48)))
        frames.append(random_frame(image, rng, int(rng.integers(low, 5)), n_mv=int(rng.integers(low, 4)), n_kps=int(rng.integers(low, 4)), first_id=7 * f))
    return frames


@functools.lru_cache(maxsize=None)
def frames_ref():
    return ref_advance(frames_case())


@functools.lru_cache(maxsize=None)
def behind_case():
    """the frame of the bound case behind three frames of a few items: the workgroups of k_adv_emit per frame follow the call's
    AVERAGE frame, so the 16 439 items of the last frame take four passes of the strided loop"""
    rng = np.random.default_rng(59)
    tiny = [random_frame(R.edge_image(rng, 17 + k, 20 + k), rng, 2 + k, n_mv=3, n_kps=2, first_id=10 * k) for k in range(3)]
    return tiny + [bound_case()[0]]


@functools.lru_cache(maxsize=None)
def behind_ref():
    return ref_advance(behind_case(), literal=False)


def emit_chunks(n_items, n_frames):
    """launch_advance's rule for k_adv_emit's workgroups per frame: min(64, ceil(n_items / n_frames / 256)), the quotient an integer's"""
    return min(64, max(1, (n_items // n_frames + 255) // 256))


def frame_part(res, f):
    """frame f of a result as the result of a call of that frame alone would hold it, for the per-feature arrays and the feature list"""
    a, b = int(res["prev_ptr"][f]), int(res["prev_ptr"][f + 1])
    out = {key: res[key][a:b] for key in PER_PREV}
    out.update({key: res[key][int(res["seg_ptr"][4 * f]):int(res["seg_ptr"][4 * f + 3])] for key in FEAT})
    return out


@functools.lru_cache(maxsize=None)
def lattice_case():
    """two frames of 240 x 320 with 300 macroblocks each and the full lattice of 14 x 19 = 266 rects, so that the scans of
    k_adv_resolve over the macroblocks and over the lattice give every thread two entries: the first with force_grid, a tenth of
    its lattice covered; the second without, and with enough new features that its lattice is not emitted"""
    rng = np.random.default_rng(60)
    frames = []
    for f in range(2):
        image = striped_image(rng, 240, 320)
        image[100:140, 0:320] = 128                                     # (a flat band: rects that are no feature in both ranges)
        fr = random_frame(image, rng, 60, n_mv=50, n_kps=300, first_id=1000 * f, force_grid=1 - f)
        fr["grid_covered"] = (rng.random(len(lattice(240, 320))) < 0.1).astype(np.uint8)
        frames.append(fr)
    return frames


@functools.lru_cache(maxsize=None)
def lattice_ref():
    return ref_advance(lattice_case())


def read_pixels(fr):
    """the (y, x) of every pixel the items of a frame read: the blocks of every candidate, macroblock and lattice rect that is in
    bounds"""
    rows, cols = shape_of(fr)
    px = set()
    rects = [tuple(int(v) for v in mb) for mb in fr["kp_rect"]] + lattice(rows, cols)
    for idx in range(len(fr["prev_age"])):
        for c in fr["prev_cand"][idx]:
            if c >= 0:
                rects.append(rect_of(fr["prev_pt"][idx], fr["mv_pt"][c], *fr["prev_mb"][idx])[1])
    for mb in rects:
        if R.rejected(mb, rows, cols) == 0:
            px |= R.read_pixels(mb, cols)
    return px
