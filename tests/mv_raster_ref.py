"""movba_mv_raster restated from the rules of include/movba.h (what the CPU and GPU tests compare against), twice: literally - the
loop of VideoDecoder::NextImage with its float half-sizes, its `continue`, its clamps, the H x W x 4 image cleared to -1, the
inclusive double loop and the four-way slot fill, the fp32 running sum of the coverage, and then the gathers at the queries - and
without any painting, written independently - integer keep test, integer extents, and per query the sorted list of the kept
records that contain the pixel, of which the first three and the last are picked (tests/test_mv_raster_cpu.py holds the two
equal on every case); a third time with numpy - a keep mask, its cumulative sum, the queries broadcast against the extents -
for the frame of 66 600 records that the first two cannot walk in seconds (held equal to both on every small case); and the
committed cases.  Everything is exact: every comparison is equality.  Helper module: no tests here.

A call is a list of frames as movba.capi.mv_raster_desc takes them: dicts with rows, cols, coverage_threshold, want_grid, records
(a dict of src_x, src_y, dst_x, dst_y, w, h and optionally source, ref) and q_pt."""
import functools

import numpy as np

SIZES = (4, 8, 16)
KEYS = ("kept_ptr", "kp_rect", "mv_pt", "mv_dindx", "rec_kept", "cand", "grid_ptr", "grid_covered", "cover_px", "coverage_area", "force_grid")
FIELDS = ("src_x", "src_y", "dst_x", "dst_y", "w", "h")


def lattice(rows, cols):
    """the rects of extract_moves, in its order"""
    return [(x - 8, y - 8, 16, 16) for y in range(8, rows - 8, 16) for x in range(8, cols - 8, 16)]


def records_of(fr):
    """-> the frame's records as a list of (src_x, src_y, dst_x, dst_y, w, h) of Python ints"""
    return list(zip(*[[int(v) for v in np.asarray(fr["records"][k]).reshape(-1)] for k in FIELDS]))


def query_pixels(fr):
    """the pixels (x, y) of the point queries: (int)pt.x, (int)pt.y, truncating toward zero"""
    return [(int(np.float32(x)), int(np.float32(y))) for x, y in np.asarray(fr["q_pt"], np.float32).reshape(-1, 2)]


# ---- (a) the literal restatement ---------------------------------------------------------------------------------------------

def paint(fr):
    """VideoDecoder.cc:198-351 on one frame with ref == 0 and source < 0 -> dict(mvi (H, W, 4), kps, mvs, rec_kept, coverage (the fp32
    sum), coverage_area)"""
    height, width = int(fr["rows"]), int(fr["cols"])
    mvi = np.full((height, width, 4), -1, np.int32)
    kps, mvs, rec_kept = [], [], []
    coverage = np.float32(0)
    for sx, sy, dx, dy, w, h in records_of(fr):
        mb_h, mb_w = np.float32(h), np.float32(w)
        mb_h_half, mb_w_half = mb_h / np.float32(2), mb_w / np.float32(2)
        mv_x, mv_y = np.float32(dx - sx), np.float32(dy - sy)
        dst_x, dst_y = np.float32(dx), np.float32(dy)
        d_x_top = dst_x - mb_w_half
        if d_x_top < 0:
            d_x_top = np.float32(0)
        d_y_top = dst_y - mb_h_half
        if d_y_top < 0:
            d_y_top = np.float32(0)
        if dst_x + mb_w_half >= width or dst_y + mb_h_half >= height:
            rec_kept.append(-1)
            continue
        d_mb = (int(d_x_top), int(d_y_top), int(mb_w), int(mb_h))
        kps.append(d_mb)
        d_indx = len(kps) - 1
        # j = 1: src = dst + mv * 1 * -1
        src_x, src_y = np.float32(dx) + mv_x * np.float32(-1), np.float32(dy) + mv_y * np.float32(-1)
        s_x_top = max(src_x - mb_w_half, np.float32(0))
        s_y_top = max(src_y - mb_h_half, np.float32(0))
        s_x_bottom = src_x + mb_w_half
        if s_x_bottom >= width:
            s_x_bottom = np.float32(width - 1)
        s_y_bottom = src_y + mb_h_half
        if s_y_bottom >= height:
            s_y_bottom = np.float32(height - 1)
        mvs.append((mv_x, mv_y, d_indx))
        s_mb_size = len(mvs) - 1
        rec_kept.append(s_mb_size)
        for y in range(int(s_y_top), int(s_y_bottom) + 1):
            row = mvi[y]
            for x in range(int(s_x_top), int(s_x_bottom) + 1):
                v = row[x]
                if v[0] == -1:
                    v[0] = s_mb_size
                elif v[1] == -1:
                    v[1] = s_mb_size
                elif v[2] == -1:
                    v[2] = s_mb_size
                else:
                    v[3] = s_mb_size
        coverage = np.float32(coverage + np.float32(d_mb[2] * d_mb[3]))
    return dict(mvi=mvi, kps=kps, mvs=mvs, rec_kept=rec_kept, coverage=coverage, coverage_area=float(coverage) / float(width * height))


def literal_frame(fr):
    p = paint(fr)
    height, width = int(fr["rows"]), int(fr["cols"])
    mvi = p["mvi"]
    # a query pixel outside the image: four -1 (the reference reads outside its matrix)
    cand = [mvi[y, x].tolist() if 0 <= x < width and 0 <= y < height else [-1] * 4 for x, y in query_pixels(fr)]
    lat = lattice(height, width)
    covered = [int(bool(fr.get("want_grid", 0)) and mvi[y + 8, x + 8, 0] >= 0) for x, y, _, _ in lat]
    return dict(kp_rect=p["kps"], mv_pt=[(m[0], m[1]) for m in p["mvs"]], mv_dindx=[m[2] for m in p["mvs"]], rec_kept=p["rec_kept"], cand=cand,
                grid_covered=covered, cover_px=int(p["coverage"]), coverage_area=p["coverage_area"],
                force_grid=int(p["coverage_area"] < float(fr["coverage_threshold"])))


# ---- (b) without painting ----------------------------------------------------------------------------------------------------

def kept_records(fr):
    """-> (rec_kept, the kept records) by the integer keep test"""
    H, W = int(fr["rows"]), int(fr["cols"])
    rec_kept, kept = [], []
    for r in records_of(fr):
        if r[2] + r[4] // 2 >= W or r[3] + r[5] // 2 >= H:
            rec_kept.append(-1)
        else:
            rec_kept.append(len(kept))
            kept.append(r)
    return rec_kept, kept


def extent(r, W, H):
    """-> (x0, y0, x1, y1), both ends inclusive; empty when x0 > x1 or y0 > y1"""
    sx, sy, _, _, w, h = r
    return max(sx - w // 2, 0), max(sy - h // 2, 0), min(sx + w // 2, W - 1), min(sy + h // 2, H - 1)


def slots_at(extents, x, y):
    inside = sorted(m for m, (x0, y0, x1, y1) in enumerate(extents) if x0 <= x <= x1 and y0 <= y <= y1)
    return (inside[:3] + [-1] * 3)[:3] + [inside[-1] if len(inside) >= 4 else -1]


def set_frame(fr):
    H, W = int(fr["rows"]), int(fr["cols"])
    rec_kept, kept = kept_records(fr)
    extents = [extent(r, W, H) for r in kept]
    cover = sum(r[4] * r[5] for r in kept)
    area = cover / (W * H)
    cand = [slots_at(extents, x, y) if 0 <= x < W and 0 <= y < H else [-1] * 4 for x, y in query_pixels(fr)]
    covered = [int(slots_at(extents, x + 8, y + 8)[0] >= 0) if fr.get("want_grid", 0) else 0 for x, y, _, _ in lattice(H, W)]
    return dict(kp_rect=[(max(r[2] - r[4] // 2, 0), max(r[3] - r[5] // 2, 0), r[4], r[5]) for r in kept],
                mv_pt=[(float(r[2] - r[0]), float(r[3] - r[1])) for r in kept], mv_dindx=list(range(len(kept))), rec_kept=rec_kept, cand=cand,
                grid_covered=covered, cover_px=cover, coverage_area=area, force_grid=int(area < float(fr["coverage_threshold"])))


# ---- (c) with numpy, for the frames too large for (a) and (b) ----------------------------------------------------------------

def slots_of(x0, y0, x1, y1, px, py, chunk=256):
    """per pixel (px[k], py[k]) the slots from the extents (arrays over the kept records, ascending m): the three smallest m
    whose extent contains it and, from four on, the largest; `chunk` pixels against all extents at a time -> (len(px), 4)"""
    out = np.full((len(px), 4), -1, np.int64)
    if not len(x0):
        return out
    for a in range(0, len(px), chunk):
        x, y = px[a:a + chunk, None], py[a:a + chunk, None]
        inside = (x0[None, :] <= x) & (x <= x1[None, :]) & (y0[None, :] <= y) & (y <= y1[None, :])
        count = inside.sum(axis=1)
        last = inside.shape[1] - 1 - inside[:, ::-1].argmax(axis=1)
        out[a:a + chunk, 3] = np.where(count >= 4, last, -1)
        row = np.arange(len(inside))
        for c in range(3):
            first = inside.argmax(axis=1)           # (the lowest m; 0 where the row is empty, which `hit` tells apart)
            hit = inside[row, first]
            out[a:a + chunk, c] = np.where(hit, first, -1)
            inside[row, first] = False
    return out


def vector_frame(fr):
    H, W = int(fr["rows"]), int(fr["cols"])
    sx, sy, dx, dy, w, h = (np.asarray(fr["records"][k]).reshape(-1).astype(np.int64) for k in FIELDS)
    keep = ~((dx + w // 2 >= W) | (dy + h // 2 >= H))
    rec_kept = np.where(keep, np.cumsum(keep) - 1, -1)
    sx, sy, dx, dy, w, h = (v[keep] for v in (sx, sy, dx, dy, w, h))
    x0, y0, x1, y1 = np.maximum(sx - w // 2, 0), np.maximum(sy - h // 2, 0), np.minimum(sx + w // 2, W - 1), np.minimum(sy + h // 2, H - 1)
    cover = int((w * h).sum())
    area = cover / (W * H)
    q = np.trunc(np.asarray(fr["q_pt"], np.float32).reshape(-1, 2)).astype(np.int64)
    cand = slots_of(x0, y0, x1, y1, q[:, 0], q[:, 1])
    cand[(q[:, 0] < 0) | (q[:, 1] < 0) | (q[:, 0] >= W) | (q[:, 1] >= H)] = -1
    lat = np.array(lattice(H, W), np.int64).reshape(-1, 4)
    covered = (slots_of(x0, y0, x1, y1, lat[:, 0] + 8, lat[:, 1] + 8)[:, 0] >= 0) if fr.get("want_grid", 0) else np.zeros(len(lat), bool)
    return dict(kp_rect=np.stack([np.maximum(dx - w // 2, 0), np.maximum(dy - h // 2, 0), w, h], axis=1), mv_pt=np.stack([dx - sx, dy - sy], axis=1).astype(np.float32),
                mv_dindx=np.arange(len(w)), rec_kept=rec_kept, cand=cand, grid_covered=covered.astype(np.uint8), cover_px=cover, coverage_area=area,
                force_grid=int(area < float(fr["coverage_threshold"])))


# ---- a whole call ------------------------------------------------------------------------------------------------------------

def ref_mv_raster(frames, literal=True, vector=False):
    """-> the fields of Solver.mv_raster's dict; (a) by default, (b) with literal=False, (c) with vector=True"""
    per = [(vector_frame if vector else literal_frame if literal else set_frame)(fr) for fr in frames]
    n_rec = sum(len(p["rec_kept"]) for p in per)

    def ptr(counts):
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

    def cat(key, dtype, width=1):
        parts = [np.asarray(p[key], dtype).reshape((-1, width) if width > 1 else (-1,)) for p in per]
        return np.concatenate(parts) if parts else np.zeros((0, width) if width > 1 else (0,), dtype)

    out = dict(status=0, kept_ptr=ptr([len(p["kp_rect"]) for p in per]), grid_ptr=ptr([len(p["grid_covered"]) for p in per]),
               rec_kept=cat("rec_kept", np.int32), cand=cat("cand", np.int32, 4), grid_covered=cat("grid_covered", np.uint8),
               cover_px=np.array([p["cover_px"] for p in per], np.int32), coverage_area=np.array([p["coverage_area"] for p in per], np.float64),
               force_grid=np.array([p["force_grid"] for p in per], np.uint8))
    total = int(out["kept_ptr"][-1])
    out["kp_rect"] = np.full((n_rec, 4), -1, np.int32); out["mv_pt"] = np.full((n_rec, 2), np.nan, np.float32); out["mv_dindx"] = np.full(n_rec, -1, np.int32)
    out["kp_rect"][:total] = cat("kp_rect", np.int32, 4); out["mv_pt"][:total] = cat("mv_pt", np.float32, 2); out["mv_dindx"][:total] = cat("mv_dindx", np.int32)
    out["rec_ptr"] = ptr([len(p["rec_kept"]) for p in per])
    out["q_ptr"] = ptr([len(p["cand"]) for p in per])
    return out


def compare(got, ref, label=""):
    """every array, padding included (mv_pt and coverage_area bit by bit: mv_pt's padding is NaN)"""
    for key in KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.dtype == r.dtype and g.shape == r.shape, (label, key, g.dtype, r.dtype, g.shape, r.shape)
        if not r.size:
            continue
        if g.dtype.kind == "f":
            g, r = g.view(np.uint32 if g.dtype.itemsize == 4 else np.uint64), r.view(np.uint32 if r.dtype.itemsize == 4 else np.uint64)
            if key == "mv_pt":      # (any NaN is padding)
                assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), (label, key, "padding")
                g, r = np.where(np.isnan(ref[key]), 0, g), np.where(np.isnan(ref[key]), 0, r)
        bad = np.flatnonzero((g != r).reshape(len(r), -1).any(axis=1))
        assert not len(bad), (label, key, bad[:8].tolist(), np.asarray(got[key])[bad[:3]].tolist(), np.asarray(ref[key])[bad[:3]].tolist())


def frame_rows(res, f):
    """one frame's share of a result, as tuples that compare"""
    a, b = int(res["rec_ptr"][f]), int(res["rec_ptr"][f + 1])
    k0, k1 = int(res["kept_ptr"][f]), int(res["kept_ptr"][f + 1])
    q0, q1 = int(res["q_ptr"][f]), int(res["q_ptr"][f + 1])
    g0, g1 = int(res["grid_ptr"][f]), int(res["grid_ptr"][f + 1])
    return (tuple(res["rec_kept"][a:b].tolist()), tuple(map(tuple, res["kp_rect"][k0:k1].tolist())), tuple(map(tuple, res["mv_pt"][k0:k1].view(np.uint32).tolist())),
            tuple(res["mv_dindx"][k0:k1].tolist()), tuple(map(tuple, res["cand"][q0:q1].tolist())), tuple(res["grid_covered"][g0:g1].tolist()),
            int(res["cover_px"][f]), float(res["coverage_area"][f]).hex(), int(res["force_grid"][f]))


# ---- building frames ---------------------------------------------------------------------------------------------------------

def frame(rows, cols, recs, q_pt=(), threshold=0.5, want_grid=0):
    """recs: a list of (src_x, src_y, dst_x, dst_y, w, h)"""
    a = np.array(recs, np.int64).reshape(-1, 6)
    records = dict(src_x=a[:, 0].astype(np.int16), src_y=a[:, 1].astype(np.int16), dst_x=a[:, 2].astype(np.int16), dst_y=a[:, 3].astype(np.int16),
                   w=a[:, 4].astype(np.uint8), h=a[:, 5].astype(np.uint8))
    return dict(rows=rows, cols=cols, coverage_threshold=threshold, want_grid=want_grid, records=records, q_pt=np.array(q_pt, np.float32).reshape(-1, 2))


def every_pixel(rows, cols):
    """one query per pixel, row by row, at the pixel's centre"""
    Y, X = np.mgrid[0:rows, 0:cols]
    return np.stack([X.reshape(-1) + 0.5, Y.reshape(-1) + 0.5], axis=1).astype(np.float32)


def random_records(rng, rows, cols, n, margin=24):
    """n records of any size pair whose sources and destinations reach `margin` pixels over every border"""
    return [(int(rng.integers(-margin, cols + margin)), int(rng.integers(-margin, rows + margin)), int(rng.integers(-6, cols + 6)),
             int(rng.integers(-6, rows + 6)), int(rng.choice(SIZES)), int(rng.choice(SIZES))) for _ in range(n)]


def named_records(rows, cols):
    """the records the full-raster test asks for by name, on a rows x cols frame -> {name: record}"""
    W, H = cols, rows
    named = {
        "extent from tile offset 15": (23, 20, 20, 20, 16, 16),             # x: 15 .. 31
        "extent from tile offset 0": (24, 24, 20, 20, 16, 16),              # x: 16 .. 32, y: 16 .. 32
        "extent from tile offset 15 in y": (10, 23, 12, 12, 8, 16),         # y: 15 .. 31
        "source left of the frame": (-20, 10, 10, 10, 16, 16),
        "source right of the frame": (W + 20, 10, 10, 10, 16, 16),
        "source above the frame": (10, -20, 10, 10, 8, 8),
        "source below the frame": (10, H + 20, 10, 10, 8, 8),
        "source clipped at 0": (3, 2, 12, 12, 16, 16),
        "source clipped at W - 1": (W - 2, 12, 12, 12, 16, 8),
        "source clipped at H - 1": (12, H - 1, 12, 12, 8, 16),
        "dst_x + hx == W": (20, 20, W - 8, 20, 16, 16),
        "dst_x + hx == W - 1": (20, 20, W - 9, 20, 16, 16),
        "dst_y + hy == H": (20, 20, 20, H - 4, 8, 8),
        "dst_y + hy == H - 1": (20, 20, 20, H - 5, 8, 8),
        "destination whose top clamps to 0": (20, 20, 20, 2, 16, 16),
        "destination whose left clamps to 0": (20, 20, 1, 20, 8, 8),
    }
    for w in SIZES:
        for h in SIZES:
            named[f"size {w} x {h}"] = (17 + w, 11 + h, 14 + w, 13 + h, w, h)
    return named


@functools.lru_cache(maxsize=None)
def full_case():
    """48 x 40 and, transposed, 40 x 48 - together a partial tile column and a partial tile row - with the named records among
    some 300 random ones each, every pixel queried, the lattice too"""
    rng = np.random.default_rng(11)
    frames = []
    for rows, cols in ((48, 40), (40, 48)):
        recs = random_records(rng, rows, cols, 280)
        for k, r in enumerate(named_records(rows, cols).values()):
            recs.insert(7 + 11 * k, r)
        frames.append(frame(rows, cols, recs, every_pixel(rows, cols), threshold=0.5, want_grid=1))
    return frames


@functools.lru_cache(maxsize=None)
def full_ref():
    return ref_mv_raster(full_case())


PILE = (3, 4, 5, 70)
PILE_PIXEL = (21, 18)


@functools.lru_cache(maxsize=None)
def pile_case():
    """one 40 x 56 frame per count of PILE: that many records cover PILE_PIXEL, with records whose extent is empty and skipped
    records between them (so the dense indices differ from the positions and from each other's neighbours); every pixel queried"""
    rng = np.random.default_rng(12)
    frames = []
    for k in PILE:
        recs = []
        for i in range(k):
            w, h = int(rng.choice(SIZES)), int(rng.choice(SIZES))
            sx, sy = PILE_PIXEL[0] + int(rng.integers(-(w // 2), w // 2 + 1)), PILE_PIXEL[1] + int(rng.integers(-(h // 2), h // 2 + 1))
            recs.append((sx, sy, int(rng.integers(8, 40)), int(rng.integers(8, 30)), w, h))
            recs.append((-20, 10, 12, 12, 16, 16))                      # empty extent, kept
            if i % 2:
                recs.append((10, 10, 56, 10, 8, 8))                     # skipped
        frames.append(frame(40, 56, recs, every_pixel(40, 56), threshold=0.25))
    return frames


@functools.lru_cache(maxsize=None)
def pile_ref():
    return ref_mv_raster(pile_case())


COUNTS = (1, 63, 64, 65, 257, 2500)
QUERY_COUNTS = (0, 1, 65, 65, 1, 65)


@functools.lru_cache(maxsize=None)
def counts_case():
    """record counts that leave wavefronts partly filled and, at 2500 with every third record skipped, take the dense index over
    the chunks of the walk; 0, 1 and 65 queries"""
    rng = np.random.default_rng(13)
    frames = []
    for n, nq in zip(COUNTS, QUERY_COUNTS):
        recs = random_records(rng, 64, 96, n, margin=10) if n > 1 else [(10, 10, 20, 20, 16, 16)]
        if n == 2500:
            recs = [(r[0], r[1], 96 if i % 3 == 2 else min(max(r[2], 0), 80), min(max(r[3], 0), 50), r[4], r[5]) for i, r in enumerate(recs)]
        q = np.stack([rng.uniform(0, 96, nq), rng.uniform(0, 64, nq)], axis=1)
        frames.append(frame(64, 96, recs, q, threshold=float(rng.uniform(0.2, 3.0)), want_grid=n % 2))
    return frames


@functools.lru_cache(maxsize=None)
def counts_ref():
    return ref_mv_raster(counts_case())


@functools.lru_cache(maxsize=None)
def mixed_case():
    """five frames of different sizes: records, queries and the lattice; an I-frame - no records - with both; records without
    queries on a frame too low for a lattice; the lattice alone; and a small frame of odd size"""
    rng = np.random.default_rng(14)

    def q(rows, cols, n):
        return np.stack([rng.uniform(-3, cols + 3, n), rng.uniform(-3, rows + 3, n)], axis=1)

    return [frame(50, 70, random_records(rng, 50, 70, 120), q(50, 70, 90), threshold=0.9, want_grid=1),
            frame(36, 52, [], q(36, 52, 20), threshold=1e-300, want_grid=1),
            frame(16, 75, random_records(rng, 16, 75, 40), [], threshold=0.1, want_grid=0),
            frame(64, 96, random_records(rng, 64, 96, 200), [], threshold=2.0, want_grid=1),
            frame(19, 33, random_records(rng, 19, 33, 30), q(19, 33, 33), threshold=0.4, want_grid=0)]


@functools.lru_cache(maxsize=None)
def mixed_ref():
    return ref_mv_raster(mixed_case())


def gate_case(threshold):
    """a 64 x 64 frame covered by exactly 2048 pixels: coverage_area is exactly 0.5"""
    recs = [(8 + 16 * k, 8, 8 + 12 * (k % 4), 8 + 16 * (k // 4), 16, 16) for k in range(8)]
    return [frame(64, 64, recs, [(5.0, 5.0)], threshold=threshold, want_grid=1)]


def edge_case():
    """queries on and over the edge of a 30 x 44 frame whose corner pixels are covered"""
    W, H = 44, 30
    recs = [(4, 4, 10, 10, 8, 8), (W - 3, 3, 12, 12, 8, 8), (3, H - 3, 12, 12, 8, 8), (2, 2, 14, 14, 16, 16)]
    q = [(-0.5, -0.5), (W, 0), (0, H), (W - 0.5, 0.25), (0.75, H - 0.5), (-1.0, 0), (0, -1.0), (-0.99, -0.99), (W + 5.0, H + 5.0), (-1048576.0, 1048576.0)]
    return [frame(H, W, recs, q)]


# ---- the cases for what only the device runs: the scans over chunks, frames and tiles ----------------------------

CHUNKS_SHAPE, CHUNKS_RECORDS, CHUNKS_QUERIES = (528, 544), 66600, 2000
CHUNKS_BAND = 480               # no source extent reaches a row from here on


@functools.lru_cache(maxsize=None)
def chunks_case():
    """one frame of 528 x 544 - 33 x 34 = 1 122 tiles, two per thread of the tile scan and none from thread 561 on - with 66 600
    records: 66 chunks of 1 024, 40 records in the last, so the carry of chunks 64 and 65 sums over two wavefronts.  About 3 % of the
    records are skipped, the last but one among them; no source reaches the rows from CHUNKS_BAND on, so the tiles there are
    empty and a query there has no record; 2 000 queries, some outside the frame; the lattice is wanted."""
    rng = np.random.default_rng(15)
    rows, cols = CHUNKS_SHAPE
    n = CHUNKS_RECORDS
    recs = np.stack([rng.integers(-24, cols + 24, n), rng.integers(-24, CHUNKS_BAND - 10, n), rng.integers(-6, cols + 6, n), rng.integers(-6, rows + 6, n),
                     rng.choice(SIZES, n), rng.choice(SIZES, n)], axis=1)
    recs[n - 2] = (100, 100, cols, 100, 8, 8)               # skipped
    recs[n - 1] = (100, 100, 100, 100, 16, 16)              # kept
    q = np.stack([rng.uniform(-3, cols + 3, CHUNKS_QUERIES), rng.uniform(-3, rows + 3, CHUNKS_QUERIES)], axis=1)
    return [frame(rows, cols, recs, q, threshold=19.0, want_grid=1)]


@functools.lru_cache(maxsize=None)
def chunks_ref():
    return ref_mv_raster(chunks_case(), vector=True)


@functools.lru_cache(maxsize=None)
def chunks_head():
    """what (a) and (b) say about the part of the chunks case they can walk: the records of the first chunk painted alone (their
    rows do not depend on what follows them), and every 20th query against the sets of (b) over all records
    -> (the literal result of the first 1 024 records, the queries taken, their slots)"""
    fr = chunks_case()[0]
    first = dict(fr, records={k: v[:1024] for k, v in fr["records"].items()}, q_pt=np.zeros((0, 2), np.float32), want_grid=0)
    taken = np.arange(0, CHUNKS_QUERIES, 20)
    _, kept = kept_records(fr)
    extents = [extent(r, fr["cols"], fr["rows"]) for r in kept]
    pixels = query_pixels(fr)
    slots = [slots_at(extents, *pixels[j]) if 0 <= pixels[j][0] < fr["cols"] and 0 <= pixels[j][1] < fr["rows"] else [-1] * 4 for j in taken]
    return ref_mv_raster([first]), taken, np.array(slots, np.int32)


def compare_head(res):
    """a result of the chunks case against chunks_head"""
    lit, taken, slots = chunks_head()
    k = int(lit["kept_ptr"][1])
    assert 0 < k < 1024 and np.array_equal(res["rec_kept"][:1024], lit["rec_kept"])
    assert np.array_equal(res["kp_rect"][:k], lit["kp_rect"][:k]) and np.array_equal(res["mv_dindx"][:k], lit["mv_dindx"][:k])
    assert np.array_equal(res["mv_pt"][:k].view(np.uint32), lit["mv_pt"][:k].view(np.uint32))
    assert np.array_equal(res["cand"][taken], slots), np.flatnonzero((res["cand"][taken] != slots).any(axis=1))[:8].tolist()


MULTIPLES = (1024, 2048, 1025)


@functools.lru_cache(maxsize=None)
def multiples_case():
    """three frames of 1 024, 2 048 and 1 025 records on 64 x 96 images: a last chunk that is full, and a chunk number at which
    the frame has exactly no record left.  Every fifth record is skipped; the last record of the first two frames is kept, the
    last of the third - a chunk of its own - is skipped."""
    rng = np.random.default_rng(16)
    frames = []
    for n in MULTIPLES:
        recs = random_records(rng, 64, 96, n, margin=10)
        recs = [(r[0], r[1], 96 if i % 5 == 3 else min(max(r[2], 0), 80), min(max(r[3], 0), 50), r[4], r[5]) for i, r in enumerate(recs)]
        recs[-1] = (10, 10, 96, 20, 8, 8) if n == 1025 else (10, 10, 20, 20, 16, 16)
        q = np.stack([rng.uniform(0, 96, 65), rng.uniform(0, 64, 65)], axis=1)
        frames.append(frame(64, 96, recs, q, threshold=float(rng.uniform(0.2, 30.0)), want_grid=1))
    return frames


@functools.lru_cache(maxsize=None)
def multiples_ref():
    return ref_mv_raster(multiples_case())


N_FRAMES = 1024
FRAMES_ALONE = (0, 63, 64, 65, 511, 1023)
FRAMES_NO_RECORDS = (0, 1, 2, 400, 401, 402, 403, 404, 1021, 1022, 1023)
FRAMES_NO_QUERIES = (0, 1, 700, 701, 702, 703, 1022, 1023)


@functools.lru_cache(maxsize=None)
def frames_case():
    """MOVBA_MAX_EXPRESS_IMAGES frames of 16 x 16 up to 40 x 40 with 0 to 5 records and 0 to 3 queries each: the scan over the frames'
    kept counts takes all 16 wavefronts, the tile scan (more than 1 024 tiles) crosses frames, and the searches over rec_ptr, q_ptr
    and g_ptr meet runs of equal entries - frames without records (FRAMES_NO_RECORDS), without queries (FRAMES_NO_QUERIES) and,
    at 16 pixels, without a lattice."""
    rng = np.random.default_rng(17)
    frames = []
    for f in range(N_FRAMES):
        rows, cols = int(rng.integers(16, 41)), int(rng.integers(16, 41))
        n = 0 if f in FRAMES_NO_RECORDS else int(rng.integers(1 if f in FRAMES_ALONE else 0, 6))
        nq = 0 if f in FRAMES_NO_QUERIES else int(rng.integers(1 if f in FRAMES_ALONE else 0, 4))
        q = np.stack([rng.uniform(-1, cols + 1, nq), rng.uniform(-1, rows + 1, nq)], axis=1)
        frames.append(frame(rows, cols, random_records(rng, rows, cols, n, margin=8), q, threshold=float(rng.uniform(0.0, 1.0)), want_grid=int(rng.integers(0, 2))))
    return frames


@functools.lru_cache(maxsize=None)
def frames_ref():
    return ref_mv_raster(frames_case())
