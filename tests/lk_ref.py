"""movba_lk_track restated twice, independently of the library and of each other, and the cases the tests run.

`ref_lk(frames, ...)` is numpy over integer arrays: a level's Scharr images are formed once and padded with the constant 0, the
level's pixels are padded by reflection, the windows of all points of a frame are gathered at once and iterated under a mask.
`ref_lk_literal(frame, ..., which)` is loops: one point, one window entry, one pixel at a time, Python integers and np.float32
scalars, the reflected read and the derivative computed where they are used.  The first is what the GPU tests compare against on
every case; the second walks every point of the small cases and every k-th point of the large ones, and tests/test_lk_cpu.py
holds the two equal there (and the pyramids equal pixel by pixel).

The rules are those of include/movba.h [opencv-upstream]: OpenCV's source is not available here, the header's restatement is the
contract.  test_lk_cpu.py checks the restatement once against ground truth that does not come from it (shift_truth_case)."""
import functools

import numpy as np

F = np.float32
FLT_EPSILON = F(1.1920928955078125e-07)
EPS, OSCILLATION, MAX_ITER_RAN, REJ_START, REJ_MIN_EIG, REJ_LOOP = 1, 2, 3, 16, 17, 18
LEVEL_START, LEVEL_MIN_EIG = REJ_START, REJ_MIN_EIG       # level_exit, per level: why that level ended (diagnostics)
PARAMS = dict(max_level=3, max_iter=20, eps=0.01, min_eig_threshold=1e-4)
KEYS = ("next_pt", "pt_status", "err", "exit_code", "keep", "kept_ptr", "kept_src")


def level_sizes(rows, cols, win, max_level):
    """[(rows, cols)] of levels 0 .. L"""
    sizes = [(rows, cols)]
    for _ in range(max_level):
        r, c = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if r <= win or c <= win:
            break
        sizes.append((r, c))
    return sizes


# ---- numpy ---------------------------------------------------------------------------------------------------------------------

def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img):
    h, w = img.shape
    src = img.astype(np.int64)
    k = (1, 4, 6, 4, 1)
    xs = _reflect(2 * np.arange((w + 1) // 2)[:, None] + np.arange(-2, 3)[None, :], w)
    ys = _reflect(2 * np.arange((h + 1) // 2)[:, None] + np.arange(-2, 3)[None, :], h)
    across = sum(k[i] * src[:, xs[:, i]] for i in range(5))
    both = sum(k[j] * across[ys[:, j], :] for j in range(5))
    return ((both + 128) >> 8).astype(np.uint8)


def pyramid(img, win, max_level):
    levels = [np.ascontiguousarray(img)]
    for size in level_sizes(img.shape[0], img.shape[1], win, max_level)[1:]:
        levels.append(pyr_down(levels[-1]))
        assert levels[-1].shape == size
    return levels


def scharr(img):
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    dx = 3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])
    dy = 3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])
    return dx, dy


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    one = F(1)
    w00 = np.rint(((one - a) * (one - b)) * F(16384)).astype(np.int64)
    w01 = np.rint((a * (one - b)) * F(16384)).astype(np.int64)
    w10 = np.rint(((one - a) * b) * F(16384)).astype(np.int64)
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _blend(pad, Y, X, w, n):
    w00, w01, w10, w11 = (v[:, None] for v in w)
    return _descale(pad[Y, X] * w00 + pad[Y, X + 1] * w01 + pad[Y + 1, X] * w10 + pad[Y + 1, X + 1] * w11, n)


def _scaled(s):
    return (s.astype(np.float64) * 2.0 ** -20).astype(F)


def _inside(fx, fy, win, w, h):
    return (fx >= -win) & (fx < w) & (fy >= -win) & (fy < h)


def track_frame(prev, nxt, win, pts, max_level=3, max_iter=20, eps=0.01, min_eig_threshold=1e-4):
    """one frame -> dict(next_pt, pt_status, err, exit_code, keep, level_exit (n, 4))"""
    pts = np.asarray(pts, F).reshape(-1, 2)
    N = len(pts)
    I_pyr, J_pyr = pyramid(prev, win, max_level), pyramid(nxt, win, max_level)
    L = len(I_pyr) - 1
    half = F((win - 1) * 0.5)
    eps_sq = float(eps) * float(eps)
    nx, ny = np.zeros(N, F), np.zeros(N, F)
    status, err, code = np.ones(N, np.uint8), np.zeros(N, F), np.zeros(N, np.uint8)
    level_exit = np.zeros((N, 4), np.uint8)
    oy, ox = np.divmod(np.arange(win * win), win)
    for l in range(L, -1, -1):
        h, w = I_pyr[l].shape
        Ipad = np.pad(I_pyr[l].astype(np.int64), win, mode="reflect")
        Jpad = np.pad(J_pyr[l].astype(np.int64), win, mode="reflect")
        dx_img, dy_img = scharr(I_pyr[l])
        Xpad, Ypad = np.pad(dx_img, win), np.pad(dy_img, win)
        s = F(1.0 / (1 << l))
        qx, qy = pts[:, 0] * s, pts[:, 1] * s
        if l == L:
            nx, ny = qx.copy(), qy.copy()
        else:
            nx, ny = nx * F(2), ny * F(2)
        ux, uy = qx - half, qy - half
        fx, fy = np.floor(ux), np.floor(uy)
        inside = _inside(fx, fy, win, w, h)
        level_exit[~inside, l] = LEVEL_START
        if l == 0:
            status[~inside], err[~inside], code[~inside] = 0, 0, REJ_START
        act = np.nonzero(inside)[0]
        if not len(act):
            continue
        ix, iy = fx[act].astype(np.int64), fy[act].astype(np.int64)
        wts = _weights(ux[act] - fx[act], uy[act] - fy[act])
        Y, X = iy[:, None] + oy[None, :] + win, ix[:, None] + ox[None, :] + win
        Iw, Ixw, Iyw = _blend(Ipad, Y, X, wts, 9), _blend(Xpad, Y, X, wts, 14), _blend(Ypad, Y, X, wts, 14)
        A11, A12, A22 = _scaled((Ixw * Ixw).sum(1)), _scaled((Ixw * Iyw).sum(1)), _scaled((Iyw * Iyw).sum(1))
        D = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / F(2 * win * win)
        assert min_eig.dtype == F and D.dtype == F
        err[act] = min_eig
        bad = (min_eig.astype(np.float64) < min_eig_threshold) | (D < FLT_EPSILON)
        level_exit[act[bad], l] = LEVEL_MIN_EIG
        if l == 0:
            status[act[bad]], code[act[bad]] = 0, REJ_MIN_EIG
        sel = ~bad
        go = act[sel]
        if not len(go):
            continue
        Iw, Ixw, Iyw, A11, A12, A22 = Iw[sel], Ixw[sel], Iyw[sel], A11[sel], A12[sel], A22[sel]
        Dinv = F(1) / D[sel]
        cx, cy = nx[go] - half, ny[go] - half
        pdx, pdy = np.zeros(len(go), F), np.zeros(len(go), F)
        why = np.full(len(go), MAX_ITER_RAN, np.uint8)
        alive = np.ones(len(go), bool)
        for j in range(max_iter):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            gx, gy = np.floor(cx[idx]), np.floor(cy[idx])
            ins = _inside(gx, gy, win, w, h)
            gone = idx[~ins]
            why[gone], alive[gone] = REJ_LOOP, False
            if l == 0:
                status[go[gone]] = 0
            idx, gx, gy = idx[ins], gx[ins], gy[ins]
            if not len(idx):
                break
            v = _weights(cx[idx] - gx, cy[idx] - gy)
            Y, X = gy.astype(np.int64)[:, None] + oy[None, :] + win, gx.astype(np.int64)[:, None] + ox[None, :] + win
            diff = _blend(Jpad, Y, X, v, 9) - Iw[idx]
            B1, B2 = _scaled((diff * Ixw[idx]).sum(1)), _scaled((diff * Iyw[idx]).sum(1))
            dx = (A12[idx] * B2 - A22[idx] * B1) * Dinv[idx]
            dy = (A12[idx] * B1 - A11[idx] * B2) * Dinv[idx]
            assert dx.dtype == F
            cx[idx], cy[idx] = cx[idx] + dx, cy[idx] + dy
            nx[go[idx]], ny[go[idx]] = cx[idx] + half, cy[idx] + half
            d64x, d64y = dx.astype(np.float64), dy.astype(np.float64)
            small = d64x * d64x + d64y * d64y <= eps_sq
            why[idx[small]], alive[idx[small]] = EPS, False
            osc = ~small & (j > 0) & (np.abs((dx + pdx[idx]).astype(np.float64)) < 0.01) & (np.abs((dy + pdy[idx]).astype(np.float64)) < 0.01)
            nx[go[idx[osc]]] = nx[go[idx[osc]]] - dx[osc] * F(0.5)
            ny[go[idx[osc]]] = ny[go[idx[osc]]] - dy[osc] * F(0.5)
            why[idx[osc]], alive[idx[osc]] = OSCILLATION, False
            pdx[idx], pdy[idx] = dx, dy
        level_exit[go, l] = why
        if l == 0:
            code[go] = why
    rows, cols = prev.shape
    keep = ((status != 0) & (nx >= 0) & (nx < F(cols)) & (ny >= 0) & (ny < F(rows))).astype(np.uint8)
    return dict(next_pt=np.stack([nx, ny], axis=1), pt_status=status, err=err, exit_code=code, keep=keep, level_exit=level_exit)


def ref_lk(frames, **params):
    """the whole call -> the fields of Solver.lk_track's dict, plus level_exit"""
    p = dict(PARAMS, **params)
    parts = []
    for fr in frames:
        pts = np.asarray(fr["pt"], F).reshape(-1, 2)
        if len(pts):
            parts.append(track_frame(fr["prev"], fr["next"], fr["win"], pts, **p))
        else:
            parts.append(dict(next_pt=np.zeros((0, 2), F), pt_status=np.zeros(0, np.uint8), err=np.zeros(0, F), exit_code=np.zeros(0, np.uint8),
                              keep=np.zeros(0, np.uint8), level_exit=np.zeros((0, 4), np.uint8)))
    out = {key: np.concatenate([q[key] for q in parts]) for key in parts[0]}
    counts = [len(q["keep"]) for q in parts]
    out["pt_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    kept = [np.nonzero(q["keep"])[0].astype(np.int32) for q in parts]
    out["kept_ptr"] = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int32)
    n_pt = int(out["pt_ptr"][-1])
    out["kept_src"] = np.full(n_pt, -1, np.int32)
    if kept:
        flat = np.concatenate(kept)
        out["kept_src"][:len(flat)] = flat
    return out


def compare(got, want, label=""):
    """exact, bit for bit (err and next_pt hold no NaN)"""
    for key in KEYS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, key, a.shape, b.shape, a.dtype, b.dtype)
        same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == F else a == b
        assert same.all(), (label, key, np.argwhere(~same)[:5].tolist(), a[~same][:5], b[~same][:5])


# ---- loops ---------------------------------------------------------------------------------------------------------------------

def _r(i, n):
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * n - 2 - i
    return i


def pyr_down_literal(img):
    h, w = img.shape
    k = (1, 4, 6, 4, 1)
    src = img.tolist()
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            total = 0
            for j in range(5):
                row = src[_r(2 * y + j - 2, h)]
                for i in range(5):
                    total += k[j] * k[i] * row[_r(2 * x + i - 2, w)]
            out[y, x] = (total + 128) >> 8
    return out


def _pix(img, w, h, x, y):
    return img[_r(y, h)][_r(x, w)]


def _deriv(img, w, h, x, y):
    if x < 0 or x >= w or y < 0 or y >= h:
        return 0, 0
    p = lambda dx, dy: _pix(img, w, h, x + dx, y + dy)                # noqa: E731
    return (3 * (p(1, -1) - p(-1, -1)) + 10 * (p(1, 0) - p(-1, 0)) + 3 * (p(1, 1) - p(-1, 1)),
            3 * (p(-1, 1) - p(-1, -1)) + 10 * (p(0, 1) - p(0, -1)) + 3 * (p(1, 1) - p(1, -1)))


def _w_literal(a, b):
    one, k = F(1), F(16384)
    w00, w01, w10 = int(np.rint(F(F(one - a) * F(one - b)) * k)), int(np.rint(F(a * F(one - b)) * k)), int(np.rint(F(F(one - a) * b) * k))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _scaled1(s):
    return F(float(s) * 2.0 ** -20)


def point_literal(I_pyr, J_pyr, win, pt, max_iter=20, eps=0.01, min_eig_threshold=1e-4):
    """one point over pyramids given as nested lists -> (x, y, status, err, exit_code)"""
    L = len(I_pyr) - 1
    half = F(F(win - 1) * F(0.5))
    px, py = F(pt[0]), F(pt[1])
    status, err, code = 1, F(0), 0
    nx = ny = F(0)
    for l in range(L, -1, -1):
        I, J = I_pyr[l], J_pyr[l]
        h, w = len(I), len(I[0])
        s = F(1.0 / (1 << l))
        qx, qy = F(px * s), F(py * s)
        if l == L:
            nx, ny = qx, qy
        else:
            nx, ny = F(nx * F(2)), F(ny * F(2))
        ux, uy = F(qx - half), F(qy - half)
        fx, fy = np.floor(ux), np.floor(uy)
        if fx < -win or fx >= w or fy < -win or fy >= h:
            if l == 0:
                status, err, code = 0, F(0), REJ_START
            continue
        ix, iy = int(fx), int(fy)
        wt = _w_literal(F(ux - fx), F(uy - fy))
        patch = []
        a11 = a12 = a22 = 0
        for y in range(win):
            for x in range(win):
                X, Y = ix + x, iy + y
                cells = ((X, Y), (X + 1, Y), (X, Y + 1), (X + 1, Y + 1))
                val = sum(_pix(I, w, h, cx, cy) * k for (cx, cy), k in zip(cells, wt))
                ds = [_deriv(I, w, h, cx, cy) for cx, cy in cells]
                sx, sy = sum(d[0] * k for d, k in zip(ds, wt)), sum(d[1] * k for d, k in zip(ds, wt))
                e = ((val + 256) >> 9, (sx + 8192) >> 14, (sy + 8192) >> 14)
                patch.append(e)
                a11 += e[1] * e[1]
                a12 += e[1] * e[2]
                a22 += e[2] * e[2]
        A11, A12, A22 = _scaled1(a11), _scaled1(a12), _scaled1(a22)
        D = F(F(A11 * A22) - F(A12 * A12))
        dA = F(A11 - A22)
        root = np.sqrt(F(F(dA * dA) + F(F(4) * F(A12 * A12))))
        min_eig = F(F(F(A22 + A11) - root) / F(2 * win * win))
        err = min_eig
        if float(min_eig) < min_eig_threshold or D < FLT_EPSILON:
            if l == 0:
                status, code = 0, REJ_MIN_EIG
            continue
        D = F(F(1) / D)
        cx, cy = F(nx - half), F(ny - half)
        pdx = pdy = F(0)
        why = MAX_ITER_RAN
        for j in range(max_iter):
            gx, gy = np.floor(cx), np.floor(cy)
            if gx < -win or gx >= w or gy < -win or gy >= h:
                if l == 0:
                    status = 0
                why = REJ_LOOP
                break
            jx, jy = int(gx), int(gy)
            v = _w_literal(F(cx - gx), F(cy - gy))
            b1 = b2 = 0
            at = 0
            for y in range(win):
                for x in range(win):
                    X, Y = jx + x, jy + y
                    val = _pix(J, w, h, X, Y) * v[0] + _pix(J, w, h, X + 1, Y) * v[1] + _pix(J, w, h, X, Y + 1) * v[2] + _pix(J, w, h, X + 1, Y + 1) * v[3]
                    diff = ((val + 256) >> 9) - patch[at][0]
                    b1 += diff * patch[at][1]
                    b2 += diff * patch[at][2]
                    at += 1
            B1, B2 = _scaled1(b1), _scaled1(b2)
            dx = F(F(F(A12 * B2) - F(A22 * B1)) * D)
            dy = F(F(F(A12 * B1) - F(A11 * B2)) * D)
            cx, cy = F(cx + dx), F(cy + dy)
            nx, ny = F(cx + half), F(cy + half)
            if float(dx) * float(dx) + float(dy) * float(dy) <= float(eps) * float(eps):
                why = EPS
                break
            if j > 0 and abs(float(F(dx + pdx))) < 0.01 and abs(float(F(dy + pdy))) < 0.01:
                nx, ny = F(nx - F(dx * F(0.5))), F(ny - F(dy * F(0.5)))
                why = OSCILLATION
                break
            pdx, pdy = dx, dy
        if l == 0:
            code = why
    return nx, ny, status, err, code


def ref_lk_literal(fr, which, literal_pyramid=True, **params):
    """points `which` of one frame, by loops -> dict of next_pt, pt_status, err, exit_code, keep for those points"""
    p = dict(PARAMS, **params)
    win, rows, cols = fr["win"], fr["prev"].shape[0], fr["prev"].shape[1]
    pyrs = []
    for img in (fr["prev"], fr["next"]):
        levels = [img]
        for _ in level_sizes(rows, cols, win, p["max_level"])[1:]:
            levels.append(pyr_down_literal(levels[-1]) if literal_pyramid else pyr_down(levels[-1]))
        pyrs.append([a.tolist() for a in levels])
    pts = np.asarray(fr["pt"], F).reshape(-1, 2)
    out = dict(next_pt=[], pt_status=[], err=[], exit_code=[], keep=[])
    for i in which:
        x, y, status, err, code = point_literal(pyrs[0], pyrs[1], win, pts[i], p["max_iter"], p["eps"], p["min_eig_threshold"])
        out["next_pt"].append((x, y)); out["pt_status"].append(status); out["err"].append(err); out["exit_code"].append(code)
        out["keep"].append(int(bool(status) and 0 <= x < cols and 0 <= y < rows))
    return dict(next_pt=np.array(out["next_pt"], F).reshape(-1, 2), pt_status=np.array(out["pt_status"], np.uint8), err=np.array(out["err"], F),
                exit_code=np.array(out["exit_code"], np.uint8), keep=np.array(out["keep"], np.uint8))


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def texture(rows, cols, seed, shift8=(0, 0), noise=0, flat=None, waves=8):
    """A deterministic 8-bit texture, integer arithmetic throughout: a sum of triangle waves over (8 x - shift8[0], 8 y - shift8[1]),
    so shift8 moves the content by eighths of a pixel; noise: uniform in [-noise, noise], drawn anew for every shift; flat: (x0, y0,
    x1, y1) painted with one value."""
    rng = np.random.default_rng(seed)
    Y, X = np.mgrid[0:rows, 0:cols].astype(np.int64)
    X, Y = 8 * X - shift8[0], 8 * Y - shift8[1]
    v = np.full((rows, cols), 128 * 64, np.int64)
    for _ in range(waves):
        a, b = (int(t) for t in rng.integers(-7, 8, 2))
        c, P, amp = int(rng.integers(0, 4096)), int(rng.integers(96, 400)), int(rng.integers(8, 24))
        t = (a * X + b * Y + c) % P
        v += amp * 64 * np.abs(2 * t - P) // P - amp * 32
    img = (v + 32) >> 6
    if noise:
        img = img + np.random.default_rng([seed, 7, shift8[0] & 0xffff, shift8[1] & 0xffff]).integers(-noise, noise + 1, img.shape)
    if flat:
        img[flat[1]:flat[3], flat[0]:flat[2]] = 90
    return np.clip(img, 0, 255).astype(np.uint8)


def frame(rows, cols, win, pts, seed, shift8=(10, -6), noise=2, flat=None):
    return dict(prev=texture(rows, cols, seed, (0, 0), noise, flat), next=texture(rows, cols, seed, shift8, noise, flat), win=win,
                pt=np.asarray(pts, F).reshape(-1, 2))


def edge_points(rows, cols, win):
    """the window's corner at -win (the furthest it may hang over), one beyond, at 0, at the last pixel (hanging over by win on the
    far side) and one beyond, on each axis and in every combination: every edge and corner"""
    half = (win - 1) / 2
    def axis(n):
        return [-win + half, -win + half - 0.5, -win + half + 0.25, half, n / 2 + 0.3, n - 1 + half, n - 1 + half + 0.75, n + half]
    return [(x, y) for x in axis(cols) for y in axis(rows)]


# rows, cols, win of sizes_case's frames, and the top level L the rule gives each.  The 96 x 80 and 80 x 96 frames stop at level 1
# with either window (their level 2 is 24 x 20, and 20 is not above 21); 96 x 88 is the frame that stops at level 2 with 21.
# 200 x 168 stops at level 2 as well - its level 3 would be 25 x 21 and a side EQUAL to the window ends the pyramid - and 200 x 169
# (25 x 22) is the smallest that reaches level 3.  40 x 36 with 31 has level 0 alone; windows 3 and 5 leave most lanes idle.
SIZES = ((96, 80, 21, 1), (96, 80, 31, 1), (80, 96, 21, 1), (80, 96, 31, 1), (40, 36, 31, 0), (200, 168, 21, 2), (200, 169, 21, 3), (96, 88, 21, 2),
         (24, 20, 3, 2), (40, 36, 5, 2))
SIZES_RANDOM = 12
FLAT = (28, 26, 78, 76)              # exits_case: a rect of one value, larger than the window and its Scharr ring at level 0
COUNTS = (0, 1, 63, 64, 65, 4097)
N_FRAMES = 1024
FRAMES_ALONE = (0, 63, 64, 65, 511, 1023)
TIE_POINT = (40.0, 20.5 + 2.0 ** -15)


@functools.lru_cache(maxsize=None)
def sizes_case():
    """every frame size and window the header's level rule distinguishes; per frame the 64 edge and corner points of edge_points
    and SIZES_RANDOM points anywhere; the content moves by (1.25, -0.75) pixels"""
    rng = np.random.default_rng(5)
    frames = []
    for rows, cols, win, _ in SIZES:
        pts = edge_points(rows, cols, win) + [(rng.uniform(0, cols), rng.uniform(0, rows)) for _ in range(SIZES_RANDOM)]
        frames.append(frame(rows, cols, win, pts, seed=1000 + rows + win))
    return frames


@functools.lru_cache(maxsize=None)
def sizes_ref():
    return ref_lk(sizes_case())


@functools.lru_cache(maxsize=None)
def exits_case():
    """96 x 88, window 21 (levels 0 .. 2): points inside the flat rect (the minimum-eigenvalue exit at level 0, while the upper
    levels, where the rect is smaller than the window, run), points on texture that moves by (2.5, 1.25) under light noise (eps),
    and points on texture under heavy noise in the next image alone, near the border, where the walk oscillates, runs out of
    iterations or leaves the bounds"""
    rng = np.random.default_rng(8)
    rows, cols, win = 96, 88, 21
    prev = texture(rows, cols, 77, (0, 0), 2, FLAT)
    nxt = texture(rows, cols, 77, (20, 10), 2, FLAT)
    heavy = np.random.default_rng(9).integers(-70, 71, (rows, 30))
    nxt[:, :30] = np.clip(nxt[:, :30].astype(np.int64) + heavy, 0, 255).astype(np.uint8)
    pts = [(53.0, 51.0), (52.25, 50.5), (54.0, 52.75)]
    pts += [(rng.uniform(40, 84), rng.uniform(2, 14) if k % 2 else rng.uniform(87, 93)) for k in range(20)]      # above and below the flat rect
    pts += [(rng.uniform(-6, 24), rng.uniform(-6, 100)) for _ in range(60)]
    return [dict(prev=prev, next=nxt, win=win, pt=np.asarray(pts, F)), fine_frame()]


def fine_frame():
    """96 x 88, window 21: a vertical edge and rows that alternate in pairs by 6 grey levels.  At level 0 the pairs give Iy, at level
    1 they are rows that alternate singly, whose central difference is exactly 0: there the matrix is singular (D < FLT_EPSILON)
    while level 0 tracks - an upper level that fails by the matrix test and a walk that goes on.  The edge moves by one pixel."""
    Y, X = np.mgrid[0:96, 0:88]
    rows = 6 * ((Y % 4) < 2)
    return dict(prev=(60 + 120 * (X >= 44) + rows).astype(np.uint8), next=(60 + 120 * (X >= 45) + rows).astype(np.uint8), win=21,
                pt=np.asarray([(44.0, 48.0), (43.25, 46.5), (45.5, 50.0)], F))


@functools.lru_cache(maxsize=None)
def exits_ref():
    return ref_lk(exits_case())


@functools.lru_cache(maxsize=None)
def counts_case():
    """COUNTS points in frames of 40 x 36 with window 5: wavefronts and workgroups of k_lk_track partly filled, and five chunks of
    k_lk_keep in the last frame; points up to 6 pixels outside, so keep is mixed"""
    rng = np.random.default_rng(12)
    return [frame(40, 36, 5, np.stack([rng.uniform(-6, 42, n), rng.uniform(-6, 46, n)], axis=1), seed=300 + k) for k, n in enumerate(COUNTS)]


@functools.lru_cache(maxsize=None)
def counts_ref():
    return ref_lk(counts_case())


@functools.lru_cache(maxsize=None)
def frames_case():
    """N_FRAMES frames of 6 .. 11 pixels a side with window 3 and 0 .. 3 points: runs of frames without points (some of them
    without images), at the start, at the end and across the wavefronts of the frame scan"""
    rng = np.random.default_rng(15)
    frames = []
    for f in range(N_FRAMES):
        rows, cols = int(rng.integers(6, 12)), int(rng.integers(6, 12))
        n = 0 if f in (0, 1, 2, N_FRAMES - 1) or 66 <= f < 76 or 126 <= f < 131 or f % 7 == 3 else int(rng.integers(1, 4))
        if f in FRAMES_ALONE[1:5]:
            n = 2
        pts = np.stack([rng.uniform(-1, cols + 1, n), rng.uniform(-1, rows + 1, n)], axis=1)
        if n == 0 and f % 2:
            frames.append(dict(prev=None, next=None, rows=rows, cols=cols, win=3, pt=np.zeros((0, 2), F)))
        else:
            frames.append(dict(prev=texture(rows, cols, 5000 + f, (0, 0), 1, None, 4), next=texture(rows, cols, 5000 + f, (4, 3), 1, None, 4), win=3,
                               pt=np.asarray(pts, F).reshape(-1, 2)))
    return frames


@functools.lru_cache(maxsize=None)
def frames_ref():
    return ref_lk(frames_case())


@functools.lru_cache(maxsize=None)
def tie_case():
    """96 x 80, window 31: TIE_POINT has a = 0 and b = 0.5 + 2^-15 at level 0, so (1 - a)(1 - b) 16384 = 8191.5 and (1 - a) b 16384 =
    8192.5: both round to the even 8192; and the same with the axes exchanged"""
    return [frame(96, 80, 31, [TIE_POINT, (TIE_POINT[1] + 20, TIE_POINT[0])], seed=41)]


@functools.lru_cache(maxsize=None)
def tie_ref():
    return ref_lk(tie_case())


def frame_part(res, f):
    """frame f's rows of a call's result, as the result of a call with that frame alone"""
    a, b = int(res["pt_ptr"][f]), int(res["pt_ptr"][f + 1])
    ka, kb = int(res["kept_ptr"][f]), int(res["kept_ptr"][f + 1])
    out = {key: res[key][a:b] for key in ("next_pt", "pt_status", "err", "exit_code", "keep")}
    out["kept_ptr"] = np.array([0, kb - ka], np.int32)
    out["kept_src"] = np.full(b - a, -1, np.int32)
    out["kept_src"][:kb - ka] = res["kept_src"][ka:kb]
    return out


def shift_truth_case(shift):
    """ground truth that does not come from the restatement: a sum of six sinusoids sampled analytically at x and at x - shift,
    rounded to 8 bits; 25 points on a lattice well inside 160 x 200; window 21, the reference's parameters"""
    rows, cols = 160, 200
    Y, X = np.mgrid[0:rows, 0:cols].astype(np.float64)
    waves = ((0.11, 0.05, 0.3, 30), (-0.07, 0.13, 1.1, 26), (0.19, -0.04, 2.0, 18), (0.03, 0.21, 0.7, 22), (0.33, 0.29, 4.0, 8), (-0.26, 0.37, 5.2, 7))

    def sample(x, y):
        return np.clip(np.rint(128 + sum(a * np.sin(fx * x + fy * y + ph) for fx, fy, ph, a in waves)), 0, 255).astype(np.uint8)

    pts = [(40.0 + 30 * i, 35.0 + 22.5 * j) for i in range(5) for j in range(5)]
    return dict(prev=sample(X, Y), next=sample(X - shift[0], Y - shift[1]), win=21, pt=np.asarray(pts, F))


def digest(res):
    """a few numbers that follow every bit of a result"""
    bits = lambda a: int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())         # noqa: E731
    return dict(next_pt=bits(res["next_pt"]), err=bits(res["err"]), kept=int(res["kept_ptr"][-1]), kept_src=int(res["kept_src"].astype(np.int64).sum()),
                exits=tuple(int((res["exit_code"] == c).sum()) for c in (EPS, OSCILLATION, MAX_ITER_RAN, REJ_START, REJ_MIN_EIG, REJ_LOOP)))


# digest(sizes_ref()) when the cases were written
PINNED = dict(next_pt=2727982194655, err=161823262230, kept=149, kept_src=8345, exits=(91, 52, 9, 280, 321, 7))
