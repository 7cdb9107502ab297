"""movba_track_match restated from the rules of include/movba.h (what the CPU and GPU tests compare against), twice: literally - a
double loop with `break` for TRIANGULATION, a first-insert dict for LOOKUP - and with a dict per searched view for the large
case (tests/test_track_match_cpu.py shows the two equal on every small case); and the committed cases: the mixed call, the call
at MOVBA_MAX_TRACK_SLOTS, the call at MOVBA_MAX_TRACK_QUERIES, the gather call and the chain into movba_triangulate.  Everything is integer or a copy of bits: every
comparison is exact equality.  Helper module: no tests here (tests/test_track_match_cpu.py, tests/test_gpu_track_match.py).

A call is (views, queries) as movba.capi.track_desc takes them: views is a list of dicts with `track` and optionally `taken`,
`obs`, `ur`, `depth`; a query is (TM_TRIANGULATION, view 1, view 2) or (TM_LOOKUP, view, ids)."""
import functools

import numpy as np

TM_TRIANGULATION, TM_LOOKUP = 0, 1
MAX_SLOTS = 16384
INT_KEYS = ("pair_ptr", "match_slot1", "match_slot2", "item_slot", "n_found")
PAYLOAD = (("obs1", "obs", 0), ("obs2", "obs", 1), ("ur1", "ur", 0), ("ur2", "ur", 1), ("depth1", "depth", 0), ("depth2", "depth", 1))
MIXED_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


def _taken(view):
    t = view.get("taken")
    return np.zeros(len(view["track"]), np.uint8) if t is None else np.asarray(t, np.uint8)


# ---- the literal restatement ------------------------------------------------------------------------------------------------

def tri_literal(view1, view2):
    """for every slot i of view 1 that is not taken, ascending: the first slot j of view 2 that is not taken and carries i's id"""
    track1, taken1, track2, taken2 = view1["track"], _taken(view1), view2["track"], _taken(view2)
    pairs = []
    for i in range(len(track1)):
        if taken1[i]:
            continue
        for j in range(len(track2)):
            if taken2[j]:
                continue
            if track2[j] == track1[i]:
                pairs.append((i, j))
                break
    return pairs


def lookup_literal(view, ids):
    """the map filled in slot order, the first insertion kept; then one lookup per id"""
    first = {}
    for j, t in enumerate(view["track"]):
        if int(t) not in first:
            first[int(t)] = j
    return [first.get(int(t), -1) for t in ids]


# ---- the same with one dict per searched view ---------------------------------------------------------------------------------

def tri_fast(view1, view2):
    track2, taken2 = np.asarray(view2["track"]).tolist(), _taken(view2).tolist()
    first = {}
    for j in range(len(track2) - 1, -1, -1):            # descending: the lowest slot is written last
        if not taken2[j]:
            first[track2[j]] = j
    track1, taken1 = np.asarray(view1["track"]).tolist(), _taken(view1).tolist()
    return [(i, first[t]) for i, t in enumerate(track1) if not taken1[i] and t in first]


def lookup_fast(view, ids):
    track = np.asarray(view["track"]).tolist()
    first = {}
    for j in range(len(track) - 1, -1, -1):
        first[track[j]] = j
    return [first.get(t, -1) for t in np.asarray(ids).tolist()]


def ref_track_match(views, queries, literal=True):
    """-> the dict Solver.track_match returns (without status): n_matches, pairs, matches, match_slot1 / 2 with their -1 tail,
    the payload with its NaN tail, item_slot, query_ptr, n_found"""
    tri, look = (tri_literal, lookup_literal) if literal else (tri_fast, lookup_fast)
    nq = len(queries)
    cap = sum(len(views[q[1]]["track"]) for q in queries if q[0] == TM_TRIANGULATION)
    have = [src for src in ("obs", "ur", "depth") if views and views[0].get(src) is not None]
    out = dict(pair_ptr=np.zeros(nq + 1, np.int32), match_slot1=np.full(cap, -1, np.int32), match_slot2=np.full(cap, -1, np.int32),
               n_found=np.zeros(nq, np.int32), matches={})
    for key, src, _ in PAYLOAD:
        if src in have:
            out["matches"][key] = np.full((cap, 2) if src == "obs" else (cap,), np.nan)
    # (the payload as 64-bit words: what is gathered is a copy of the bits, NaN payloads included)
    words = [{src: np.ascontiguousarray(v[src], np.float64).reshape(len(v["track"]), 2 if src == "obs" else 1).view(np.uint64) for src in have} for v in views]
    dest = {key: out["matches"][key].reshape(cap, 2 if key.startswith("obs") else 1).view(np.uint64) for key in out["matches"]}
    slots, qview, at = [], [], 0
    for q, query in enumerate(queries):
        if query[0] == TM_LOOKUP:
            found = look(views[query[1]], query[2])
            slots.append(np.asarray(found, np.int32).reshape(-1))
            out["n_found"][q] = sum(1 for j in found if j >= 0)
            qview.append((-1, query[1]))
        else:
            for i, j in tri(views[query[1]], views[query[2]]):
                out["match_slot1"][at], out["match_slot2"][at] = i, j
                for key, src, side in PAYLOAD:
                    if src in have:
                        dest[key][at] = words[query[2]][src][j] if side else words[query[1]][src][i]
                at += 1
            slots.append(np.zeros(0, np.int32))
            qview.append((query[1], query[2]))
        out["pair_ptr"][q + 1] = at
    out["n_matches"] = at
    out["item_slot"] = np.concatenate(slots).astype(np.int32) if slots else np.zeros(0, np.int32)
    out["query_ptr"] = np.concatenate([[0], np.cumsum([len(s) for s in slots])]).astype(np.int32)
    out["pairs"] = dict(pair_view=np.array(qview, np.int32).reshape(nq, 2), pair_ptr=out["pair_ptr"])
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def compare(got, ref, label=""):
    """every integer array equal entry by entry with its -1 tail, every payload array equal as uint64 up to the last match and
    NaN behind it; the number of differing entries printed first"""
    assert int(got["n_matches"]) == int(ref["n_matches"]), (label, got["n_matches"], ref["n_matches"])
    n = int(ref["n_matches"])
    for key in INT_KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape and g.dtype == np.int32, (label, key, g.shape, r.shape)
        bad = int((g != r).sum())
        print(label, key, "differing entries", bad)
        assert bad == 0, (label, key, np.argwhere(g != r)[:5].tolist())
    assert np.array_equal(got["pairs"]["pair_view"], ref["pairs"]["pair_view"]) and np.array_equal(got["query_ptr"], ref["query_ptr"]), label
    assert sorted(got["matches"]) == sorted(ref["matches"]), (label, sorted(got["matches"]))
    for key in ref["matches"]:
        g, r = np.asarray(got["matches"][key]), np.asarray(ref["matches"][key])
        assert g.shape == r.shape and g.dtype == np.float64, (label, key, g.shape, r.shape)
        bad = int((bits(g[:n]) != bits(r[:n])).sum())
        print(label, key, "differing words", bad)
        assert bad == 0 and np.isnan(g[n:]).all(), (label, key)


def rows(res, qs):
    """the per-query rows of a result, for the queries qs in that order: (matches as (slot1, slot2) lists, payload words, item
    slots, n_found)"""
    out = []
    for q in qs:
        a, b = int(res["pair_ptr"][q]), int(res["pair_ptr"][q + 1])
        i0, i1 = int(res["query_ptr"][q]), int(res["query_ptr"][q + 1])
        out.append((res["match_slot1"][a:b].tolist(), res["match_slot2"][a:b].tolist(),
                    {k: bits(v[a:b]).tolist() for k, v in res["matches"].items()}, res["item_slot"][i0:i1].tolist(), int(res["n_found"][q])))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _payload(rng, n, view_index):
    """distinct bit patterns per slot, NaNs with payload bits among them"""
    words = (np.uint64(0x3ff0000000000000) + np.arange(4 * n, dtype=np.uint64) * np.uint64(0x10001) + np.uint64(view_index << 40)).reshape(n, 4)
    nan = rng.random(n) < 0.1
    words[nan] = np.uint64(0x7ff8000000000000) | (words[nan] & np.uint64(0x0007ffffffffffff)) | np.uint64(1)
    w = np.ascontiguousarray(words)
    return dict(obs=w[:, :2].copy().view(np.float64), ur=w[:, 2].copy().view(np.float64), depth=w[:, 3].copy().view(np.float64))


@functools.lru_cache(maxsize=None)
def mixed_case(payload=True):
    """Views of 0, 1, 63, 64, 65, 255, 256, 257 and 1 000 slots with ids from a pool small enough that about a quarter of the slots
    repeat an id of their view, half the slots taken; one more view with every slot taken, one with every slot carrying one id;
    about 40 queries of both modes, one of them a view against itself, items absent from their view, a LOOKUP without items."""
    rng = np.random.default_rng(9100)
    views = []
    for n in MIXED_SIZES:
        pool = max(2 * n, 1)                                # n draws from 2 n ids: about a fifth to a quarter repeat
        v = dict(track=rng.integers(-pool // 2, pool - pool // 2, n).astype(np.int32), taken=(rng.random(n) < 0.5).astype(np.uint8))
        views.append(v)
    views.append(dict(track=rng.integers(-128, 128, 256).astype(np.int32), taken=np.ones(256, np.uint8)))     # 9: all taken
    views.append(dict(track=np.full(300, 77, np.int32), taken=(rng.random(300) < 0.5).astype(np.uint8)))     # 10: one id
    views[10]["taken"][:3] = 1                                                                                # (its lowest free slot is not 0)
    views[8]["track"][::97] = 77                                                                              # (the big view meets view 10)
    if payload:
        for k, v in enumerate(views):
            v.update(_payload(rng, len(v["track"]), k))
    T, L = TM_TRIANGULATION, TM_LOOKUP
    queries = [(T, 8, 8), (T, 8, 7), (T, 7, 8), (T, 5, 6), (T, 6, 5), (T, 3, 4), (T, 4, 2), (T, 1, 2), (T, 2, 1), (T, 0, 8), (T, 8, 0),
               (T, 0, 0), (T, 9, 8), (T, 8, 9), (T, 10, 8), (T, 8, 10), (T, 10, 10), (T, 1, 1), (T, 7, 6), (T, 2, 8), (T, 6, 7)]
    for view in (8, 7, 6, 5, 4, 3, 2, 1, 0, 9, 10):
        track = views[view]["track"]
        n_items = (0, 1, 64, 257, 1500)[view % 5]
        own = rng.choice(track, n_items) if len(track) else np.zeros(n_items, np.int32)
        absent = rng.integers(5000, 6000, n_items).astype(np.int32)
        queries.append((L, view, np.where(rng.random(n_items) < 0.7, own, absent).astype(np.int32)))
    queries += [(L, 8, np.zeros(0, np.int32)), (L, 8, views[8]["track"][::-1].copy()), (L, 10, np.array([77, 78, 77], np.int32)),
                (L, 9, views[9]["track"][:40].copy()), (T, 5, 8), (L, 2, np.array([5000], np.int32)), (T, 8, 5), (L, 0, np.array([0, -1], np.int32))]
    return views, queries


@functools.lru_cache(maxsize=None)
def mixed_ref(payload=True):
    return ref_track_match(*mixed_case(payload))


@functools.lru_cache(maxsize=None)
def full_case():
    """One view at MOVBA_MAX_TRACK_SLOTS with all-distinct ids, INT32_MIN and negatives among them, a third of its slots taken,
    against itself and against a 1-slot view, in both modes."""
    rng = np.random.default_rng(9200)
    ids = rng.choice(np.setdiff1d(np.arange(-(1 << 20), 1 << 20, dtype=np.int64), [0, -1]), MAX_SLOTS, replace=False).astype(np.int32)
    ids[5] = np.iinfo(np.int32).min
    ids[6], ids[7] = 0, -1
    big = dict(track=ids, taken=(rng.random(MAX_SLOTS) < 1 / 3).astype(np.uint8))
    big["taken"][[5, 6, 7, 11000]] = 0
    one = dict(track=ids[11000:11001].copy(), taken=np.zeros(1, np.uint8))
    T, L = TM_TRIANGULATION, TM_LOOKUP
    items = np.concatenate([ids[::-3], np.array([1 << 25, -(1 << 25)], np.int32)]).astype(np.int32)
    queries = [(T, 0, 0), (T, 0, 1), (T, 1, 0), (L, 0, items), (L, 1, ids[10990:11010].copy()), (L, 0, ids.copy())]
    return [big, one], queries


@functools.lru_cache(maxsize=None)
def full_ref():
    return ref_track_match(*full_case(), literal=False)


def strip(views, keys):
    """the views without the given optional arrays"""
    return [{k: v for k, v in view.items() if k not in keys} for view in views]


def hand_cases():
    """the header's rules one by one, under 10 slots each: (label, views, queries, expected matches or item slots per query)"""
    T, L = TM_TRIANGULATION, TM_LOOKUP
    lo = int(np.iinfo(np.int32).min)

    def view(track, taken=None):
        v = dict(track=np.array(track, np.int32))
        if taken is not None:
            v["taken"] = np.array(taken, np.uint8)
        return v

    return [
        ("duplicates in view 1 share a j", [view([4, 9, 4, 4]), view([1, 4, 4, 9])], [(T, 0, 1)], [[(0, 1), (1, 3), (2, 1), (3, 1)]]),
        ("taken slots are skipped on both sides", [view([4, 5, 6, 7], [0, 1, 0, 0]), view([4, 4, 5, 6, 7], [1, 0, 0, 1, 0])], [(T, 0, 1)],
         [[(0, 1), (3, 4)]]),
        ("LOOKUP ignores taken and returns the first slot", [view([8, 3, 8, 3], [1, 1, 1, 1])], [(L, 0, [3, 8, 5, 3])], [[1, 0, -1, 1]]),
        ("view 1 equal to view 2", [view([2, 2, 3, 2], [1, 0, 0, 0])], [(T, 0, 0)], [[(1, 1), (2, 2), (3, 1)]]),
        ("ids 0, -1 and INT32_MIN", [view([0, -1, lo, 1]), view([lo, 5, -1, 0, 0])], [(T, 0, 1), (L, 1, [0, -1, lo, 1]), (L, 0, [lo])],
         [[(0, 3), (1, 2), (2, 0)], [3, 2, 0, -1], [2]]),
        ("slot_taken left out: no slot is taken", [view([1, 2]), view([2, 1, 2])], [(T, 0, 1), (T, 1, 0)], [[(0, 1), (1, 0)], [(0, 1), (1, 0), (2, 1)]]),
        ("an empty view on either side", [view([]), view([3])], [(T, 0, 1), (T, 1, 0), (L, 0, [3]), (T, 0, 0)], [[], [], [-1], []]),
    ]


@functools.lru_cache(maxsize=None)
def chain_case():
    """movba.synth.make_triangulation's scene of 3 pairs of 200 matches (half the near observations stereo) taken apart into slots:
    the current keyframe's slots are the 600 first observations in a shuffled order plus 40 that no neighbour carries, a neighbour's
    slots are its 200 second observations shuffled plus 20 strangers; an id per map point; a tenth of the slots taken.  -> (the
    scene, the views of track_match, its queries)"""
    from movba import synth
    sc = synth.make_triangulation(n_pairs=3, n_per_pair=200, seed=9300, stereo=True, stereo_frac=0.5)
    rng = np.random.default_rng(9301)
    m, ptr = sc["matches"], sc["pairs"]["pair_ptr"]
    M = int(ptr[-1])
    ids = rng.permutation(4000)[:M].astype(np.int32) - 2000

    def slots(obs, ur, depth, track, extra):
        n = len(track) + extra
        v = dict(obs=np.concatenate([obs, rng.uniform(0, 480, (extra, 2))]), ur=np.concatenate([ur, np.full(extra, -1.0)]),
                 depth=np.concatenate([depth, np.full(extra, -1.0)]), track=np.concatenate([track, 10000 + rng.permutation(1000)[:extra]]).astype(np.int32))
        order = rng.permutation(n)
        v = {k: np.ascontiguousarray(a[order]) for k, a in v.items()}
        v["taken"] = (rng.random(n) < 0.1).astype(np.uint8)
        return v

    views = [slots(m["obs1"], m["ur1"], m["depth1"], ids, 40)]
    for p in range(3):
        a, b = int(ptr[p]), int(ptr[p + 1])
        views.append(slots(m["obs2"][a:b], m["ur2"][a:b], m["depth2"][a:b], ids[a:b], 20))
    queries = [(TM_TRIANGULATION, int(v1), int(v2)) for v1, v2 in sc["pairs"]["pair_view"]]
    return sc, views, queries


MANY_QUERIES = 4096
MANY_ALONE = (0, 255, 256, 257, 4095)


@functools.lru_cache(maxsize=None)
def many_case():
    """MOVBA_MAX_TRACK_QUERIES queries over 64 views of 0 to 300 slots, both modes interleaved: k_tm_pack's sum over the query counts
    takes 16 passes of its stride of 256 and every wavefront of it holds counts.  Ids come from one pool of 600 for all views, so
    two views share a good part of theirs; views 1 and 2 are of 300 slots over a pool of 150 with nothing taken (several hundred
    matches), views 0 and 3 are empty.  The first and the last query match, and so do queries 255 to 257."""
    rng = np.random.default_rng(9400)
    sizes = rng.integers(0, 301, 64)
    sizes[[0, 3]] = 0
    sizes[[1, 2]] = 300
    views = []
    for k, n in enumerate(sizes.tolist()):
        pool = 150 if k in (1, 2) else 600
        taken = np.zeros(n, np.uint8) if k in (1, 2) else (rng.random(n) < 0.3).astype(np.uint8)
        v = dict(track=rng.integers(0, pool, n).astype(np.int32), taken=taken)
        v.update(_payload(rng, n, k))
        views.append(v)
    T, L = TM_TRIANGULATION, TM_LOOKUP
    queries = []
    for q in range(MANY_QUERIES):
        if q in (0, 255, 256, 257, MANY_QUERIES - 1):
            queries.append((T, 1 + q % 2, 2 - q % 2))
        elif q % 3 == 1 or rng.random() < 0.2:
            view = int(rng.integers(0, 64))
            queries.append((L, view, rng.integers(0, 600, int(rng.integers(0, 6))).astype(np.int32)))
        else:
            queries.append((T, int(rng.integers(0, 64)), int(rng.integers(0, 64))))
    return views, queries


@functools.lru_cache(maxsize=None)
def many_ref():
    return ref_track_match(*many_case(), literal=False)
