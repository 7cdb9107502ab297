"""movba_covisibility restated from the rules of include/movba.h (what the CPU and GPU tests compare against) - a dict counter per
query and `sorted`, nothing else - and the committed cases: the parity call, the wide call at MOVBA_MAX_COVIS_VIEWS and the tiny
one.  Everything is integer: every comparison is exact equality.  Helper module: no tests here
(tests/test_covisibility_cpu.py, tests/test_gpu_covisibility.py)."""
import numpy as np

KEYS = ("n_counted", "n_connected", "best_view", "best_weight", "out_view", "out_weight")
PARITY_VIEWS, PARITY_POINTS, PARITY_QUERIES = 300, 2000, 40
PARITY_LIST_LENGTHS = (0, 1, 2, 5, 17, 63, 64, 65, 300)
PARITY_QUERY_LENGTHS = (0, 1, 63, 64, 65, 257, 1500)
HIDDEN_BEST = 7             # the view of the parity case that would be best for query 5 and is not eligible
MAX_VIEWS = 8192


def ref_query(lists, items, self_view, eligible, min_weight):
    """one query -> (counter as dict view -> weight, ordered list of (view, weight), best_view, best_weight, n_connected)"""
    counter = {}
    for p in items:
        for v in lists[int(p)]:
            v = int(v)
            if v == self_view or (eligible is not None and not eligible[v]):
                continue
            counter[v] = counter.get(v, 0) + 1
    # sort(vPairs) ascending by (weight, view), pushed to the front one by one: descending by (weight, view)
    order = sorted(counter.items(), key=lambda kv: (kv[1], kv[0]), reverse=True)
    best_view, best_weight = -1, 0
    for v in sorted(counter):               # `>` in map order keeps the first maximum
        if counter[v] > best_weight:
            best_view, best_weight = v, counter[v]
    reaching = sum(1 for w in counter.values() if w >= min_weight)
    n_connected = reaching if reaching else (1 if counter else 0)
    return counter, order, best_view, best_weight, n_connected


def ref_covisibility(n_views, lists, queries, query_self=None, eligible=None, min_weight=15, max_out=None):
    """-> dict of the six arrays of movba_covis_result, out_view / out_weight as (Q, max_out), and `counters`: per query its dict"""
    max_out = n_views if max_out is None else max_out
    nq = len(queries)
    out = dict(n_counted=np.zeros(nq, np.int32), n_connected=np.zeros(nq, np.int32), best_view=np.zeros(nq, np.int32),
               best_weight=np.zeros(nq, np.int32), out_view=np.full((nq, max_out), -1, np.int32), out_weight=np.zeros((nq, max_out), np.int32),
               counters=[])
    for q, items in enumerate(queries):
        self_view = -1 if query_self is None else int(query_self[q])
        counter, order, bv, bw, nc = ref_query(lists, items, self_view, eligible, min_weight)
        out["counters"].append(counter)
        out["n_counted"][q], out["n_connected"][q], out["best_view"][q], out["best_weight"][q] = len(counter), nc, bv, bw
        for k, (v, w) in enumerate(order[:max_out]):
            out["out_view"][q, k], out["out_weight"][q, k] = v, w
    return out


def compare(got, ref, label=""):
    """all six arrays equal, entry by entry, the -1 / 0 padding included; the number of differing entries printed first"""
    for key in KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape and g.dtype == np.int32, (label, key, g.shape, r.shape)
        bad = int((g != r).sum())
        print(label, key, "differing entries", bad)
        assert bad == 0, (label, key, np.argwhere(g != r)[:5].tolist())


def subset(case, idx):
    """the call over the queries idx of a case, in that order"""
    idx = [int(i) for i in idx]
    return dict(case, queries=[case["queries"][i] for i in idx],
                query_self=None if case.get("query_self") is None else np.asarray(case["query_self"])[idx])


def rows(res, idx):
    """the rows idx of a result"""
    return {key: np.asarray(res[key])[list(idx)] for key in KEYS}


# ---- the parity call ------------------------------------------------------------------------------------------------------

_cache = {}


def parity_case():
    """300 views, 2 000 points with lists of 0, 1, 2, 5, 17, 63, 64, 65 and 300 (a hub: every view) observers, 40 queries of 0, 1,
    63, 64, 65, 257 and 1 500 items in turn; a quarter of the points with a list of 2 .. 65 name view 7, and view 7 is not
    eligible, as are about 10 % of the others.  Made on purpose: query 1 one point seen by five views (no view reaches 15); query
    2 hubs alone (every eligible view ties at the top); query 5 points that all name view 7; query 8 a point nobody sees; query 15
    a point seen by view 7 alone; every third query drawn with repetition; a third of the queries have themselves among their
    points' observers, a third have a self entry no list of theirs names (their points are drawn without hubs), the rest -1.
    -> dict(n_views, lists, queries, query_self, eligible, min_weight); computed once, not to be changed."""
    if "parity" in _cache:
        return _cache["parity"]
    rng = np.random.default_rng(20250907)
    V, P = PARITY_VIEWS, PARITY_POINTS
    lengths = rng.choice(PARITY_LIST_LENGTHS, size=P, p=[0.08, 0.15, 0.2, 0.25, 0.15, 0.05, 0.05, 0.05, 0.02])
    lengths[:len(PARITY_LIST_LENGTHS)] = PARITY_LIST_LENGTHS                 # (every length at least once)
    lists = []
    for p in range(P):
        l = rng.permutation(V)[:lengths[p]].astype(np.int32)
        if p % 4 == 0 and 2 <= lengths[p] < V and HIDDEN_BEST not in l:
            l[rng.integers(len(l))] = HIDDEN_BEST
        lists.append(l)
    eligible = (rng.random(V) >= 0.1).astype(np.uint8)
    eligible[HIDDEN_BEST] = 0
    by_len = {n: [p for p in range(P) if lengths[p] == n] for n in PARITY_LIST_LENGTHS}
    lonely = by_len[1][0]
    lists[lonely] = np.array([HIDDEN_BEST], np.int32)                         # its one observer is not eligible
    hubs, no_hubs = by_len[V], np.array([p for p in range(P) if lengths[p] != V])
    with_hidden = [p for p in range(P) if lengths[p] < V and HIDDEN_BEST in lists[p] and p != lonely]
    five = next(p for p in by_len[5] if eligible[lists[p]].sum() >= 2)
    queries, query_self = [], np.full(PARITY_QUERIES, -1, np.int32)
    for q in range(PARITY_QUERIES):
        n = PARITY_QUERY_LENGTHS[q % len(PARITY_QUERY_LENGTHS)]
        pool = no_hubs if q % 3 == 2 else np.arange(P)
        items = rng.choice(pool, size=n, replace=(q % 3 == 0))
        if q == 1:
            items = np.array([five])
        elif q == 2:
            items = rng.choice(hubs, size=n, replace=True)
        elif q == 5:
            items = rng.choice(with_hidden, size=n, replace=False)
        elif q == 8:
            items = np.array([by_len[0][0]])
        elif q == 15:
            items = np.array([lonely])
        items = items.astype(np.int32)
        queries.append(items)
        named = np.bincount(np.concatenate([lists[p] for p in items] + [np.zeros(0, np.int32)]), minlength=V)
        if q % 3 == 1 and named.any() and q not in (1, 15):
            query_self[q] = int(np.argmax(named * eligible))                  # inside: the view that would be best
        elif q % 3 == 2 and not named.all():
            query_self[q] = int(np.flatnonzero(named == 0)[-1])               # outside: a view no item names
    _cache["parity"] = dict(n_views=V, lists=lists, queries=queries, query_self=query_self, eligible=eligible, min_weight=15)
    return _cache["parity"]


def parity_ref():
    if "parity_ref" not in _cache:
        _cache["parity_ref"] = ref_covisibility(**parity_case())
    return _cache["parity_ref"]


# ---- the wide call: the bound on the views ----------------------------------------------------------------------------------

def wide_case(max_out=MAX_VIEWS):
    """8 192 views, 64 points: point 0 seen by every view, the others by 1 .. 8 192 of them; three queries: every point (every
    view is counted: the largest sort, weights 1 .. 64 with long ties), the point everybody sees alone (8 192 views tie), and 70
    items drawn with repetition with a self entry.  max_out 8 192 hands out the whole order, 7 its front."""
    if "wide" not in _cache:
        rng = np.random.default_rng(31)
        V = MAX_VIEWS
        lengths = [V] + [int(n) for n in rng.integers(1, V + 1, size=63)]
        lengths[1], lengths[2] = 1, V - 1
        lists = [rng.permutation(V)[:n].astype(np.int32) for n in lengths]
        queries = [np.arange(64, dtype=np.int32), np.zeros(1, np.int32), rng.integers(0, 64, size=70).astype(np.int32)]
        _cache["wide"] = dict(n_views=V, lists=lists, queries=queries, query_self=np.array([-1, -1, 4000], np.int32), eligible=None, min_weight=15)
    return dict(_cache["wide"], max_out=max_out)


def wide_ref(max_out=MAX_VIEWS):
    key = ("wide_ref", max_out)
    if key not in _cache:
        _cache[key] = ref_covisibility(**wide_case(max_out))
    return _cache[key]


# ---- the tiny call ----------------------------------------------------------------------------------------------------------

def tiny_case(self_view):
    """one view, one point seen by it, one query holding that point; self 0: nothing is counted, self -1: view 0 with weight 1"""
    return dict(n_views=1, lists=[np.zeros(1, np.int32)], queries=[np.zeros(1, np.int32)], query_self=np.array([self_view], np.int32),
                eligible=None, min_weight=15)
