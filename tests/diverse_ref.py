"""What an answer of GpuIndex.search_diverse (eps_index_search_diverse) is held to, in numpy: for tests/test_diverse_ref_cpu.py (hand-written cases
and planted faults) and tests/test_gpu_search_diverse.py (fed with what the device returns).  Nothing here is fitted to device output.

The rule, for one query.  The pool is a list of rows in ascending (distance, id) order - a flat search's fetch_k closest visible rows, or
search_among's over the caller's lists; d[i] is the distance of pool position i to the query, D[c][s] the distance search_among returns for pool
row c when the QUERY is pool row s.  lam = float32(lambda), mu = float32(1) - lam.  Step 1 takes position 0, score lam * d[0].  After a row s is
selected every unselected c updates m[c]: m[c] = D[c][s] after the first selection, later m[c] = D[c][s] iff D[c][s] < m[c] (IEEE: a NaN never
replaces a value, a NaN m is never replaced).  Step t >= 2 scores every unselected c as (lam * d[c]) - (mu * m[c]) - two rounded fp32 multiplies, one
rounded fp32 subtract - and takes the smallest score in the library's key order (-0 equals +0, every NaN after +inf), ties to the smaller position.
Selection stops at min(k, pool size).  Scores are reported as their keys hold them: -0 as +0, a NaN as the quiet NaN.

numpy_diverse runs the loop on np.float32 scalars: every `*` and `-` below is one IEEE fp32 operation.  `fault` plants the mistakes the CPU tests
show the comparator catches."""
import numpy as np

import among_ref as ar
import groups_ref as gr
import range_ref as rr

F = np.float32
QNAN = np.uint32(0x7FC00000)
ORD_NAN = np.uint32(0xFFC00000)


def ordinal(x):
    """make_key's order-preserving image of a float32 array: -0 folded into +0, every NaN the one ordinal above +inf"""
    x = np.asarray(x, F) + F(0)
    u = x.view(np.uint32)
    o = np.where(u >> np.uint32(31), ~u, u ^ np.uint32(0x80000000))
    return np.where(np.isnan(x), ORD_NAN, o).astype(np.uint32)


def key_float(x):
    """a float32 as a key holds it: -0 as +0, a NaN as the quiet NaN"""
    x = np.asarray(x, F) + F(0)
    return np.where(np.isnan(x), QNAN, x.view(np.uint32)).astype(np.uint32).view(F)


def numpy_diverse(d_pool, D, k, lam, fault=None, info=None):
    """one query: d_pool float32[np] in pool order, D float32[np][np] (D[c][s]: row c, query s).  Returns (positions int64[k] -1 padded,
    dist float32[k] +inf padded, score float32[k] +inf padded, count).  info (a dict): "tied_steps" = steps whose smallest score two positions share"""
    d = key_float(np.asarray(d_pool, F).reshape(-1))
    npool = len(d)
    D = key_float(np.asarray(D, F).reshape(npool, npool))
    lam = F(lam)
    mu = F(1) - lam
    pos = np.full(k, -1, np.int64)
    dist = np.full(k, np.inf, F)
    score = np.full(k, np.inf, F)
    sel = min(k, npool)
    tied = 0
    m = np.zeros(npool, F)
    taken = np.zeros(npool, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(sel):
            if t == 0 and fault != "first_by_score":
                c, s = 0, lam * d[0]
            else:
                if fault == "fma":   # one rounding instead of two: the product is exact in fp64
                    sc = (np.float64(lam) * d.astype(np.float64) - (mu * m).astype(np.float64)).astype(F)
                else:
                    sc = lam * d - mu * m   # elementwise: two rounded multiplies, one rounded subtract (m = 0 before the first selection: first_by_score)
                o = ordinal(sc).astype(np.int64)
                if fault == "nan_first":
                    o[np.isnan(sc)] = -1
                if fault != "reselect":
                    o[taken] = 1 << 40
                at = np.flatnonzero(o == o.min())
                c = int(at[-1] if fault == "ties_larger" else at[0])
                tied += len(at) > 1
                s = sc[c]
            pos[t], dist[t], score[t] = c, d[c], key_float(s)
            taken[c] = True
            x = D[:, c]   # m of the unselected rows (a selected row's m is never read again)
            if fault == "overwrite" or (t == 0 and fault != "seed0"):
                m = x.copy()
            else:
                m = np.where(x < m, x, m)
    if info is not None:
        info["tied_steps"] = tied
    return pos, dist, score, sel


def pool_rows(d32_col, visible_col, fetch_k, rows=None):
    """a query's pool: the visible rows (of `rows`, default all) in ascending (distance, row) order, the first fetch_k"""
    cand = np.flatnonzero(visible_col) if rows is None else np.asarray(rows, np.int64)[np.asarray(visible_col)[np.asarray(rows, np.int64)]]
    return cand[gr.key_order(d32_col[cand], cand)][:fetch_k]


def numpy_answer(d32, pair_dist, k, fetch_k, lam, visible=None, lists=None, base=0, stride=1, fault=None, info=None):
    """the call's answer from fp32 distances d32 [n][nq] and pair_dist(rows) -> D float32 [len(rows)][len(rows)] (D[c][s]: row rows[c], query row
    rows[s]).  lists: None (the flat form), ONE array of ROWS or nq of them (among_ref.rows_of).  Returns (ids under the id map, dist, score, counts)"""
    n, nq = d32.shape
    vis = rr.visible2(n, nq, visible)
    if lists is not None:
        vis = vis & ar.list_masks(lists, n, nq)
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F)
    score = np.full((nq, k), np.inf, F)
    counts = np.zeros(nq, np.int32)
    tied = []
    for q in range(nq):
        pool = pool_rows(d32[:, q], vis[:, q], fetch_k)
        one = {}
        pos, dist[q], score[q], counts[q] = numpy_diverse(d32[pool, q], pair_dist(pool), k, lam, fault=fault, info=one)
        ids[q, :counts[q]] = pool[pos[:counts[q]]] * stride + base
        tied.append(one["tied_steps"])
    if info is not None:
        info["tied_steps"] = tied
    return ids, dist, score, counts


def ties_pairs(X, metric):
    """pair_dist of a table of ties: exact in any summation order (groups_ref.assert_ties_table checks that on the pool)"""
    return lambda rows: gr.assert_ties_table(X[rows], X[rows], metric) if len(rows) else np.zeros((0, 0), F)


def bits(x):
    x = np.asarray(x, F) + F(0)
    return np.where(np.isnan(x), QNAN, x.view(np.uint32))


def same(got, want, what=""):
    """ids, distance bits, score bits (a NaN equals a NaN), counts: equality, position by position"""
    for x, y, name in zip(got, want, ("ids", "dist", "score", "counts")):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, "%s %s: shape %s != %s" % (what, name, x.shape, y.shape)
        if name in ("dist", "score"):
            x, y = bits(x), bits(y)
        bad = np.argwhere(x != y)
        assert len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


# the ties fixtures of the GPU tests: groups_ref.ties_table(metric, n, d, nq, seed=3) with (fetch_k, k, lambdas).  tests/test_diverse_ref_cpu.py
# checks on each that the selection differs from the pool's head for every query at lambda <= 0.75, and that tied best scores occur
FIXTURES = ((300, 8, 5, 64, 10, (0.5, 0.75)), (500, 16, 8, 100, 10, (0.25,)), (200, 4, 6, 200, 32, (0.5,)))
LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)
