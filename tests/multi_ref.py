"""What an answer of GpuIndex.search_multi (eps_index_search_multi) is held to, in numpy: for tests/test_multi_ref_cpu.py (fed with hand-written
cases and planted faults) and tests/test_gpu_multi.py (fed with what the device returns).  Nothing here is fitted to device output.

The rule.  Query j is a bag of t_j vectors, vectors[offsets[j] .. offsets[j + 1]).  For a vector u of the bag and a group g (rows with equal int64
keys): b(u, g) = the visible row of g with the smallest (distance, row) key - NaN after +inf, ties to the smaller row -, d(u, g) its distance.  g
QUALIFIES for the bag iff it has a visible row for EVERY vector of the bag; an empty bag has no qualifying group.  score = +0.0f, then
score = score + d(u, g) in fp32 for u in bag order, one add after the other: nothing is reassociated, NaN and infinities propagate.  The qualifying
groups are ordered by (score, group key), every NaN score in the one place after +inf, ties to the smaller key; the answer is the k smallest,
counts = min(k, qualifying).  match (j, slot s, vector u), flat at k * offsets[j] + s * t_j + u: the row of b(u, g_s) and d(u, g_s); unused slots
key 0 / +inf / -1 / +inf.  Candidates: only the groups whose keys the bag's list names; unknown keys are ignored, repeated ones count once.

numpy_multi computes the per-(vector, group) minima twice - from the minimum key of every group, and by a walk of every vector's visible rows in
ascending key order that records first occurrences - and asserts that the two agree.

The yardstick tables are tables of ties (groups_ref.ties_table): every distance is a small integer (or a multiple of 1 / 256 for COSINE) and
assert_ties_bags checks that every partial sum of every bag stays below 2^24 in magnitude (in units of the table's grid), so a sum is exact in
ANY order and the table pins the rule - minima, qualification, order, layout - without relying on the device's distances.  The order of the sum
is pinned by the continuous tables, where the model is fed the device's own flat distances."""
import numpy as np

import groups_ref as gr

F = np.float32


def bag_offsets(sizes):
    o = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=o[1:])
    return o


def assert_ties_bags(d32, offsets, grid=1.0):
    """every distance a multiple of `grid` and every bag's sum of |distance| / grid below 2^24: every partial sum is exact in any order"""
    d = np.asarray(d32, np.float64) / grid
    fin = np.isfinite(d)
    assert np.array_equal(d[fin], np.rint(d[fin])), "not a table of ties: a distance is not a multiple of the grid"
    worst = np.where(fin, np.abs(d), 0).max(axis=1, initial=0)   # per vector, over the rows
    for j in range(len(offsets) - 1):
        assert worst[offsets[j]:offsets[j + 1]].sum() < 2 ** 24, "bag %d: a partial sum may leave the exact range" % j


def minima_by_group(d, vis, keys):
    """form 1 of b(u, .): {group key: row} from the minimum key of every group's visible rows"""
    rows = np.flatnonzero(vis)
    rows = rows[gr.key_order(d[rows], rows)]
    rows = rows[np.argsort(keys[rows], kind="stable")]
    first = np.ones(len(rows), bool)
    first[1:] = keys[rows][1:] != keys[rows][:-1]
    return {int(keys[r]): int(r) for r in rows[first]}


def minima_by_walk(d, vis, keys):
    """form 2: the visible rows in ascending key order, the first row of every group recorded"""
    rows = np.flatnonzero(vis)
    out = {}
    for r in rows[gr.key_order(d[rows], rows)].tolist():
        out.setdefault(int(keys[r]), r)
    return out


def seq_sum(terms, start=F(0.0)):
    s = F(start)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in terms:
            s = F(s + F(x))
    return s


def score_order(scores, gkeys):
    """positions in ascending (score, group key) order, NaN after +inf"""
    s = np.asarray(scores, F) + F(0)
    nan = np.isnan(s)
    return np.lexsort((np.asarray(gkeys, np.int64), np.where(nan, F(0), s), nan))


def minima_all(d32, vis, keys, minima=None):
    """b(u, .) for every vector u: a list of {group key: row}, both forms computed and compared"""
    best = []
    for u in range(len(d32)):
        a, b = minima_by_group(d32[u], vis[u], keys), minima_by_walk(d32[u], vis[u], keys)
        assert a == b, "the two forms of the rule disagree on vector %d" % u
        best.append(a if minima is None else minima(d32[u], vis[u], keys))
    return best


def numpy_multi(d32, vis, keys, offsets, k, cand_keys=None, cand_offsets=None, minima=None, summed=seq_sum, best=None):
    """d32, vis [T][n]; keys [n]; offsets [nq + 1].  Returns (group_keys [nq][k], score [nq][k], counts [nq], match_rows [k * T], match_dist
    [k * T]) with ROW numbers in match_rows.  best: minima_all of the same (d32, vis, keys), where a caller asks for several k or lists"""
    d32 = np.asarray(d32, F)
    T, n = d32.shape
    keys = np.asarray(keys, np.int64)
    vis = np.broadcast_to(np.ones((1, 1), bool) if vis is None else np.asarray(vis, bool), (T, n))
    offsets = np.asarray(offsets, np.int64)
    nq = len(offsets) - 1
    assert offsets[0] == 0 and offsets[-1] == T and keys.shape == (n,)
    gk = np.zeros((nq, k), np.int64)
    score = np.full((nq, k), np.inf, F)
    counts = np.zeros(nq, np.int32)
    mrow = np.full(k * T, -1, np.int64)
    mdist = np.full(k * T, np.inf, F)
    if best is None:
        best = minima_all(d32, vis, keys, minima)
    known = set(keys.tolist())
    for j in range(nq):
        lo, hi = int(offsets[j]), int(offsets[j + 1])
        t = hi - lo
        if t == 0:
            continue
        if cand_keys is None:
            groups = sorted(known)
        else:
            mine = np.asarray(cand_keys, np.int64) if cand_offsets is None else np.asarray(cand_keys, np.int64)[cand_offsets[j]:cand_offsets[j + 1]]
            groups = sorted(set(mine.tolist()) & known)
        groups = [g for g in groups if all(g in best[u] for u in range(lo, hi))]
        if not groups:
            continue
        rows = np.array([[best[u][g] for u in range(lo, hi)] for g in groups], np.int64)   # [groups][t]: the row of b(u, g)
        terms = d32[np.arange(lo, hi)[None, :], rows]
        if summed is seq_sum:   # the same adds in the same order, all groups at once
            sc = np.zeros(len(groups), F)
            with np.errstate(invalid="ignore", over="ignore"):
                for c in range(t):
                    sc = (sc + terms[:, c]).astype(F)
        else:
            sc = np.array([summed(list(row)) for row in terms], F)
        order = score_order(sc, groups)[:k]
        m = counts[j] = len(order)
        gk[j, :m] = np.array(groups, np.int64)[order]
        score[j, :m] = sc[order]
        mrow[k * lo:k * lo + m * t] = rows[order].reshape(-1)          # slot s, vector u at k * lo + s * t + u
        mdist[k * lo:k * lo + m * t] = terms[order].reshape(-1) + F(0)   # (key_dist of a key: -0 reads as +0)
    return gk, score, counts, mrow, mdist


NAMES = ("group_keys", "score", "counts", "match_ids", "match_dist")


def same(got, want, what=""):
    """group keys, score bits (a NaN equals a NaN), counts, match ids, match distance bits: equality, position by position"""
    for x, y, name in zip(got, want, NAMES):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, "%s %s: shape %s != %s" % (what, name, x.shape, y.shape)
        if name in ("score", "match_dist"):
            x, y = (np.where(np.isnan(a), np.uint32(0xFFC00000), np.ascontiguousarray(a, F).view(np.uint32)) for a in (x, y))   # (raw bits: -0 is not +0)
        bad = np.argwhere(x != y)
        assert len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def check_multi(got, d32, vis, keys, offsets, k, cand_keys=None, cand_offsets=None, base=0, stride=1, what="", best=None):
    """got as the call returns it, match ids under the id map (base, stride)"""
    gk, score, counts, mrow, mdist = numpy_multi(d32, vis, keys, offsets, k, cand_keys, cand_offsets, best=best)
    same(got, (gk, score, counts, np.where(mrow >= 0, mrow * stride + base, -1), mdist), what)


def matches(flat, offsets, k, j):
    """bag j's [k, t_j] view of a flat match array"""
    lo, t = int(offsets[j]), int(offsets[j + 1] - offsets[j])
    return np.asarray(flat)[k * lo:k * (lo + t)].reshape(k, t)
