"""What an answer of GpuIndex.search_range (eps_index_search_range) is held to, in numpy: for tests/test_range_ref_cpu.py (fed with numpy's own fp32
answer and with planted faults) and tests/test_gpu_search_range.py (fed with what the device returns).  Nothing here is fitted to device output.

A row belongs to query j's answer iff it is visible and its exact fp32 distance is <= radius[j].  From exact_ref.Ref - fp64 distances d64 and the
allowed error B of ONE fp32 distance - every (row, query) is one of
    a certain member       visible and d64 + B < r
    a certain non-member   hidden, or d64 - B > r
    undecided              the band between them: fp32 may put it on either side.
check_range holds a result to:  1 structure - unique visible ids inside the table, the -1 / +inf tail, counts = min(totals, cap);  2 every returned
distance within B of the fp64 distance of its row, and <= r in fp32;  3 (distance, id) strictly increasing;  4 totals within [#certain,
#certain + #undecided], and - total <= cap - every certain member present, no certain non-member; - total > cap - the rows held to
exact_ref.check_topk with k = cap.  It returns (undecided rows, certain members) summed over the queries: the caller asserts the cap
exact_ref.CAP on their ratio - a condition on the TABLE, not a measurement.  Tables of small integers have no band: numpy_range is the answer."""
import numpy as np

import exact_ref as er

F = np.float32


def dist32(X, Q, metric):
    """numpy's own fp32 distances [n][nq] (pairwise sums: within the order-free bound); exact on tables of small integers"""
    X, Q = np.asarray(X, F), np.atleast_2d(np.asarray(Q, F))
    out = np.empty((len(X), len(Q)), F)
    for q in range(len(Q)):
        if metric == 0:
            diff = X - Q[q]
            out[:, q] = (diff * diff).sum(axis=1, dtype=F)
        else:
            acc = (X * Q[q]).sum(axis=1, dtype=F)
            out[:, q] = F(1) - acc if metric == 1 else -acc
    return out + F(0)


def visible2(n, nq, visible):
    """visible: None, bool [n], row numbers, or bool [n][nq] (a program that reads @distance judges per query) -> bool [n][nq]"""
    v = np.asarray(visible) if visible is not None else None
    if v is not None and v.dtype == bool and v.ndim == 2:
        assert v.shape == (n, nq)
        return v
    return np.repeat(er._visible(n, visible)[:, None], nq, axis=1)


def numpy_range(d32, radius, cap, visible=None):
    """the answer from fp32 distances d32 [n][nq]: (ids [nq][cap], dist [nq][cap], counts [nq], totals [nq]), ids = row numbers"""
    n, nq = d32.shape
    vis = visible2(n, nq, visible)
    radius = np.broadcast_to(np.asarray(radius, F), (nq,))
    ids = np.full((nq, cap), -1, np.int64)
    dist = np.full((nq, cap), np.inf, F)
    counts = np.zeros(nq, np.int32)
    totals = np.zeros(nq, np.int64)
    for q in range(nq):
        rows = np.flatnonzero(vis[:, q] & (d32[:, q] <= radius[q]))
        rows = rows[np.lexsort((rows, d32[rows, q]))]
        totals[q] = len(rows)
        m = counts[q] = min(len(rows), cap)
        ids[q, :m] = rows[:m]
        dist[q, :m] = d32[rows[:m], q]
    return ids, dist, counts, totals


def split(ref, radius, visible=None, bound="free", vec4=None):
    """(certain members, certain non-members, undecided) as bool [n][nq], from the fp64 reference alone"""
    vis = visible2(ref.n, ref.nq, visible)
    B = ref.bound(bound, vec4)
    r = np.broadcast_to(np.asarray(radius, F), (ref.nq,)).astype(np.float64)[None, :]
    must = vis & (ref.d64 + B < r)
    never = ~vis | (ref.d64 - B > r)
    return must, never, ~must & ~never


def check_range(ids, dist, counts, totals, ref, radius, cap, visible=None, bound="free", vec4=None, what=""):
    """ids [nq][cap] are ROW numbers (undo an id map first).  Returns (undecided rows, certain members) over the queries."""
    ids, dist, counts, totals = np.asarray(ids), np.asarray(dist), np.asarray(counts), np.asarray(totals)
    n, nq = ref.n, ref.nq
    assert ids.shape == (nq, cap) and dist.shape == (nq, cap) and counts.shape == (nq,) and totals.shape == (nq,), "%s: shapes" % what
    radius = np.broadcast_to(np.asarray(radius, F), (nq,))
    vis = visible2(n, nq, visible)
    B = ref.bound(bound, vec4)
    must, never, und = split(ref, radius, vis, bound, vec4)
    n_und = n_must = 0
    for q in range(nq):
        m, total = int(counts[q]), int(totals[q])
        assert m == min(total, cap), "%s query %d: count %d, total %d, cap %d" % (what, q, m, total, cap)
        r = np.asarray(ids[q, :m], np.int64)
        assert (r >= 0).all() and (r < n).all(), "%s query %d: id outside the table: %s" % (what, q, r[(r < 0) | (r >= n)][:4])
        uq, c = np.unique(r, return_counts=True)
        assert len(uq) == m, "%s query %d: row %d is returned %d times" % (what, q, uq[c > 1][0] if (c > 1).any() else -1, c.max(initial=0))
        assert vis[r, q].all(), "%s query %d: row %d is not visible" % (what, q, r[~vis[r, q]][0] if (~vis[r, q]).any() else -1)
        assert (ids[q, m:] == -1).all() and np.isposinf(dist[q, m:]).all(), "%s query %d: the tail is not -1 / +inf" % (what, q)
        d32 = np.asarray(dist[q, :m], F)
        err = np.abs(d32.astype(np.float64) - ref.d64[r, q])
        bad = np.flatnonzero(~(err <= B[r, q]))
        assert len(bad) == 0, "%s query %d rank %d row %d: distance %r, fp64 %r, |error| %.3g > bound %.3g" % (
            what, q, bad[0], r[bad[0]], d32[bad[0]], ref.d64[r[bad[0]], q], err[bad[0]], B[r[bad[0]], q])
        bad = np.flatnonzero(~(d32 <= radius[q]))
        assert len(bad) == 0, "%s query %d rank %d row %d: distance %r beyond the radius %r" % (what, q, bad[0], r[bad[0]], d32[bad[0]], radius[q])
        er._ordered(r, d32, q, what)
        nm, nu = int(must[:, q].sum()), int(und[:, q].sum())
        n_must += nm
        n_und += nu
        assert nm <= total <= nm + nu, "%s query %d: total %d outside [%d certain members, + %d undecided]" % (what, q, total, nm, nu)
        if total <= cap:
            got = np.zeros(n, bool)
            got[r] = True
            miss = np.flatnonzero(must[:, q] & ~got)
            assert len(miss) == 0, "%s query %d: row %d (fp64 %r, bound %.3g, radius %r) is not returned (%d rows missing)" % (
                what, q, miss[0], ref.d64[miss[0], q], B[miss[0], q], radius[q], len(miss))
            extra = np.flatnonzero(never[:, q] & got)
            assert len(extra) == 0, "%s query %d: row %d (fp64 %r, bound %.3g) lies beyond the radius %r or is hidden (%d such rows)" % (
                what, q, extra[0], ref.d64[extra[0], q], B[extra[0], q], radius[q], len(extra))
        else:   # the cap closest visible rows (all of them within the radius: more than cap rows are)
            n_und += er.check_topk(ids[q:q + 1], dist[q:q + 1], counts[q:q + 1], None, None, ref.metric, cap, visible=vis[:, q], bound=bound, vec4=vec4,
                                   ref=ref.take([q]), what="%s query %d (total %d > cap)" % (what, q, total))
    return n_und, n_must


def assert_cap(n_und, n_must, what=""):
    assert n_und <= er.CAP * n_must, "%s: %d undecided rows against %d certain members: more than %.0f %% - change the TABLE or the radii, not the cap" % (
        what, n_und, n_must, 100 * er.CAP)


def midway_radii(ref, k, visible=None):
    """per query the fp64 distance midway between its k-th and (k + 1)-th visible neighbour, as fp32: the widest gap a radius can sit in"""
    vis = visible2(ref.n, ref.nq, visible)
    out = np.empty(ref.nq, F)
    for q in range(ref.nq):
        d = np.sort(ref.d64[vis[:, q], q])
        out[q] = F(0.5 * (d[k - 1] + d[k]))
    return out
