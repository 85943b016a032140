"""What an EXACT answer of the library is held to: a plain fp64 reference of the three distances and a contract on the top-k built from it, for
tests/test_exact_ref_cpu.py (fed with the fp32 oracle and with planted faults) and tests/test_gpu_exact_pin.py (fed with what GpuIndex.search
returns).  numpy float64 / int64 only; nothing here is fitted to device output.

The allowed error of ONE fp32 distance, u = 2^-24, gamma(m) = m u / (1 - m u), mag = the sum of the magnitudes of the d terms
(sum (x - q)^2 for L2 - the distance itself -, sum |x q| for the two dot metrics):

  order-free   |computed - exact| <= gamma(d + 3) mag.  Any summation order of d terms built from fmas and adds puts at most d - 1 additions
               on a path, each product or fma rounds once, L2 squares a rounded x - q (2u), one spare.  It does not know the kernel's order:
               every engine and any later rewrite must meet it.
  tree         the DOCUMENTED order (the comment over group_lanes in device_common.hpp): G lanes per row, G
               the smallest power of two with 4 G >= d (16-byte form) or G >= d (scalar form), capped at 64; each lane one chain of fmas over
               its pieces, then log2 G adds across the lanes:  m = 4 ceil(d / 4G) + log2 G + 3  (scalar: ceil(d / G) + log2 G + 3).  Restated
               here from the documentation, not imported from the library: a change of the tree has to change tree_terms() knowingly.
  COSINE       + u |1 - acc| for the final subtraction (DOT_PRODUCT's negation is exact).

check_topk holds a result to:  1 counts, unique visible ids, the -1 / +inf tail;  2 every distance within the bound of the fp64 distance of
the row it comes with;  3 (distance, id) pairs strictly increasing - equal fp32 distances in id order;  4 with t the k-th smallest visible
fp64 distance: every row with d64 + B(row) < t - B(kth) is there, none with d64 - B(row) > t + B(kth).  Rows in between may go either way:
where the band leaves a choice open they are counted as UNDECIDED and returned, so that the caller can cap what the band may hide.
check_exact (tables of small integers: fp32 is exact in any order) has no band at all."""
import math

import numpy as np

import mirror_ref as mr

F = np.float32
U = 2.0 ** -24
CHUNK = 8192          # rows per block of the fp64 reference (200k x 768 stays within a few hundred MB)
CAP = 0.05            # undecided rows <= 5 % of k x queries on every table that is held to check 4


def gamma(m):
    return m * U / (1.0 - m * U)


def group_lanes(d, vec4):
    need = (d + 3) // 4 if vec4 else d
    g = 1
    while g < 64 and g < need:
        g *= 2
    return g


def free_terms(d):
    return d + 3


def tree_terms(d, vec4=None):
    """roundings on the longest path of the documented tree; vec4 None: the 16-byte form iff d % 4 == 0 (rows 16-byte aligned)"""
    vec4 = (d % 4 == 0) if vec4 is None else vec4
    g = group_lanes(d, vec4)
    chain = 4 * math.ceil(d / (4.0 * g)) if vec4 else math.ceil(d / float(g))
    return chain + int(math.log2(g)) + 3


class Ref:
    """fp64 distances d64 [n][nq] and term magnitudes mag [n][nq] of one (table, queries, metric): computed once, used across k and engines"""

    def __init__(self, X, Q, metric):
        X, Q = np.asarray(X), np.atleast_2d(np.asarray(Q))
        self.n, self.d, self.nq, self.metric = len(X), X.shape[1], len(Q), metric
        self.d64 = dist64(X, Q, metric)
        self.mag = self.d64 if metric == 0 else mag64(X, Q, metric)

    def take(self, queries):
        """the same reference for a subset of its queries"""
        r = object.__new__(Ref)
        r.n, r.d, r.metric = self.n, self.d, self.metric
        r.d64 = np.ascontiguousarray(self.d64[:, queries])
        r.mag = r.d64 if self.metric == 0 else np.ascontiguousarray(self.mag[:, queries])
        r.nq = r.d64.shape[1]
        return r

    def bound(self, which="free", vec4=None):
        m = free_terms(self.d) if which == "free" else tree_terms(self.d, vec4)
        e = gamma(m) * self.mag
        if self.metric == 1:
            e = e + U * (np.abs(self.d64) + e)
        return e


def dist64(X, Q, metric):
    """mirror_ref.dist64 in blocks of rows"""
    X, Q = np.asarray(X), np.atleast_2d(np.asarray(Q))
    out = np.empty((len(X), len(Q)), np.float64)
    for r0 in range(0, len(X), CHUNK):
        out[r0:r0 + CHUNK] = mr.dist64(X[r0:r0 + CHUNK], Q, metric)
    return out


def mag64(X, Q, metric):
    """sum of the magnitudes of the d terms of a distance, [n][nq]"""
    if metric == 0:
        return dist64(X, Q, 0)
    X, Q = np.asarray(X), np.atleast_2d(np.asarray(Q))
    aq = np.abs(Q.astype(np.float64)).T
    out = np.empty((len(X), len(Q)), np.float64)
    for r0 in range(0, len(X), CHUNK):
        out[r0:r0 + CHUNK] = np.abs(X[r0:r0 + CHUNK].astype(np.float64)) @ aq
    return out


def _visible(n, visible):
    if visible is None:
        return np.ones(n, bool)
    v = np.asarray(visible)
    if v.dtype == bool:
        assert len(v) == n
        return v
    m = np.zeros(n, bool)
    m[v] = True
    return m


def _structure(ids, dist, cnt, q, k, vis, what):
    """check 1 for one query; returns the returned rows"""
    want = min(k, int(vis.sum()))
    m = int(cnt[q])
    assert m == want, "%s query %d: %d results, %d expected (k %d, %d visible rows)" % (what, q, m, want, k, int(vis.sum()))
    r = np.asarray(ids[q, :m], np.int64)
    assert (r >= 0).all() and (r < len(vis)).all(), "%s query %d: id outside the table: %s" % (what, q, r[(r < 0) | (r >= len(vis))][:4])
    uq, c = np.unique(r, return_counts=True)
    assert len(uq) == m, "%s query %d: row %d is returned %d times" % (what, q, uq[c > 1][0] if (c > 1).any() else -1, c.max(initial=0))
    assert vis[r].all(), "%s query %d: row %d is not visible (deleted or filtered)" % (what, q, r[~vis[r]][0] if (~vis[r]).any() else -1)
    assert (np.asarray(ids[q, m:]) == -1).all() and np.isposinf(np.asarray(dist[q, m:])).all(), "%s query %d: the tail is not -1 / +inf" % (what, q)
    return r


def _ordered(r, d32, q, what):
    """check 3: strictly increasing as (distance, id) pairs"""
    if len(r) < 2:
        return
    ok = (d32[:-1] < d32[1:]) | ((d32[:-1] == d32[1:]) & (r[:-1] < r[1:]))
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, "%s query %d: ranks %d, %d out of order: (%r, row %d) then (%r, row %d)" % (
        what, q, bad[0], bad[0] + 1, d32[bad[0]], r[bad[0]], d32[bad[0] + 1], r[bad[0] + 1])


def band(ref, q, k, vis, B):
    """(must-be-returned mask, must-not-be-returned mask, undecided count) of query q from the fp64 reference alone"""
    d, b = ref.d64[:, q], B[:, q]
    rows = np.flatnonzero(vis)
    if k >= len(rows):
        return vis.copy(), ~vis, 0
    o = rows[np.lexsort((rows, d[rows]))]
    kth = o[k - 1]
    t, bk = d[kth], b[kth]
    must = vis & (d + b < t - bk)
    never = ~vis | (d - b > t + bk)
    between = int((~must & ~never).sum())
    open_slots = k - int(must.sum())
    return must, never, (between if between > open_slots else 0)


def undecided(ref, k, visible=None, bound="free", vec4=None, queries=None):
    """rows the band leaves open over the queries, from the reference alone (the condition asserted BEFORE a device is asked)"""
    vis = _visible(ref.n, visible)
    B = ref.bound(bound, vec4)
    return sum(band(ref, q, k, vis, B)[2] for q in (range(ref.nq) if queries is None else queries))


def assert_cap(ref, k, visible=None, what=""):
    u = undecided(ref, k, visible)
    assert u <= CAP * k * ref.nq, "%s k %d: %d undecided rows over %d queries: more than %.0f %% of k x queries - change the TABLE, not the cap" % (
        what, k, u, ref.nq, 100 * CAP)
    return u


def check_topk(ids, dist, cnt, X, Q, metric, k, visible=None, bound="free", vec4=None, ref=None, membership=True, what=""):
    """ids [nq][k] are ROW numbers (undo an id map first).  bound: "free" or "tree"; vec4: which form of the tree (None: by d % 4).
    membership False: checks 1-3 only (tables that are exempt from check 4 by name).  Returns the undecided rows."""
    ref = ref if ref is not None else Ref(X, Q, metric)
    ids, dist, cnt = np.asarray(ids), np.asarray(dist), np.asarray(cnt)
    vis = _visible(ref.n, visible)
    B = ref.bound(bound, vec4)
    und = 0
    for q in range(ref.nq):
        r = _structure(ids, dist, cnt, q, k, vis, what)
        d32 = dist[q, :len(r)]
        err = np.abs(d32.astype(np.float64) - ref.d64[r, q])
        bad = np.flatnonzero(~(err <= B[r, q]))      # (a NaN is not within any bound)
        assert len(bad) == 0, "%s query %d rank %d row %d: distance %r, fp64 %r, |error| %.3g > bound %.3g (%s, %d of %d distances)" % (
            what, q, bad[0], r[bad[0]], d32[bad[0]], ref.d64[r[bad[0]], q], err[bad[0]], B[r[bad[0]], q], bound, len(bad), len(r))
        _ordered(r, d32, q, what)
        if not membership:
            continue
        must, never, u = band(ref, q, k, vis, B)
        und += u
        got = np.zeros(ref.n, bool)
        got[r] = True
        miss = np.flatnonzero(must & ~got)
        if len(miss):
            o = np.lexsort((np.arange(ref.n), np.where(vis, ref.d64[:, q], np.inf)))
            rank = int(np.flatnonzero(o == miss[0])[0])
            raise AssertionError("%s query %d: row %d (fp64 %r, bound %.3g, true rank %d of k %d) is not returned; the last returned distance is %r (%d rows missing)" % (
                what, q, miss[0], ref.d64[miss[0], q], B[miss[0], q], rank, k, d32[-1] if len(d32) else None, len(miss)))
        extra = np.flatnonzero(never & got)
        if len(extra):
            rank = int(np.flatnonzero(r == extra[0])[0])
            raise AssertionError("%s query %d rank %d: row %d (returned %r, fp64 %r, bound %.3g) lies beyond the k-th fp64 distance (%d such rows)" % (
                what, q, rank, extra[0], d32[rank], ref.d64[extra[0], q], B[extra[0], q], len(extra)))
    return und


def check_exact(ids, dist, cnt, X, Q, metric, k, visible=None, ref=None, what=""):
    """tables fp32 computes exactly: the distances are the fp64 ones bit for bit, the ids np.lexsort((row, d64))[:k] position by position"""
    ref = ref if ref is not None else Ref(X, Q, metric)
    ids, dist, cnt = np.asarray(ids), np.asarray(dist), np.asarray(cnt)
    vis = _visible(ref.n, visible)
    rows = np.flatnonzero(vis)
    assert np.array_equal(ref.d64.astype(F).astype(np.float64), ref.d64), "not an exact table: an fp64 distance is not an fp32 number"
    for q in range(ref.nq):
        r = _structure(ids, dist, cnt, q, k, vis, what)
        want = rows[np.lexsort((rows, ref.d64[rows, q]))][:k]
        wd = ref.d64[want, q].astype(F)
        d32 = np.asarray(dist[q, :len(r)], F)
        bad = np.flatnonzero((r != want) | ((d32 + F(0)).view(np.uint32) != (wd + F(0)).view(np.uint32)))      # (-0 and +0 are one distance)
        assert len(bad) == 0, "%s query %d rank %d: (row %d, %r) returned, (row %d, %r) expected; fp64 of the returned row %r (%d of %d places differ)" % (
            what, q, bad[0], r[bad[0]], d32[bad[0]], want[bad[0]], wd[bad[0]], ref.d64[r[bad[0]], q], len(bad), len(r))


def error_ratios(ids, dist, cnt, ref, vec4=None):
    """largest |d32 - d64| / B over what was returned, for the order-free and the tree bound (evidence for the log, not an assertion)"""
    out = []
    for which in ("free", "tree"):
        B = ref.bound(which, vec4)
        worst = 0.0
        for q in range(ref.nq):
            r = np.asarray(ids[q, :int(cnt[q])], np.int64)
            if len(r):
                e = np.abs(np.asarray(dist[q, :len(r)], np.float64) - ref.d64[r, q])
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(e == 0, 0.0, e / B[r, q])
                worst = max(worst, float(np.nanmax(ratio)))
        out.append(worst)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the tables (seeds fixed by the callers)
def unit(X):
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(F)


def embedding_like(rng, n, d):
    """unit rows with 8 dominant columns (tests/test_gpu_mirror_pin.py uses the same table)"""
    scale = np.ones(d, F)
    scale[:8] = 4.0
    return unit(rng.standard_normal((n, d)).astype(F) * scale)


def _outlier_rows(rng, n, d):
    X = rng.random((n, d), dtype=F)
    X[rng.choice(n, size=min(5, n), replace=False)] *= F(1e4)
    return X


def _ints(rng, n, d):
    return rng.integers(-8, 9, (n, d)).astype(F)


# name -> (rows(rng, n, d), queries(rng, nq, d), metrics, which of them are held to check 4, exact)
TABLES = {
    "uniform": (lambda r, n, d: r.random((n, d), dtype=F), lambda r, n, d: r.random((n, d), dtype=F), (0, 2), (0, 2), False),
    "uniform unit rows": (lambda r, n, d: unit(r.random((n, d), dtype=F)), lambda r, n, d: unit(r.random((n, d), dtype=F)), (1,), (1,), False),
    "gaussian": (lambda r, n, d: r.standard_normal((n, d), dtype=F), lambda r, n, d: r.standard_normal((n, d), dtype=F), (0,), (0,), False),
    "gaussian x 3 queries": (lambda r, n, d: r.standard_normal((n, d), dtype=F), lambda r, n, d: F(3) * r.standard_normal((n, d), dtype=F), (2,), (2,), False),
    "embedding-like": (embedding_like, embedding_like, (1,), (1,), False),
    # DOT_PRODUCT near 100: the sum itself is ill-conditioned against the spread of the distances (a third of k and more is undecided): checks 1-3
    "rows near 100": (lambda r, n, d: F(100) + r.random((n, d), dtype=F), lambda r, n, d: F(100) + r.random((n, d), dtype=F), (0, 2), (0,), False),
    "values ~1e-3": (lambda r, n, d: F(1e-3) * r.random((n, d), dtype=F), lambda r, n, d: F(1e-3) * r.random((n, d), dtype=F), (0, 2), (0, 2), False),
    "values ~1e+3": (lambda r, n, d: F(1e3) * r.random((n, d), dtype=F), lambda r, n, d: F(1e3) * r.random((n, d), dtype=F), (0, 2), (0, 2), False),
    "a few rows 1e4 times larger": (_outlier_rows, lambda r, n, d: r.random((n, d), dtype=F), (0, 2), (0, 2), False),
    "integers -8..8": (_ints, _ints, (0, 2), (0, 2), True),
    "integers / 16": (lambda r, n, d: _ints(r, n, d) / F(16), lambda r, n, d: _ints(r, n, d) / F(16), (1,), (1,), True),
}


def make(name, n, d, nq, seed=0):
    rows, queries = TABLES[name][:2]
    rng = np.random.default_rng([seed, n, d])
    return rows(rng, n, d), queries(rng, nq, d)


def cases(exact=None):
    """(table name, metric, held to check 4) over the table list; exact: None all, True / False only those"""
    return [(name, m, m in four) for name, (_, _, metrics, four, ex) in TABLES.items() for m in metrics if exact is None or ex == exact]
