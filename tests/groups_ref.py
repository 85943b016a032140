"""What an answer of GpuIndex.search_groups (eps_index_search_groups) is held to, in numpy: for tests/test_groups_ref_cpu.py (fed with hand-written
cases and planted faults) and tests/test_gpu_groups.py (fed with what the device returns).  Nothing here is fitted to device output.

The rule, for query j.  V_j = the visible rows.  Every group (rows with equal int64 keys) with a row in V_j is represented by its row of V_j with
the smallest (distance, row) key - NaN after +inf, ties to the smaller row - and the answer is the k smallest representatives in ascending key
order.  Equivalently: walk V_j in ascending key order, keep a row iff its group has not been seen, stop at k.  numpy_groups computes both forms
and asserts that they agree.

The yardstick tables are tables of ties: small-integer coordinates (or those / 16) for which every fp32 sum is exact in any order, so the device's
distance IS the fp64 distance and (distance, row) order is decided with no band.  assert_ties_table checks that condition on the inputs before
the model is used as a yardstick, as walk_ref does."""
import numpy as np

import exact_ref as er
import range_ref as rr

F = np.float32
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
TIES = {0: "integers -8..8", 1: "integers / 16", 2: "integers -8..8"}   # metric -> exact_ref table


def assert_ties_table(X, Q, metric):
    """every coordinate a small integer (/ 16 for COSINE) and every fp32 distance equal to the fp64 one; returns the fp32 distances [n][nq]"""
    X, Q = np.asarray(X, F), np.atleast_2d(np.asarray(Q, F))
    scale = 16 if metric == 1 else 1
    for a in (X, Q):
        v = a.astype(np.float64) * scale
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max(initial=0) <= 8, "not a table of ties: coordinates must be integers -8..8 (/ 16 for COSINE)"
    d64 = er.dist64(X, Q, metric)
    d32 = d64.astype(F)
    assert np.array_equal(d32.astype(np.float64), d64), "not a table of ties: a distance is not an fp32 number"
    assert np.array_equal(rr.dist32(X, Q, metric).astype(np.float64), d64), "not a table of ties: numpy's fp32 sum differs from the fp64 one"
    return d32


def ties_table(metric, n, d, nq, seed=0):
    X, Q = er.make(TIES[metric], n, d, nq, seed=seed)
    return X, Q, assert_ties_table(X, Q, metric)


def key_order(d, rows):
    """positions of `rows` in ascending (distance, row) order, NaN after +inf"""
    d = np.asarray(d, F) + F(0)
    nan = np.isnan(d)
    return np.lexsort((rows, np.where(nan, F(0), d), nan))


def by_representatives(d, vis, keys, k):
    """form 1: the representative of every group with a visible row, then the k smallest; rows in answer order"""
    rows = np.flatnonzero(vis)
    rows = rows[key_order(d[rows], rows)]                # ascending key order ...
    rows = rows[np.argsort(keys[rows], kind="stable")]   # ... kept inside every group: a group's first row is its representative
    first = np.ones(len(rows), bool)
    first[1:] = keys[rows][1:] != keys[rows][:-1]
    reps = rows[first]
    return reps[key_order(d[reps], reps)][:k]


def by_walk(d, vis, keys, k):
    """form 2: the visible rows in ascending key order, a row kept iff its group has not been seen, until k are kept"""
    rows = np.flatnonzero(vis)
    seen, out = set(), []
    for r in rows[key_order(d[rows], rows)].tolist():
        g = int(keys[r])
        if g not in seen:
            seen.add(g)
            out.append(r)
            if len(out) == k:
                break
    return np.array(out, np.int64)


def numpy_groups(d32, keys, k, visible=None):
    """the answer from fp32 distances d32 [n][nq] and int64 keys [n]: (ids [nq][k] ROW numbers, dist [nq][k], group_keys [nq][k], counts [nq])"""
    n, nq = d32.shape
    keys = np.asarray(keys, np.int64)
    assert keys.shape == (n,)
    vis = rr.visible2(n, nq, visible)
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F)
    gk = np.zeros((nq, k), np.int64)
    counts = np.zeros(nq, np.int32)
    for q in range(nq):
        a = by_representatives(d32[:, q], vis[:, q], keys, k)
        b = by_walk(d32[:, q], vis[:, q], keys, k)
        assert np.array_equal(a, b), "the two forms of the rule disagree on query %d" % q
        m = counts[q] = len(a)
        ids[q, :m] = a
        dist[q, :m] = d32[a, q]
        gk[q, :m] = keys[a]
    return ids, dist, gk, counts


def bits(x):
    return (np.asarray(x, F) + F(0)).view(np.uint32)


def same(got, want, what=""):
    """ids, distance bits (a NaN equals a NaN), group keys, counts: equality, position by position"""
    for x, y, name in zip(got, want, ("ids", "dist", "group_keys", "counts")):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, "%s %s: shape %s != %s" % (what, name, x.shape, y.shape)
        if name == "dist":
            x, y = np.where(np.isnan(x), np.uint32(0xFFC00000), bits(x)), np.where(np.isnan(y), np.uint32(0xFFC00000), bits(y))
        bad = np.argwhere(x != y)
        assert len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def check_groups(got, d32, keys, k, visible=None, base=0, stride=1, what=""):
    """got = (ids, dist, group_keys, counts) as the call returns them, ids under the id map (base, stride)"""
    ids, dist, gk, counts = numpy_groups(d32, keys, k, visible)
    same(got, (np.where(ids >= 0, ids * stride + base, -1), dist, gk, counts), what)


# ---- group layouts over n rows (the GPU tests and the CPU tests share them)
def layouts(n, seed=0):
    rng = np.random.default_rng([seed, n])
    zipf = np.minimum(rng.zipf(1.3, n), max(n // 2, 1)).astype(np.int64)   # a few large groups, a long tail of small ones
    return {
        "one group": np.full(n, 42, np.int64),
        "every row its own": rng.permutation(n).astype(np.int64) * 1000003 - 500,
        "n / 8 groups": rng.integers(0, max(n // 8, 1), n).astype(np.int64),
        "zipf": zipf,
        "extreme keys": np.array([I64_MIN, -1, 0, I64_MAX], np.int64)[rng.integers(0, 4, n)],
    }
