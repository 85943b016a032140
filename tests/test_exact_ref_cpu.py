"""tests/exact_ref.py against itself, without a GPU: the contract accepts the fp32 oracle (the C restatement of the reference's own distance
functions and of BruteForceSearch) on every table of tests/test_gpu_exact_pin.py at reduced n, it rejects planted faults - a test that cannot
see these is not done -, and the band of check 4 hides at most 5 % of k x queries on every table that is held to it.

The oracle's sums follow the reference's order (four SSE lanes), not the device's tree: it is held to the ORDER-FREE bound only."""
import numpy as np
import pytest

import exact_ref as xr

F = np.float32


def oracle_topk(oracle, metric, X, Q, k):
    ids = np.full((len(Q), k), -1, np.int64)
    dist = np.full((len(Q), k), np.inf, F)
    cnt = np.zeros(len(Q), np.int32)
    for qi, q in enumerate(Q):
        rid, rd = oracle.topk_flat(metric, X, q, k)
        ids[qi, :len(rid)], dist[qi, :len(rid)], cnt[qi] = rid, rd, len(rid)
    return ids, dist, cnt


def ideal_topk(ref, k, visible=None):
    """the fp64 reference's own answer rounded to fp32: what a perfect engine returns"""
    vis = xr._visible(ref.n, visible)
    rows = np.flatnonzero(vis)
    m = min(k, len(rows))
    ids = np.full((ref.nq, k), -1, np.int64)
    dist = np.full((ref.nq, k), np.inf, F)
    for q in range(ref.nq):
        d32 = ref.d64[rows, q].astype(F) + F(0)
        o = np.lexsort((rows, d32))[:m]
        ids[q, :m], dist[q, :m] = rows[o], d32[o]
    return ids, dist, np.full(ref.nq, m, np.int32)


# ------------------------------------------------------------------------------------------------ the bounds themselves
def test_the_restated_tree_is_the_documented_one():
    """G and the roundings on the longest path, worked by hand from DESIGN.md 3.3 / the comment over group_lanes"""
    assert [xr.group_lanes(d, True) for d in (1, 4, 5, 64, 100, 256, 257, 768, 16384)] == [1, 1, 2, 16, 32, 64, 64, 64, 64]
    assert [xr.group_lanes(d, False) for d in (1, 3, 7, 33, 64, 65, 333)] == [1, 4, 8, 64, 64, 64, 64]
    assert xr.tree_terms(768) == 12 + 6 + 3 and xr.tree_terms(128) == 4 + 5 + 3 and xr.tree_terms(1000) == 16 + 6 + 3
    assert xr.tree_terms(8192) == 128 + 6 + 3 and xr.tree_terms(4) == 4 + 0 + 3
    assert xr.tree_terms(333) == 6 + 6 + 3 and xr.tree_terms(768, vec4=False) == 12 + 6 + 3 and xr.tree_terms(7) == 1 + 3 + 3
    assert 35 < xr.gamma(xr.free_terms(768)) / xr.gamma(xr.tree_terms(768)) < 45      # "about forty times tighter"
    for d in (1, 3, 7, 33, 100, 333, 768, 1000, 4100, 8192):
        assert xr.tree_terms(d) <= xr.free_terms(d) and xr.tree_terms(d, vec4=False) <= xr.free_terms(d)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_a_numpy_restatement_of_the_tree_meets_the_tree_bound(metric):
    """the documented order in numpy fp32 on signed rows (d = 768: 64 lanes, 12 terms per lane, 6 levels).  Products are rounded on their own
    here where an fma rounds once: the spare rounding of the `+ 3` is exactly that."""
    rng = np.random.default_rng(3)
    d, n, G = 768, 400, 64
    X, Q = rng.standard_normal((n, d), dtype=F), rng.standard_normal((2, d), dtype=F)
    ref = xr.Ref(X, Q, metric)
    for q in range(2):
        T = ((X - Q[q]) ** 2 if metric == 0 else X * Q[q]).astype(F)
        lanes = np.zeros((n, G), F)
        for c0 in range(0, d, 4 * G):          # lane t: columns c0 + 4 t .. c0 + 4 t + 3 of every block of 4 G columns, in order
            for e in range(4):
                lanes += T[:, c0 + e:c0 + 4 * G:4]
        while lanes.shape[1] > 1:              # the xor tree: offsets G / 2 .. 1
            h = lanes.shape[1] // 2
            lanes = (lanes[:, :h] + lanes[:, h:]).astype(F)
        acc = lanes[:, 0]
        got = acc if metric == 0 else (F(1) - acc if metric == 1 else -acc)
        err = np.abs(got.astype(np.float64) - ref.d64[:, q])
        assert (err <= ref.bound("tree")[:, q]).all(), (err / ref.bound("tree")[:, q]).max()
        assert err.max() > 0


# ------------------------------------------------------------------------------------------------ the oracle is accepted
@pytest.mark.parametrize("name,metric,four", xr.cases())
@pytest.mark.parametrize("n,d", [(3000, 128), (1500, 768), (4097, 33)])
def test_the_contract_accepts_the_fp32_oracle(oracle, name, metric, four, n, d):
    X, Q = xr.make(name, n, d, 4, seed=11)
    ref = xr.Ref(X, Q, metric)
    exact = xr.TABLES[name][4]
    for k in (1, 10, 100, n + 7):
        got = oracle_topk(oracle, metric, X, Q, k)
        if exact:
            xr.check_exact(*got, X, Q, metric, k, ref=ref, what=name)
        xr.check_topk(*got, X, Q, metric, k, ref=ref, bound="free", membership=four, what=name)


def test_the_contract_accepts_the_oracle_behind_a_visible_set(oracle):
    from helpers import bitset
    from oracle.pyoracle import make_filter
    n, d = 3000, 64
    X, Q = xr.make("gaussian", n, d, 3, seed=12)
    gone = list(range(0, n, 11))
    vis = np.ones(n, bool)
    vis[gone] = False
    flt, keep = make_filter(deleted=bitset(n, gone))
    ref = xr.Ref(X, Q, 0)
    for k in (10, 3000):
        ids = np.full((3, k), -1, np.int64)
        dist = np.full((3, k), np.inf, F)
        cnt = np.zeros(3, np.int32)
        for qi in range(3):
            rid, rd = oracle.topk_flat(0, X, Q[qi], k, flt=flt)
            ids[qi, :len(rid)], dist[qi, :len(rid)], cnt[qi] = rid, rd, len(rid)
        xr.check_topk(ids, dist, cnt, X, Q, 0, k, visible=vis, ref=ref)
        with pytest.raises(AssertionError, match="not visible|results"):
            xr.check_topk(ids, dist, cnt, X, Q, 0, k, visible=None if k > 10 else ~vis, ref=ref)


# ------------------------------------------------------------------------------------------------ planted faults are rejected
def _drop_last_column(X, Q, metric, ref, got, q, rank):
    ids, dist, cnt = (a.copy() for a in got)
    r = ids[q, rank]
    x, y = X[r].astype(np.float64), Q[q].astype(np.float64)
    term = (x[-1] - y[-1]) ** 2 if metric == 0 else -(x[-1] * y[-1])
    dist[q, rank] = F(ref.d64[r, q] - term)
    return (ids, dist, cnt), abs(term), r


@pytest.mark.parametrize("d,n", [(768, 2000), (8192, 300)])
def test_a_dropped_column_is_rejected(d, n):
    """one column missing from ONE returned distance on U[0,1) rows under L2.  d = 768: a 1.3e-3 share of the distance, thirty times the
    order-free bound.  d = 8192: a 1.2e-4 share, INSIDE the order-free bound (4.9e-4 of the distance) - the tree bound (8.2e-6) is what
    rejects it, and that is what the tree bound is for."""
    X, Q = xr.make("uniform", n, d, 2, seed=13)
    ref = xr.Ref(X, Q, 0)
    got = ideal_topk(ref, 10)
    xr.check_topk(*got, X, Q, 0, 10, ref=ref, bound="free")
    xr.check_topk(*got, X, Q, 0, 10, ref=ref, bound="tree")
    # the returned row whose last column carries the largest term (ranks 1..8: the row stays inside the top-k order or not - either way caught)
    terms = [(X[got[0][1, r], -1].astype(np.float64) - np.float64(Q[1, -1])) ** 2 for r in range(10)]
    rank = int(np.argmax(terms))
    bad, term, row = _drop_last_column(X, Q, 0, ref, got, 1, rank)
    assert term > ref.bound("tree")[row, 1], "the planted fault is below the tree bound: pick another row"
    with pytest.raises(AssertionError, match="bound|out of order"):
        xr.check_topk(*bad, X, Q, 0, 10, ref=ref, bound="tree")
    if d == 768:
        assert term > ref.bound("free")[row, 1]
        with pytest.raises(AssertionError, match="bound|out of order"):
            xr.check_topk(*bad, X, Q, 0, 10, ref=ref, bound="free")
    else:      # inside the order-free bound: with the list put back in order that bound has nothing to object to - the tree bound is what sees it
        assert term < ref.bound("free")[row, 1], "at d = 8192 the fault is meant to lie inside the order-free bound"
        o = np.lexsort((bad[0][1], bad[1][1]))
        bad[0][1], bad[1][1] = bad[0][1][o], bad[1][1][o]
        xr.check_topk(*bad, X, Q, 0, 10, ref=ref, bound="free")
        with pytest.raises(AssertionError, match="bound"):
            xr.check_topk(*bad, X, Q, 0, 10, ref=ref, bound="tree")


def _exact_case(k=50, n=4000, d=32, nq=3):
    X, Q = xr.make("integers -8..8", n, d, nq, seed=14)
    ref = xr.Ref(X, Q, 0)
    got = ideal_topk(ref, k)
    xr.check_exact(*got, X, Q, 0, k, ref=ref)
    xr.check_topk(*got, X, Q, 0, k, ref=ref, bound="tree")
    return X, Q, ref, got


def test_two_equal_distance_rows_swapped_are_rejected():
    X, Q, ref, got = _exact_case()
    ids, dist, cnt = (a.copy() for a in got)
    same = np.flatnonzero(dist[0, :-1] == dist[0, 1:])
    assert len(same), "the exact table is meant to be all ties"
    i = same[0]
    ids[0, [i, i + 1]] = ids[0, [i + 1, i]]
    with pytest.raises(AssertionError, match="out of order"):
        xr.check_topk(ids, dist, cnt, X, Q, 0, 50, ref=ref)
    with pytest.raises(AssertionError, match="expected"):
        xr.check_exact(ids, dist, cnt, X, Q, 0, 50, ref=ref)


def test_a_tied_row_dropped_at_the_k_th_place_is_rejected_on_an_exact_table():
    """the k-th place inside a group of equal distances: the band of check_topk cannot see which of the tied rows came back (their fp64
    distances are equal); check_exact can, and does"""
    X, Q, ref, _ = _exact_case()
    for k in range(20, 60):
        ids, dist, cnt = ideal_topk(ref, k + 1)
        if dist[0, k - 1] == dist[0, k]:
            break
    else:
        pytest.fail("no k with a tie across the k-th place")
    ids, dist = np.delete(ids, k - 1, axis=1), np.delete(dist, k - 1, axis=1)      # the later id of the tie instead of the earlier one
    with pytest.raises(AssertionError, match="expected"):
        xr.check_exact(ids, dist, cnt - 1, X, Q, 0, k, ref=ref)


def test_a_row_missing_from_the_head_a_duplicate_and_a_nan_first_are_rejected():
    n, d, k = 5000, 128, 10
    X, Q = xr.make("gaussian", n, d, 3, seed=15)
    ref = xr.Ref(X, Q, 0)
    wide = ideal_topk(ref, k + 1)
    got = tuple(a[:, :k].copy() if a.ndim == 2 else np.minimum(a, k) for a in wide)
    assert xr.check_topk(*got, X, Q, 0, k, ref=ref) == 0
    # the best row is not there; everything moves up and the (k+1)-th comes in
    ids, dist = wide[0][:, 1:].copy(), wide[1][:, 1:].copy()
    with pytest.raises(AssertionError, match="is not returned"):
        xr.check_topk(ids, dist, got[2], X, Q, 0, k, ref=ref)
    # a row far beyond the k-th place is returned last
    ids, dist, cnt = (a.copy() for a in got)
    far = int(np.argmax(ref.d64[:, 2]))
    ids[2, -1], dist[2, -1] = far, F(ref.d64[far, 2])
    with pytest.raises(AssertionError, match="beyond the k-th"):
        xr.check_topk(ids, dist, cnt, X, Q, 0, k, ref=ref)
    # a duplicate id
    ids, dist, cnt = (a.copy() for a in got)
    ids[1, 4], dist[1, 4] = ids[1, 3], dist[1, 3]
    with pytest.raises(AssertionError, match="returned 2 times"):
        xr.check_topk(ids, dist, cnt, X, Q, 0, k, ref=ref)
    # a short count, a tail that is not empty
    ids, dist, cnt = (a.copy() for a in got)
    cnt[0] = k - 1
    with pytest.raises(AssertionError, match="results"):
        xr.check_topk(ids, dist, cnt, X, Q, 0, k, ref=ref)
    # a row holding a NaN ranked first (what an ordinal that puts a negative NaN below every finite distance returns)
    Xn = X.copy()
    Xn[77, 5] = np.nan
    ids = np.concatenate([np.full((3, 1), 77, np.int64), got[0][:, :-1]], axis=1)
    dist = np.concatenate([np.full((3, 1), np.nan, F), got[1][:, :-1]], axis=1)
    fin = np.ones(n, bool)
    fin[77] = False
    with pytest.raises(AssertionError, match="not visible"):      # held against the finite rows: the NaN row may not be among them
        xr.check_topk(ids, dist, got[2], X, Q, 0, k, visible=fin, ref=ref)
    with pytest.raises(AssertionError, match="bound"):            # held against all rows: a NaN is within no bound
        xr.check_topk(ids, dist, got[2], Xn, Q, 0, k, ref=xr.Ref(Xn, Q, 0))


# ------------------------------------------------------------------------------------------------ the cap on what the band may hide
@pytest.mark.parametrize("name,metric,four", xr.cases(exact=False))
@pytest.mark.parametrize("n,d", [(100_000, 128), (50_000, 768)])
def test_the_band_hides_at_most_five_percent(name, metric, four, n, d):
    """a condition on the INPUTS, from the fp64 reference alone: with the order-free bound the rows that may go either way are at most 5 % of
    k x queries (16 queries; k = 10, 100, 1024).  Rows near 100 under DOT_PRODUCT do not meet it - the sum itself is ill-conditioned against
    the spread of the distances - and are exempt from check 4 BY NAME in exact_ref.TABLES; that they miss it is asserted too, so that the
    exemption cannot outlive its reason.  Unit rows made from U[0,1) values at d = 768 crowd their cosines (6 % at k = 100 with 100k rows):
    that table is used with at most 20 000 rows at that width, here and on the device."""
    if name == "uniform unit rows" and d == 768:
        n = 20_000
    X, Q = xr.make(name, n, d, 16, seed=16)
    ref = xr.Ref(X, Q, metric)
    shares = {k: xr.undecided(ref, k) / (16.0 * k) for k in (10, 100, 1024)}
    print("undecided share, %s metric %d, %d x %d: %s (tree bound: %s)" % (
        name, metric, n, d, {k: "%.2f %%" % (100 * s) for k, s in shares.items()},
        {k: "%.2f %%" % (100 * xr.undecided(ref, k, bound="tree") / (16.0 * k)) for k in (10, 100, 1024)}))
    if four:
        for k in (10, 100, 1024):
            xr.assert_cap(ref, k, what=name)
    else:
        assert min(shares.values()) > 0.25, "the table is exempt from check 4 because the band hides a third of k: it no longer does"
