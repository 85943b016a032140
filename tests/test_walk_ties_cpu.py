"""tests/walk_ref.py on the CPU: the conditions on the inputs hold for every case tests/test_gpu_traverse_ties.py runs (one case list, defined
in walk_ref.py), the comparator rejects the faults that helpers.assert_topk_match lets through, and the oracle's SearchImpl is itself
the reference's on tables of ties (T = 1, the compiled reference - which side is right when the device and the oracle disagree)."""
import numpy as np
import pytest

import walk_ref as wr
from helpers import assert_topk_match


def _stand_in_graph(n):
    """case 3 walks a graph the device builds; here a random CSR stands in for it (24 random out-edges and the next row per node): what the
    conditions ask of the TABLE - exact distances, ties - does not depend on which valid graph is walked"""
    rng = np.random.default_rng([3, n])
    nb = np.concatenate([rng.integers(0, n, (n, 24)), ((np.arange(n) + 1) % n)[:, None]], axis=1).astype(np.int64)
    return np.arange(n + 1, dtype=np.int64) * 25, nb.reshape(-1), 0


def _walk(oracle, c):
    graph = _stand_in_graph(c["n"]) if c["graph"] == "device" else None
    X, Q, off, nbr, nav = wr.case_inputs(c, oracle, graph)
    return X, Q, wr.oracle_walks(oracle, c, graph, tag="stand-in" if graph else None)


@pytest.mark.parametrize("group", ["queue", "width", "large", "shape"])
def test_preconditions_hold_for_every_gpu_case(oracle, group):
    cases = [c for c in wr.all_walk_cases() if c["group"] == group]
    assert cases
    for c in cases:
        X, Q, res = _walk(oracle, c)
        share = wr.preconditions(c, res, X, Q, wr.case_id(c))
        assert share >= wr.TIE_FLOOR


def test_preconditions_hold_for_the_search_case(oracle):
    c = wr.SEARCH_CASE
    X, Q, off, nbr, nav, dele, col = wr.search_inputs(oracle)
    for T in (1, 4):
        res = wr.oracle_searches(oracle, T)
        wr.preconditions(dict(compared=c["limit"], metric=c["metric"]), res, X, Q, "search T%d" % T)
        assert wr.border_ties(res, c["n"]) >= 1, "no tie between a graph row and a tail row in any result"
        for ids, dist, ev in res:          # the post-filter had something to drop and something to keep
            assert len(ids) == c["limit"] and (ids % c["every"] != 0).all() and (col[ids] >= c["value"]).all()
            assert (ids >= c["n"]).any() and (ids < c["n"]).any()


def test_case_list_covers_what_it_claims():
    """every metric meets a width in the 16-byte form and one in the scalar form; every distance-phase form of the kernel has a width"""
    cs = wr.width_cases()
    for m in (0, 1, 2):
        ds = {c["d"] for c in cs if c["metric"] == m}
        assert any(d % 4 == 0 for d in ds) and any(d % 4 for d in ds), (m, ds)
    ds = {c["d"] for c in cs}
    assert ds == set(wr.WIDTHS)
    assert any(d <= 128 for d in ds) and any(d > 128 and d % 4 == 0 and d < 768 for d in ds) and any(d > 1024 for d in ds)
    assert any(c.get("tiled", 0) > 256 for c in cs)
    assert {(c["T"], c["L"], c["I"]) for c in wr.queue_cases()} == set(wr.QUEUE_PARAMS)
    assert len({wr.case_id(c) for c in wr.all_walk_cases()}) == len(wr.all_walk_cases())


# ------------------------------------------------------------------------------------------------ the comparator can fail
def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_comparator_rejects_what_the_tolerance_accepts(oracle, metric):
    """The gap this file closes, stated as the assertion: a swap inside a tie group and a foreign row of equal distance at rank k pass
    helpers.assert_topk_match (distances agree, the set differs by at most the allowed one) and are rejected by assert_same_walk; an
    evaluation count off by one passes the eval-count slack of the tolerance tests and is rejected by same_evals."""
    c = [c for c in wr.queue_cases() if c["metric"] == metric and (c["T"], c["L"], c["I"]) == (1, 100, 4)][0]
    X, Q, res = _walk(oracle, c)
    L, Lq, k = wr.effective(c)
    swaps = foreign = 0
    for qi, (oid, od, ev) in enumerate(res):
        ids, dist = oid[:k].copy(), od[:k].copy()
        wr.assert_same_walk(ids, dist, k, oid, od, k, "clean q%d" % qi)
        assert_topk_match(ids, dist, oid[:k], od[:k])
        # 1. two ids swapped inside a tie group
        pos = np.flatnonzero(dist[1:] == dist[:-1])
        if len(pos):
            p = int(pos[len(pos) // 2])
            m = ids.copy()
            m[p], m[p + 1] = m[p + 1], m[p]
            assert_topk_match(m, dist, oid[:k], od[:k], what="swap")
            msg = _rejected(wr.assert_same_walk, m, dist, k, oid, od, k, "swap q%d" % qi)
            assert msg and "rank %d" % p in msg and "tie group" in msg, msg
            swaps += 1
        # 2. the id at rank k replaced by a row of equal distance that is not in the queue
        d64 = wr.xr.dist64(X, Q[qi][None, :], metric)[:, 0]
        out = np.setdiff1d(np.flatnonzero(d64 == np.float64(dist[k - 1])), oid)
        if len(out):
            m = ids.copy()
            m[k - 1] = out[0]
            assert_topk_match(m, dist, oid[:k], od[:k], what="foreign")
            msg = _rejected(wr.assert_same_walk, m, dist, k, oid, od, k, "foreign q%d" % qi)
            assert msg and "rank %d" % (k - 1) in msg, msg
            foreign += 1
        # a distance that differs in its last bit, a short count, a NaN, a non-empty tail
        m = dist.copy()
        m[k // 2] = np.nextafter(m[k // 2], np.float32(np.inf))
        assert _rejected(wr.assert_same_walk, ids, m, k, oid, od, k)
        assert _rejected(wr.assert_same_walk, ids, dist, k - 1, oid, od, k)
        m = dist.copy()
        m[0] = np.nan
        assert _rejected(wr.assert_same_walk, ids, m, k, oid, od, k)
        assert _rejected(wr.assert_same_walk, np.append(ids, 7), np.append(dist, np.float32(np.inf)), k, oid, od, k)
        wr.assert_same_walk(np.append(ids, -1), np.append(dist, np.float32(np.inf)), k, oid, od, k)
    assert swaps >= len(res) // 2 and foreign >= 1, (swaps, foreign)
    # 3. an evaluation count off by one
    total = sum(r[2] for r in res)
    wr.same_evals(total, total)
    assert abs((total + 1) - total) <= max(2, total // 200)          # (what _close_evals of test_gpu_traverse.py lets through)
    assert _rejected(wr.same_evals, total + 1, total) and _rejected(wr.same_evals, total - 1, total)


def test_zero_signs_are_one_distance():
    oid, od = np.arange(3), np.array([0.0, 0.0, 1.0], np.float32)
    wr.assert_same_walk(oid, np.array([-0.0, 0.0, 1.0], np.float32), 3, oid, od, 3)


def test_preconditions_can_fail(oracle):
    """a continuous table is turned away by condition 2, a table fp32 does not compute exactly by condition 1"""
    c = wr.queue_cases()[0]
    X, Q, off, nbr, nav = wr.case_inputs(c, oracle)
    init = oracle.prepare_init_ids(off, nbr, nav, c["L"])
    rng = np.random.default_rng(1)
    Xc, Qc = rng.random(X.shape, dtype=np.float32), rng.random(Q.shape, dtype=np.float32)
    res = [oracle.search_impl(0, Xc, off, nbr, init, q, T=1, L=c["L"], lockstep=True) for q in Qc[:4]]
    msg = _rejected(wr.preconditions, c, res, Xc, Qc[:4])
    assert msg and ("fp64" in msg or "ties" in msg), msg
    Xh = (X + np.float32(0.5)) * np.float32(1.0 / 3.0)
    res = [oracle.search_impl(0, Xh, off, nbr, init, q, T=1, L=c["L"], lockstep=True) for q in Q[:4]]
    msg = _rejected(wr.preconditions, c, res, Xh, Q[:4])
    assert msg and "fp64" in msg, msg


# ------------------------------------------------------------------------------------------------ the oracle against the compiled reference
@pytest.mark.ref
@pytest.mark.parametrize("shape", ["plain", "long"])
@pytest.mark.parametrize("L", [100, 500])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_oracle_is_the_reference_on_ties_T1(oracle, ref, metric, L, shape):
    """The reference's own SearchImpl (compiled verbatim) and the oracle's restatement at T = 1 on the narrow tie table: the whole master
    queue, ids and distances, and the number of distance evaluations, bit for bit.  This is the arbiter when the device and the oracle
    disagree on a tie (tests/test_oracle_vs_ref.py::test_search_impl_T1_bit_exact and test_dist_eval_count_T1 do the same on continuous rows)."""
    c = dict(wr.queue_cases()[0], metric=metric, T=1, L=L, Lq=L, shape=shape, k=L)
    X, Q, off, nbr, nav = wr.case_inputs(c, oracle)
    X = np.ascontiguousarray(X)
    g = ref.graph_from_arrays(off, nbr, nav)
    ex = ref.executor(g, X, metric=metric, T=1, L=L, count=True)
    init = oracle.prepare_init_ids(off, nbr, nav, L)
    assert np.array_equal(ref.init_ids(ex, L), init)
    res = []
    for qi, q in enumerate(Q):
        ref.L.ref_dist_calls_reset()
        rid, rd = ref.search_impl(ex, np.ascontiguousarray(q), L)
        ev_ref = ref.L.ref_dist_calls_reset()
        oid, od, ev = oracle.search_impl(metric, X, off, nbr, init, q, T=1, L=L)
        res.append((oid, od, ev))
        wr.assert_same_walk(rid, rd, L, oid, od, L, "reference vs oracle m%d L%d %s q%d" % (metric, L, shape, qi))
        assert np.array_equal(rd.view(np.uint32), od.view(np.uint32)), qi
        wr.same_evals(ev_ref, ev, "q%d" % qi)
        lid, ld, lev = oracle.search_impl(metric, X, off, nbr, init, q, T=1, L=L, lockstep=True)      # one worker: both schedules are one walk
        assert np.array_equal(lid, oid) and np.array_equal(ld.view(np.uint32), od.view(np.uint32)) and lev == ev
    ref.L.ref_executor_free(ex)
    ref.L.ref_graph_free(g)
    wr.preconditions(c, res, X, Q, "reference vs oracle")
