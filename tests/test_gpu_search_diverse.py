"""GpuIndex.search_diverse (eps_index_search_diverse) on the device, held to tests/diverse_ref.py for EQUALITY: ids, distance bits, score bits, counts.

Tables of ties (groups_ref.ties_table: every fp32 sum exact in any order) give the pool and the pair distances D from numpy alone.  On continuous
tables the pool and d come from search(fetch_k) and D from search_among with the pool rows as queries - the parent's code, with the orientation
the rule fixes (selected row = query side) - and numpy_diverse runs the greedy loop on those bits: a fused score, a reordered update or a wrong tie
rule changes a bit somewhere.  tests/test_diverse_ref_cpu.py holds the conditions on the fixtures (the selection differs from the pool's head for
every query at lambda <= 0.75; tied best scores occur)."""
import numpy as np
import pytest

import among_ref as ar
import diverse_ref as dr
import groups_ref as gr
import select_ref as sr
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
ENGINES = (amd.FLAT_STREAM, amd.FLAT_MFMA, amd.FLAT_MFMA_I8, amd.FLAT_AUTO)
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])
TIMING = ("kernel_ms", "main_kernel_ms", "filter_ms_all")


def index(X, metric):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    if len(X):
        ix.attach_rows(X)
    return ix


def pairs_given_a_distance(counts, pool_sizes):
    """(row, selected row) pairs of a call: np - t unselected rows after the t-th selection, the last selection gathers nothing"""
    return int(sum((int(c) - 1) * int(p) - int(c) * (int(c) - 1) // 2 for c, p in zip(counts, pool_sizes) if c > 1))


# ---- 1. tables of ties: pool and D from numpy
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("n,d,nq,fetch_k,k,lams", dr.FIXTURES)
def test_ties_fixtures_equal_numpy_for_every_lambda(n, d, nq, fetch_k, k, lams, metric):
    X, Q, d32 = gr.ties_table(metric, n, d, nq, seed=3)
    ix = index(X, metric)
    pairs = dr.ties_pairs(X, metric)
    for lam in dr.LAMBDAS:
        want = dr.numpy_answer(d32, pairs, k, fetch_k, lam)
        dr.same(ix.search_diverse(Q, k, fetch_k, lam=lam), want, "lambda %g" % lam)
        dr.same(ix.search_diverse(Q, k, fetch_k, lam=lam, flat_engine="stream"), want, "lambda %g, the stream scan" % lam)
        st = ix.stats()
        assert st["main_kernel_bits"] == 32 and st["main_kernel_launches"] == 1 and st["main_kernel_rows"] == fetch_k and st["main_kernel_queries"] == nq, st
        assert st["dist_evals"] == nq * n + pairs_given_a_distance(want[3], [min(fetch_k, n)] * nq) and st["main_kernel_ms"] > 0, st
    ix.close()


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [7, 768, 1028])   # the scalar form | G = 64, three pieces per lane | G = 64, five pieces, the last partial
def test_row_widths_scalar_form_and_more_than_one_piece_per_lane(d, metric):
    X, Q, d32 = gr.ties_table(metric, 300, d, 3, seed=3)
    ix = index(X, metric)
    for lam in (0.25, 0.5):
        dr.same(ix.search_diverse(Q, 10, 64, lam=lam), dr.numpy_answer(d32, dr.ties_pairs(X, metric), 10, 64, lam), "d %d lambda %g" % (d, lam))
    ix.close()


def test_the_widest_pool_with_k_equal_to_fetch_k():
    X, Q, d32 = gr.ties_table(0, 1500, 8, 2, seed=3)
    ix = index(X, 0)
    want = dr.numpy_answer(d32, dr.ties_pairs(X, 0), 1024, 1024, 0.5)
    assert (want[3] == 1024).all() and not np.array_equal(want[0], dr.numpy_answer(d32, dr.ties_pairs(X, 0), 1024, 1024, 1.0)[0])
    dr.same(ix.search_diverse(Q, 1024, 1024, lam=0.5, flat_engine="stream"), want, "fetch_k = k = 1024")
    assert ix.stats()["dist_evals"] == 2 * 1500 + 2 * (1023 * 1024 - 1024 * 1023 // 2)
    ix.close()


def test_a_short_pool_pads_k_one_gathers_nothing_and_an_empty_table_answers_empty():
    X, Q, d32 = gr.ties_table(0, 40, 8, 4, seed=3)
    ix = index(X, 0)
    want = dr.numpy_answer(d32, dr.ties_pairs(X, 0), 50, 64, 0.5)
    assert (want[3] == 40).all() and (want[0][:, 40:] == -1).all()
    dr.same(ix.search_diverse(Q, 50, 64, lam=0.5), want, "n = 40, fetch_k = 64, k = 50")
    got = ix.search_diverse(Q, 1, 64, lam=0.25, flat_engine="stream")   # k = 1: position 0, no gather
    dr.same(got, dr.numpy_answer(d32, dr.ties_pairs(X, 0), 1, 64, 0.25), "k = 1")
    assert ix.stats()["dist_evals"] == 4 * 40
    ix.close()
    empty = index(X[:0], 0)
    got = empty.search_diverse(Q, 5, 20, lam=0.5)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and np.isposinf(got[2]).all() and (got[3] == 0).all()
    got = empty.search_diverse(Q, 5, 20, lam=0.5, ids=np.arange(7))
    assert (got[0] == -1).all() and np.isposinf(got[2]).all() and (got[3] == 0).all()
    empty.close()


def test_seventy_queries():
    X, Q, d32 = gr.ties_table(2, 300, 8, 70, seed=3)
    ix = index(X, 2)
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5), dr.numpy_answer(d32, dr.ties_pairs(X, 2), 10, 64, 0.5), "nq = 70")
    ix.close()


# ---- 2. continuous tables: the pool from search, D from search_among, the loop from numpy
def continuous(metric):
    rng = np.random.default_rng(17 + metric)
    X = rng.standard_normal((2000, 96)).astype(F)
    Q = rng.standard_normal((16, 96)).astype(F)
    if metric == 1:
        X /= np.linalg.norm(X, axis=1, keepdims=True).astype(F)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True).astype(F)
    return X, Q


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_continuous_tables_equal_the_loop_over_the_parents_bits(metric):
    X, Q = continuous(metric)
    nq, fetch_k, k, lam = len(Q), 100, 10, 0.7
    ix = index(X, metric)
    pool_ids, pool_d, pool_cnt = ix.search(Q, fetch_k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    assert (pool_cnt == fetch_k).all()
    want = [np.full((nq, k), -1, np.int64), np.full((nq, k), np.inf, F), np.full((nq, k), np.inf, F), np.zeros(nq, np.int32)]
    differs = 0
    for q in range(nq):
        # D[c][s]: what search_among returns for row c when the query is row s (selected row = query side)
        a_ids, a_dist, a_cnt = ix.search_among(X[pool_ids[q]], pool_ids[q], fetch_k)
        assert (a_cnt == fetch_k).all()
        position = np.full(len(X), -1, np.int64)
        position[pool_ids[q]] = np.arange(fetch_k)
        D = np.empty((fetch_k, fetch_k), F)
        for s in range(fetch_k):
            D[position[a_ids[s]], s] = a_dist[s]
        pos, want[1][q], want[2][q], want[3][q] = dr.numpy_diverse(pool_d[q], D, k, lam)
        want[0][q] = pool_ids[q][pos]
        differs += not np.array_equal(pos, np.arange(k))
    assert differs == nq   # the selection is not the pool's head for any query
    for engine in ENGINES:
        dr.same(ix.search_diverse(Q, k, fetch_k, lam=lam, flat_engine=engine), want, "metric %d engine %d" % (metric, engine))
    ix.close()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_lambda_one_is_search_k_on_every_flat_engine(metric):
    X, Q = continuous(metric)
    ix = index(X, metric)
    for engine in ENGINES:
        ids, dist, cnt = ix.search(Q, 10, mode=amd.MODE_FLAT, flat_engine=engine)
        got = ix.search_diverse(Q, 10, 100, lam=1.0, flat_engine=engine)
        dr.same(got, (ids, dist, dist, cnt), "engine %d" % engine)   # (score = 1 * d - 0 * m = d)
    ix.close()


# ---- 3. visibility and forms
@pytest.fixture(scope="module")
def table():
    X, Q, d32 = gr.ties_table(0, 300, 8, 5, seed=3)
    ix = index(X, 0)
    yield ix, X, Q, d32, dr.ties_pairs(X, 0)
    ix.close()


def reset(ix):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)


def test_deleted_bitset_and_an_id_map(table):
    ix, X, Q, d32, pairs = table
    reset(ix)
    n = len(X)
    deleted = np.packbits(np.random.default_rng(5).random((n + 7) // 8 * 8) < 0.4, bitorder="little")
    vis = sr.visible_rows(n, deleted=deleted)
    ix.set_deleted(deleted)
    free = dr.numpy_answer(d32, pairs, 10, 64, 0.5)
    want = dr.numpy_answer(d32, pairs, 10, 64, 0.5, visible=vis)
    assert not np.array_equal(want[0], free[0])   # (the filter bites)
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5), want, "deleted")
    ix.set_id_map(7, 3)
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5), dr.numpy_answer(d32, pairs, 10, 64, 0.5, visible=vis, base=7, stride=3), "deleted, id map")
    rows = np.arange(20, 280)
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5, ids=rows * 3 + 7),
            dr.numpy_answer(d32, pairs, 10, 64, 0.5, visible=vis, lists=rows, base=7, stride=3), "deleted, id map, a list")
    reset(ix)


def test_int_column(table):
    ix, X, Q, d32, pairs = table
    reset(ix)
    n = len(X)
    col = np.random.default_rng(3).integers(-100, 100, n).astype(np.int32)
    ix.set_int_filter(col, "<", 13)
    vis = sr.visible_rows(n, int_filter=(col, "<", 13))
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.25), dr.numpy_answer(d32, pairs, 10, 64, 0.25, visible=vis), "int column")
    reset(ix)


def test_program_on_the_exact_distance_shortens_the_pool_on_every_engine(table):
    ix, X, Q, d32, pairs = table
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(3)
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    t = float(np.sort(d32, axis=0)[60].min())   # an integer some row's distance EQUALS: `<=` keeps it
    assert (d32 == F(t)).any()
    prog = [("dist",), ("const", t), ("<=",), ("f32", 4), ("const", 0.3), (">",), ("and",)]
    ix.set_filter_program(prog, rows)
    vis = np.stack([sr.visible_rows(n, program=prog, rows=rows, dist=d32[:, q].astype(np.float64)) for q in range(d32.shape[1])], axis=1)
    want = dr.numpy_answer(d32, pairs, 50, 64, 0.5, visible=vis)
    assert (want[3] < 50).any() and (want[3] > 1).all()   # a pool shorter than k for some query: the program judges (row, query)
    for engine in ENGINES:   # (a program that reads @distance takes the exact scan whichever engine is asked for)
        dr.same(ix.search_diverse(Q, 50, 64, lam=0.5, flat_engine=engine), want, "program, engine %d" % engine)
    dr.same(ix.search_diverse(Q, 50, 64, lam=0.5, ids=np.arange(n)), want, "program, all ids")
    reset(ix)


def test_candidate_lists_shared_and_per_query_with_repeated_unknown_and_invisible_ids(table):
    ix, X, Q, d32, pairs = table
    reset(ix)
    n, nq = len(X), len(Q)
    for lam in (0.25, 0.75):
        dr.same(ix.search_diverse(Q, 10, 64, lam=lam, ids=np.arange(n)), ix.search_diverse(Q, 10, 64, lam=lam), "all ids = the flat form")
    deleted = np.packbits(np.random.default_rng(6).random((n + 7) // 8 * 8) < 0.3, bitorder="little")
    vis = sr.visible_rows(n, deleted=deleted)
    ix.set_deleted(deleted)
    ix.set_id_map(5, 2)
    rng = np.random.default_rng(8)
    named = rng.choice(n, size=150, replace=False).astype(np.int64)
    assert (~vis[named]).any()
    ids = np.concatenate([named * 2 + 5, named[:40] * 2 + 5, [-3, 4, 6, 5 + 2 * n, 2 ** 40]])   # repeats; below the base, between rows, beyond the table
    rng.shuffle(ids)
    rows = ar.rows_of(ids, 5, 2, n)
    assert set(rows.tolist()) == set(named.tolist())
    want = dr.numpy_answer(d32, pairs, 10, 64, 0.5, visible=vis, lists=rows, base=5, stride=2)
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5, ids=ids), want, "a shared list")
    st = ix.stats()
    pools = [int(vis[rows].sum())] * nq
    assert st["dist_evals"] == (len(ids) - 5) * nq + pairs_given_a_distance(want[3], [min(64, p) for p in pools]), st
    lists = [ids[:30], ids[30:31], ids[:0], ids, ids[100:]]
    cat = np.concatenate(lists)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    want = dr.numpy_answer(d32, pairs, 10, 64, 0.5, visible=vis, lists=[ar.rows_of(x, 5, 2, n) for x in lists], base=5, stride=2)
    assert want[3][2] == 0 and want[3][1] <= 1
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5, ids=cat, offsets=off), want, "per-query lists")
    got = ix.search_diverse(Q, 10, 64, lam=0.5, ids=ids[:0])   # an empty list is a list: an empty pool, not the flat form
    assert (got[0] == -1).all() and (got[3] == 0).all()
    reset(ix)


def test_device_tensors_in_and_out_equal_the_host_path(table):
    import torch
    ix, X, Q, d32, pairs = table
    reset(ix)
    n = len(X)
    want = dr.numpy_answer(d32, pairs, 10, 64, 0.5)
    ids = np.random.default_rng(15).choice(n, size=200, replace=False).astype(np.int64)
    want_list = dr.numpy_answer(d32, pairs, 10, 64, 0.5, lists=np.sort(ids))
    dq, dids = torch.from_numpy(Q).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    out = ix.search_diverse(dq, 10, 64, lam=0.5, flat_engine="stream")
    assert all(hasattr(t, "data_ptr") for t in out)
    ix.synchronize()
    dr.same([t.cpu().numpy() for t in out], want, "device, flat form")
    dr.same(ix.search_diverse(Q, 10, 64, lam=0.5), want, "host")
    out = ix.search_diverse(dq, 10, 64, lam=0.5, ids=dids)
    ix.synchronize()
    dr.same([t.cpu().numpy() for t in out], want_list, "device, a device list")
    mine = (torch.full((len(Q), 10), -7, dtype=torch.int64, device="cuda"), torch.zeros((len(Q), 10), dtype=torch.float32, device="cuda"),
            torch.zeros((len(Q), 10), dtype=torch.float32, device="cuda"), torch.zeros(len(Q), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    out = ix.search_diverse(Q, 10, 64, lam=0.5, ids=ids, out=mine)   # host queries and ids, device results
    assert out[0] is mine[0]
    ix.synchronize()
    dr.same([t.cpu().numpy() for t in out], want_list, "host in, device out")
    host = (np.full((len(Q), 10), -7, np.int64), np.zeros((len(Q), 10), F), np.zeros((len(Q), 10), F), np.zeros(len(Q), np.int32))
    out = ix.search_diverse(Q, 10, 64, lam=0.5, out=host)
    assert out[0] is host[0]
    dr.same(host, want, "out= host buffers")
    # score_out and counts_out may be NULL
    p = lambda a: a.ctypes.data   # noqa: E731
    ids_o, dist_o = np.empty((len(Q), 10), np.int64), np.empty((len(Q), 10), F)
    assert ix.L.eps_index_search_diverse(ix.h, p(Q), len(Q), 10, 64, 0.5, None, None, 0, None, p(ids_o), p(dist_o), None, None) == 0
    dr.same((ids_o, dist_o), want[:2], "no scores, no counts")


# ---- 4. nothing a later call can observe changes; refusals leave the outputs and the handle as they were
def test_search_diverse_leaves_no_trace(table):
    ix, X, Q, d32, pairs = table
    reset(ix)
    for engine in ENGINES:
        before = ix.search(Q, 10, mode=amd.MODE_FLAT, flat_engine=engine)
        st_before = {k: v for k, v in ix.stats().items() if k not in TIMING}
        ix.search_diverse(Q, 10, 64, lam=0.5, flat_engine=engine)
        ix.search_diverse(Q, 10, 64, lam=0.5, ids=np.arange(100))
        after = ix.search(Q, 10, mode=amd.MODE_FLAT, flat_engine=engine)
        st_after = {k: v for k, v in ix.stats().items() if k not in TIMING}
        for a, b in zip(before, after):
            assert np.array_equal(a, b), engine
        for f in ("one_pass", "i8_rotated", "main_kernel_bits", "main_kernel_rows", "main_kernel_queries", "dist_evals"):
            assert st_before[f] == st_after[f], (engine, f, st_before[f], st_after[f])


def test_refusals(table):
    import torch
    ix, X, Q, d32, pairs = table
    reset(ix)
    n, nq = len(X), len(Q)
    ids = np.arange(100, dtype=np.int64)
    search_before = ix.search(Q, 10, mode=amd.MODE_FLAT)
    want = dr.numpy_answer(d32, pairs, 10, 64, 0.5)
    host = (np.full((nq, 10), -7, np.int64), np.full((nq, 10), -7, F), np.full((nq, 10), -7, F), np.full(nq, -7, np.int32))

    def untouched_and_usable():
        assert all((a == -7).all() for a in host)
        for a, b in zip(search_before, ix.search(Q, 10, mode=amd.MODE_FLAT)):
            assert np.array_equal(a, b)
        dr.same(ix.search_diverse(Q, 10, 64, lam=0.5), want, "after a refusal")

    for k, fetch_k in ((0, 64), (-1, 64), (65, 64), (10, 1025), (1025, 1025), (1, 0)):
        with pytest.raises(EpsillaError) as e:
            ix.search_diverse(Q, k, fetch_k, out=host if k == 10 else None)
        assert e.value.code == 30000 and "fetch_k" in str(e.value), (k, fetch_k)
        untouched_and_usable()
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(EpsillaError) as e:
            ix.search_diverse(Q, 10, 64, lam=lam, out=host)
        assert e.value.code == 30000 and "lambda" in str(e.value), lam
        untouched_and_usable()
    for off in ([0, 20, 40, 30, 60, 100], [1, 20, 40, 50, 60, 100], [0, 20, 40, 50, 60, 99], [0, 20, 40, 50, 60, 101]):
        with pytest.raises(EpsillaError) as e:
            ix.search_diverse(Q, 10, 64, ids=ids, offsets=off, out=host)
        assert e.value.code == 30000 and "cand_offsets" in str(e.value), off
        untouched_and_usable()
    dev = [torch.empty((nq, 10), dtype=torch.int64, device="cuda"), torch.empty((nq, 10), dtype=torch.float32, device="cuda"),
           torch.empty((nq, 10), dtype=torch.float32, device="cuda"), torch.empty(nq, dtype=torch.int32, device="cuda")]
    with pytest.raises(ValueError):   # the wrapper refuses a mixed set, and so does the library
        ix.search_diverse(Q, 10, 64, out=(host[0], dev[1], host[2], host[3]))
    p = lambda a: a.ctypes.data   # noqa: E731
    L = ix.L
    rc = L.eps_index_search_diverse(ix.h, p(Q), nq, 10, 64, 0.5, None, None, 0, None, p(host[0]), p(host[1]), dev[2].data_ptr(), p(host[3]))
    assert rc == 30000 and "host or all be device" in L.eps_index_last_error(ix.h).decode()
    untouched_and_usable()
    assert L.eps_index_search_diverse(ix.h, None, nq, 10, 64, 0.5, None, None, 0, None, p(host[0]), p(host[1]), p(host[2]), p(host[3])) == 30000   # null queries
    assert L.eps_index_search_diverse(ix.h, p(Q), nq, 10, 64, 0.5, None, None, 0, None, None, p(host[1]), p(host[2]), p(host[3])) == 30000   # null ids_out
    assert L.eps_index_search_diverse(ix.h, p(Q), nq, 10, 64, 0.5, None, None, 0, None, p(host[0]), None, p(host[2]), p(host[3])) == 30000   # null dist_out
    assert L.eps_index_search_diverse(ix.h, p(Q), nq, 10, 64, 0.5, None, None, 100, None, p(host[0]), p(host[1]), p(host[2]), p(host[3])) == 30000   # a list without its ids
    assert L.eps_index_search_diverse(ix.h, p(Q), nq, 10, 64, 0.5, p(ids), None, -1, None, p(host[0]), p(host[1]), p(host[2]), p(host[3])) == 30000
    assert L.eps_index_search_diverse(ix.h, p(Q), -1, 10, 64, 0.5, None, None, 0, None, p(host[0]), p(host[1]), p(host[2]), p(host[3])) == 30000
    assert L.eps_index_search_diverse(ix.h, None, 0, 10, 64, 0.5, None, None, 0, None, None, None, None, None) == 0   # nq = 0
    doff = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    rc = L.eps_index_search_diverse(ix.h, p(Q), nq, 10, 64, 0.5, p(ids), doff.data_ptr(), len(ids), None, p(host[0]), p(host[1]), p(host[2]), p(host[3]))
    assert rc == 30000 and "host array" in L.eps_index_last_error(ix.h).decode()
    untouched_and_usable()
    # a sharded handle
    sh = amd.GpuIndex(X.shape[1], "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(np.zeros((300, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        sh.search_diverse(Q, 10, 64, out=host)
    assert e.value.code == 50002 and "shard" in str(e.value)
    sh.search(Q, 3, mode=amd.MODE_FLAT)
    sh.close()
    untouched_and_usable()
    # stale filter state after an append
    ix2 = index(X[:100], 0)
    gone = np.zeros(13, np.uint8)
    gone[0] = 1
    ix2.set_deleted(gone)
    ix2.append_rows(np.zeros((8, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        ix2.search_diverse(Q, 10, 64, out=host)
    assert e.value.code == 30000 and "set_deleted" in str(e.value)
    assert all((a == -7).all() for a in host)
    ix2.set_deleted(np.zeros(14, np.uint8))
    assert (ix2.search_diverse(Q, 10, 64)[3] == 10).all()
    ix2.close()
