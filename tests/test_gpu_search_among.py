"""GpuIndex.search_among / eps_index_search_among on the MI355X: the k closest visible rows among the ids the caller names - one list for the
batch (a candidate row is gathered once per tile of queries) or one list per query - by among_gather_kernel and among_merge_kernel
(csrc/among.hip).

Integer tables (coordinates -8 .. 8, or those / 16 for COSINE: every fp32 distance is exact in any order, and full of ties, so the id order
decides) are held to numpy's answer exactly: ids, distance bits, counts.  Continuous tables are held to tests/among_ref.py (checked on the CPU in
tests/test_among_ref_cpu.py, which also keeps the run that shows the band hides no row on them), and to the bits a flat search returns under
the complementary deleted bitset - the route a caller had before."""
import numpy as np
import pytest

import among_ref as ar
import exact_ref as er
import range_ref as rr
import select_ref as sr
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
KS = (1, 10, 64, 65, 130, 1024)   # one register of keys per lane, its edge, two (130: one query per workgroup), sixteen
TIMING = ("kernel_ms", "main_kernel_ms", "filter_ms_all")


def same(a, b, what=""):
    """ids, distance bits, counts"""
    for x, y, name in zip(a, b, ("ids", "dist", "counts")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "dist":
            x, y = (x + F(0)).view(np.uint32), (y + F(0)).view(np.uint32)
        bad = np.argwhere(x != y)
        assert x.shape == y.shape and len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def index(X, metric, appended=0):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    ix.attach_rows(X[:len(X) - appended])
    if appended:
        ix.append_rows(X[len(X) - appended:])
    return ix


def concat(lists):
    """per-query lists -> (ids, offsets)"""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return (np.concatenate(lists).astype(np.int64) if len(lists) else np.zeros(0, np.int64)), off


def want_of(d32, lists, k, n, visible=None, base=0, stride=1):
    """numpy's answer for lists of IDS under the id map; returns (answer with ids mapped back, (row, query) pairs that get a distance)"""
    nq = d32.shape[1]
    shared = isinstance(lists, np.ndarray)
    rows = ar.rows_of(lists, base, stride, n) if shared else [ar.rows_of(x, base, stride, n) for x in lists]
    ids, dist, counts = ar.numpy_among(d32, rows, k, visible)
    evals = int(ar.names_a_row(lists if shared else np.concatenate(list(lists) + [np.zeros(0, np.int64)]), base, stride, n).sum())
    return (np.where(ids >= 0, ids * stride + base, -1), dist, counts), evals * (nq if shared else 1)


def rows_per_round(d):
    """RPW * U of the gather: lane groups per wavefront x rows in flight per group"""
    vec4 = d % 4 == 0
    return 64 // er.group_lanes(d, vec4) * 4


# ---- 1. integer tables, bit for bit: both forms, every shape of the kernel, list lengths around one round of a wavefront
@pytest.mark.parametrize("d", [19, 64, 260])   # scalar form, G = 32 | 16-byte form, G = 16 | G = 64, two pieces per lane, the last partial
@pytest.mark.parametrize("n,appended", [(1000, 0), (2600, 2)])
@pytest.mark.parametrize("name,metric", [("integers -8..8", 0), ("integers -8..8", 2), ("integers / 16", 1)])
def test_integer_tables_equal_numpy(name, metric, n, appended, d):
    X, Q70 = er.make(name, n, d, 70, seed=metric)
    d70 = rr.dist32(X, Q70, metric)
    assert np.array_equal(d70.astype(np.float64), er.dist64(X, Q70, metric))
    ru = rows_per_round(d)
    assert ru == {19: 8, 64: 16, 260: 4}[d]
    lengths = (0, 1, ru - 1, ru, ru + 1, 1000)
    rng = np.random.default_rng([metric, n, d])
    ix = index(X, metric, appended)
    for nq in (1, 3, 5, 70):
        Q, d32 = Q70[:nq], d70[:, :nq]
        for k in KS:
            for m in lengths:   # one list for the batch
                ids = rng.choice(n, size=m, replace=False).astype(np.int64)
                want, evals = want_of(d32, ids, k, n)
                what = "shared nq %d k %d m %d" % (nq, k, m)
                same(ix.search_among(Q, ids, k), want, what)
                st = ix.stats()
                assert st["dist_evals"] == evals == m * nq and st["main_kernel_bits"] == 32 and st["main_kernel_rows"] == m and st["main_kernel_queries"] == nq, (what, st)
                assert (want[2] == min(k, m)).all()
            # one list per query: the lengths in turn, starting somewhere else for every (nq, k)
            start = int(rng.integers(len(lengths)))
            lists = [rng.choice(n, size=lengths[(start + j) % len(lengths)], replace=False).astype(np.int64) for j in range(nq)]
            if nq == 1:
                lists = [rng.choice(n, size=lengths[KS.index(k)], replace=False).astype(np.int64)]   # (each length once over the ks)
            ids, off = concat(lists)
            want, evals = want_of(d32, lists, k, n)
            what = "per query nq %d k %d lengths %s" % (nq, k, [len(x) for x in lists][:8])
            same(ix.search_among(Q, ids, k, offsets=off), want, what)
            st = ix.stats()
            assert st["dist_evals"] == evals == len(ids) and st["main_kernel_rows"] == len(ids) and st["main_kernel_queries"] == nq, (what, st)
    ix.close()


def test_a_list_of_the_whole_table_splits_one_query_over_workgroups():
    """20 000 entries: 157 workgroups share a query's list (628 partial lists) and the merge joins them"""
    n, d = 20000, 16
    X, Q = er.make("integers -8..8", n, d, 5, seed=2)
    d32 = rr.dist32(X, Q, 0)
    ix = index(X, 0)
    ids = np.random.default_rng(2).permutation(n).astype(np.int64)
    for nq in (1, 5):
        for k in (10, 130, 1024):
            want, evals = want_of(d32[:, :nq], ids, k, n)
            same(ix.search_among(Q[:nq], ids, k), want, "shared nq %d k %d" % (nq, k))
            assert ix.stats()["dist_evals"] == n * nq
            flat = ix.search(Q[:nq], k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
            same(flat, want, "the flat search itself, nq %d k %d" % (nq, k))
    lists = [ids, ids[:7000], ids[:0], ids[5000:]]   # per-query lists of very different lengths in one launch
    cat, off = concat(lists)
    want, evals = want_of(d32[:, :4], lists, 64, n)
    same(ix.search_among(Q[:4], cat, 64, offsets=off), want, "per query")
    assert ix.stats()["dist_evals"] == len(cat)
    ix.close()


def test_more_query_tiles_than_one_launch_takes():
    """33 000 queries at one query per workgroup (k = 130, and per-query lists): more than the 32 768 tiles of a launch's y extent, so the
    gather runs in two slices.  The reference is vectorised: short lists of distinct rows, exact integer distances"""
    n, d, nq, m = 509, 16, 33000, 6   # (n prime: base + step * i mod n are m distinct rows for any step)
    X, Q = er.make("integers -8..8", n, d, nq, seed=21)
    ix = index(X, 0)
    rng = np.random.default_rng(21)

    def want_of_rows(rows, k):   # rows [nq][m], ascending and distinct per query
        dist = ((X[rows] - Q[:, None, :]) ** 2).sum(axis=2, dtype=F)
        o = np.argsort(dist, axis=1, kind="stable")[:, :k]   # (stable over ascending rows: ties in id order)
        ids = np.full((nq, k), -1, np.int64)
        dd = np.full((nq, k), np.inf, F)
        ids[:, :o.shape[1]] = np.take_along_axis(rows, o, axis=1)
        dd[:, :o.shape[1]] = np.take_along_axis(dist, o, axis=1)
        return ids, dd, np.full(nq, min(k, m), np.int32)

    shared = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    same(ix.search_among(Q, shared[::-1].copy(), 130), want_of_rows(np.repeat(shared[None, :], nq, axis=0), 130), "shared, k 130")
    assert ix.stats()["dist_evals"] == m * nq
    rows = np.sort((rng.integers(n, size=(nq, 1)) + rng.integers(1, n, size=(nq, 1)) * np.arange(m)) % n, axis=1).astype(np.int64)
    assert (np.diff(rows, axis=1) > 0).all()
    off = np.arange(nq + 1, dtype=np.int64) * m
    for k in (1, 130):
        same(ix.search_among(Q, rows.reshape(-1), k, offsets=off), want_of_rows(rows, k), "per query, k %d" % k)
        assert ix.stats()["dist_evals"] == m * nq
    ix.close()


# ---- 2. the same bits as a flat search under the complementary bitset
@pytest.mark.parametrize("name,metric,d", [("gaussian", 0, 64), ("embedding-like", 1, 96), ("uniform", 2, 19), ("integers -8..8", 0, 260)])
def test_same_bits_as_a_flat_search_under_the_complementary_bitset(name, metric, d):
    n, nq = 3000, 9
    X, Q = er.make(name, n, d, nq, seed=4)
    ix = index(X, metric)
    rng = np.random.default_rng(4)
    for m in (1, 40, 700, n):
        rows = rng.choice(n, size=m, replace=False).astype(np.int64)
        for k in (1, 10, 100):
            got = ix.search_among(Q, rows, k)
            gone = np.ones(n, bool)
            gone[rows] = False
            ix.set_deleted(np.packbits(np.concatenate([gone, np.zeros(-n % 8, bool)]), bitorder="little"))
            flat = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
            ix.set_deleted(None)
            assert np.array_equal(got[0], flat[0]) and np.array_equal(got[1].view(np.uint32), flat[1].view(np.uint32)) and np.array_equal(got[2], flat[2]), (m, k)
    ix.close()


# ---- 3. the id rule: repeated ids, ids that name no row
@pytest.fixture(scope="module")
def table3():
    n, d = 1000, 19
    X, Q = er.make("integers -8..8", n, d, 5, seed=3)
    d32 = rr.dist32(X, Q, 0)
    ix = index(X, 0)
    yield ix, X, Q, d32
    ix.close()


def reset(ix):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)


def test_every_id_three_times_counts_once(table3):
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(6)
    for distinct, k in ((50, 64), (700, 1024), (7, 10), (100, 130)):   # (700 x 3: several wavefronts and workgroups hold the same row)
        rows = rng.choice(n, size=distinct, replace=False).astype(np.int64)
        ids = rng.permutation(np.repeat(rows, 3))
        want, evals = want_of(d32, ids, k, n)
        assert (want[2] == distinct).all() and distinct < k
        same(ix.search_among(Q, ids, k), want, "shared, %d distinct" % distinct)
        assert ix.stats()["dist_evals"] == 3 * distinct * len(Q) == evals   # (every entry that names a row is given a distance)
        lists = [rng.permutation(np.repeat(rows[j:], 3)) for j in range(len(Q))]
        cat, off = concat(lists)
        want, evals = want_of(d32, lists, k, n)
        same(ix.search_among(Q, cat, k, offsets=off), want, "per query, %d distinct" % distinct)
    # k below the distinct count: the duplicates must not push a row out
    rows = rng.choice(n, size=200, replace=False).astype(np.int64)
    ids = rng.permutation(np.repeat(rows, 3))
    for k in (1, 10, 64, 130):
        same(ix.search_among(Q, ids, k), want_of(d32, ids, k, n)[0], "k %d of 200 distinct" % k)


def test_ids_that_name_no_row_are_ignored(table3):
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(8)
    none = np.array([-1, n, n + 5, 2 ** 40, -2 ** 63, 2 ** 63 - 1], np.int64)
    rows = rng.choice(n, size=90, replace=False).astype(np.int64)
    ids = rng.permutation(np.concatenate([rows, none, none]))
    want, evals = want_of(d32, ids, 100, n)
    assert (want[2] == 90).all() and evals == 90 * len(Q)
    same(ix.search_among(Q, ids, 100), want, "identity map")
    assert ix.stats()["dist_evals"] == evals and ix.stats()["main_kernel_rows"] == len(ids)
    got = ix.search_among(Q, none, 10)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and (got[2] == 0).all() and ix.stats()["dist_evals"] == 0
    # base 3, stride 8: row r is id 8 r + 3; everything else names nothing
    ix.set_id_map(3, 8)
    good = rows * 8 + 3
    bad = np.concatenate([rows * 8 + 4, rows[:20] * 8 + 2, rows[:20] * 8 - 5 + 3 + 4, [2, 1, 0, -5, -13, 8 * n + 3, 8 * (n + 5) + 3, 2 ** 40 + 3, 2 ** 40]]).astype(np.int64)
    assert len(ar.rows_of(bad, 3, 8, n)) == 0 and np.array_equal(ar.rows_of(good, 3, 8, n), np.sort(rows))
    ids = rng.permutation(np.concatenate([good, bad]))
    want, evals = want_of(d32, ids, 100, n, base=3, stride=8)
    assert (want[2] == 90).all() and (want[0][:, :90] % 8 == 3).all()
    same(ix.search_among(Q, ids, 100), want, "base 3 stride 8")
    assert ix.stats()["dist_evals"] == 90 * len(Q)
    got = ix.search_among(Q, bad, 10)
    assert (got[0] == -1).all() and (got[2] == 0).all()
    lists = [good[:30], bad, good[30:], np.concatenate([bad[:50], good[:5]]), good[:0]]
    cat, off = concat(lists)
    want, evals = want_of(d32, lists, 64, n, base=3, stride=8)
    assert want[2].tolist() == [30, 0, 60, 5, 0]
    same(ix.search_among(Q, cat, 64, offsets=off), want, "per query, base 3 stride 8")
    assert ix.stats()["dist_evals"] == evals == 95
    ix.set_id_map(-7, 3)   # a negative base: ids below zero name rows
    good = rows * 3 - 7
    ids = rng.permutation(np.concatenate([good, [-8, -10, -6, 3 * n - 7]])).astype(np.int64)
    want, evals = want_of(d32, ids, 100, n, base=-7, stride=3)
    assert (want[2] == 90).all()
    same(ix.search_among(Q, ids, 100), want, "base -7 stride 3")
    reset(ix)


def test_disjoint_per_query_lists_stay_apart(table3):
    ix, X, Q, d32 = table3
    reset(ix)
    n, nq = len(X), len(Q)
    perm = np.random.default_rng(10).permutation(n).astype(np.int64)
    lists = [perm[j::nq] for j in range(nq)]
    cat, off = concat(lists)
    for k in (10, 130):
        got = ix.search_among(Q, cat, k, offsets=off)
        for j in range(nq):
            assert got[2][j] == k and np.isin(got[0][j], lists[j]).all(), (k, j)
        same(got, want_of(d32, lists, k, n)[0], "k %d" % k)


# ---- 4. visibility: the installed bitset, column and program, judged as a search judges them
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


def check_visible(ix, Q, d32, vis, n, base=0, stride=1):
    rng = np.random.default_rng(12)
    rows = rng.choice(n, size=400, replace=False).astype(np.int64)
    ids = rows * stride + base
    for k in (10, 130):
        want, _ = want_of(d32, ids, k, n, visible=vis, base=base, stride=stride)
        free, _ = want_of(d32, ids, k, n, base=base, stride=stride)
        assert not np.array_equal(want[0], free[0]) and (want[2] > 0).all()   # (the filter bites, and leaves something)
        same(ix.search_among(Q, ids, k), want, "shared k %d" % k)
        lists = [ids[j * 50:] for j in range(len(Q))]
        cat, off = concat(lists)
        same(ix.search_among(Q, cat, k, offsets=off), want_of(d32, lists, k, n, visible=vis, base=base, stride=stride)[0], "per query k %d" % k)


def test_deleted_bitset(table3):
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    deleted = np.packbits(np.random.default_rng(5).random((n + 7) // 8 * 8) < 0.4, bitorder="little")
    ix.set_deleted(deleted)
    check_visible(ix, Q, d32, sr.visible_rows(n, deleted=deleted), n)
    ix.set_id_map(7, 3)
    check_visible(ix, Q, d32, sr.visible_rows(n, deleted=deleted), n, base=7, stride=3)
    reset(ix)


def test_int_column(table3):
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    col = np.random.default_rng(3).integers(-100, 100, n).astype(np.int32)
    ix.set_int_filter(col, "<", 13)
    check_visible(ix, Q, d32, sr.visible_rows(n, int_filter=(col, "<", 13)), n)
    reset(ix)


def test_program_reads_the_exact_distance(table3):
    """@distance <= t AND attr > c: the program is judged per (row, query), with the row's exact distance"""
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(3)
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    t = float(np.sort(d32, axis=0)[300].min())   # an integer some row's distance EQUALS: `<=` keeps it
    assert (d32 == F(t)).any()
    prog = [("dist",), ("const", t), ("<=",), ("f32", 4), ("const", 0.3), (">",), ("and",)]
    ix.set_filter_program(prog, rows)
    vis = np.stack([sr.visible_rows(n, program=prog, rows=rows, dist=d32[:, q].astype(np.float64)) for q in range(d32.shape[1])], axis=1)
    check_visible(ix, Q, d32, vis, n)
    got = ix.search_among(Q, np.arange(n), 1024)
    assert (got[1][np.isfinite(got[1])] <= F(t)).all() and (got[2] == vis.sum(axis=0)).all()
    reset(ix)


# ---- 5. continuous tables: among_ref under the tree bound, after the condition on the tables themselves
@pytest.mark.parametrize("name,metric", ar.CONT)
def test_continuous_tables_against_the_fp64_reference(name, metric):
    n, d, nq = ar.CONT_SHAPE
    X, Q = er.make(name, n, d, nq, seed=7)
    ref = er.Ref(X, Q, metric)
    lists = ar.cont_lists()
    ix = index(X, metric)
    for rows in lists:
        mask = er._visible(n, rows)
        for k in ar.CONT_K:
            er.assert_cap(ref, k, visible=mask, what=name)
            und0 = er.undecided(ref, k, visible=mask, bound="tree")
            assert und0 <= er.CAP * k * nq, (name, len(rows), k, und0)
            got = ix.search_among(Q, rows, k)
            und = ar.check_among(*got, ref, rows, k, what="%s m %d k %d" % (name, len(rows), k))
            print("%s metric %d m %d k %d: %d undecided rows; error / bound (free, tree) %s" % (name, metric, len(rows), k, und, er.error_ratios(*got, ref)))
            assert und <= er.CAP * k * nq
    per_query = [lists[j % 3] for j in range(nq)]   # the three lists in turn, one launch
    cat, off = concat(per_query)
    for k in ar.CONT_K:
        ar.check_among(*ix.search_among(Q, cat, k, offsets=off), ref, per_query, k, what="%s per query k %d" % (name, k))
    ix.close()


# ---- 6. host and device buffers
@pytest.mark.parametrize("staging", [None, "0"])
def test_host_in_host_out_with_and_without_page_locked_staging(monkeypatch, table3, staging):
    if staging is None:
        monkeypatch.delenv("EPS_HOST_STAGING", raising=False)
    else:
        monkeypatch.setenv("EPS_HOST_STAGING", staging)
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    ids = np.random.default_rng(14).choice(n, size=300, replace=False).astype(np.int64)
    lists = [ids[:5], ids[5:105], ids[:0], ids, ids[100:]]
    cat, off = concat(lists)
    for k in (10, 130):
        got = ix.search_among(Q, ids, k)
        assert all(isinstance(a, np.ndarray) for a in got)
        same(got, want_of(d32, ids, k, n)[0], "shared staging=%r" % staging)
        want = want_of(d32, lists, k, n)[0]
        assert (want[2] < k).any() and (want[2] == k).any()   # (full and partly filled lists: a part read at the wrong offset shows)
        same(ix.search_among(Q, cat, k, offsets=off), want, "per query staging=%r" % staging)
    mine = (np.full((len(Q), 10), -7, np.int64), np.zeros((len(Q), 10), F), np.zeros(len(Q), np.int32))
    out = ix.search_among(Q, ids, 10, out=mine)
    assert out[0] is mine[0]
    same(out, want_of(d32, ids, 10, n)[0], "out= staging=%r" % staging)


def test_device_tensors_in_give_device_tensors_out(table3):
    import torch
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    ids = np.random.default_rng(15).choice(n, size=300, replace=False).astype(np.int64)
    lists = [ids[:5], ids[5:105], ids[:0], ids, ids[100:]]
    cat, off = concat(lists)
    dq, dids, dcat = torch.from_numpy(Q).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(cat).cuda()
    torch.cuda.synchronize()
    for k in (10, 130):
        out = ix.search_among(dq, dids, k)
        assert all(hasattr(t, "data_ptr") for t in out)
        ix.synchronize()
        same([t.cpu().numpy() for t in out], want_of(d32, ids, k, n)[0], "device, shared")
        assert ix.stats()["dist_evals"] == 300 * len(Q)
        out = ix.search_among(dq, dcat, k, offsets=off)
        ix.synchronize()
        same([t.cpu().numpy() for t in out], want_of(d32, lists, k, n)[0], "device, per query")
        assert ix.stats()["dist_evals"] == len(cat)
    same(ix.search_among(Q, dids, 10), want_of(d32, ids, 10, n)[0], "host queries, device ids")   # (each buffer is classified by itself)
    mine = (torch.full((len(Q), 10), -7, dtype=torch.int64, device="cuda"), torch.zeros((len(Q), 10), dtype=torch.float32, device="cuda"),
            torch.zeros(len(Q), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    out = ix.search_among(Q, ids, 10, out=mine)   # host queries and ids, device results
    assert out[0] is mine[0]
    ix.synchronize()
    same([t.cpu().numpy() for t in out], want_of(d32, ids, 10, n)[0], "host in, device out")


# ---- 7. nothing a later search, select or search_range can observe changes
def test_search_among_leaves_no_trace(table3):
    ix, X, Q, d32 = table3
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(3)
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    prog = [("i32", 0), ("const", 3), ("%",), ("const", 0), ("=",), ("f32", 4), ("const", 0.5), (">",), ("or",)]
    ix.set_filter_program(prog, rows)
    vis = sr.visible_rows(n, program=prog, rows=rows)
    radius = (np.sort(d32, axis=0)[120] + F(0.5)).astype(F)
    ids = rng.choice(n, size=500, replace=False).astype(np.int64)
    cat, off = concat([ids[j * 60:] for j in range(len(Q))])
    for kw in (dict(flat_engine=amd.FLAT_STREAM), dict(flat_engine=amd.FLAT_MFMA), dict(flat_engine=amd.FLAT_MFMA_I8), dict(flat_engine=amd.FLAT_AUTO)):
        before = ix.search(Q, 10, mode=amd.MODE_FLAT, **kw)
        st_before = {k: v for k, v in ix.stats().items() if k not in TIMING}
        sel_before = ix.select(3, 200)
        rng_before = ix.search_range(Q, radius, 64, flat_engine=kw["flat_engine"])
        for k in (10, 130):
            same(ix.search_among(Q, ids, k), want_of(d32, ids, k, n, visible=vis)[0], "among, program installed")
            st = ix.stats()
            assert st["main_kernel_bits"] == 32 and st["dist_evals"] == 500 * len(Q) and st["main_kernel_launches"] == 1, st
            assert st["main_kernel_rows"] == 500 and st["main_kernel_queries"] == len(Q) and st["main_kernel_ms"] > 0 and st["one_pass"] == 0, st
            ix.search_among(Q, cat, k, offsets=off)
            assert ix.stats()["dist_evals"] == len(cat)
        after = ix.search(Q, 10, mode=amd.MODE_FLAT, **kw)
        st_after = {k: v for k, v in ix.stats().items() if k not in TIMING}
        sel_after = ix.select(3, 200)
        rng_after = ix.search_range(Q, radius, 64, flat_engine=kw["flat_engine"])
        for a, b in zip(before + rng_before, after + rng_after):
            assert np.array_equal(a, b), kw
        assert np.array_equal(sel_before[0], sel_after[0]) and sel_before[1] == sel_after[1]
        for f in ("one_pass", "i8_rotated", "main_kernel_bits", "main_kernel_rows", "main_kernel_queries"):
            assert st_before[f] == st_after[f], (kw, f, st_before[f], st_after[f])
    reset(ix)


# ---- 8. refusals: each leaves the handle usable
def test_refusals(table3):
    import torch
    ix, X, Q, d32 = table3
    reset(ix)
    n, nq = len(X), len(Q)
    ids = np.arange(100, dtype=np.int64)
    want = want_of(d32, ids, 10, n)[0]

    def usable():
        same(ix.search_among(Q, ids, 10), want, "after a refusal")

    for k in (0, 1025, -1):
        with pytest.raises(EpsillaError) as e:
            ix.search_among(Q, ids, k)
        assert e.value.code == 30000 and "k must be" in str(e.value)
        usable()
    for off in ([0, 20, 40, 30, 60, 100], [1, 20, 40, 50, 60, 100], [0, 20, 40, 50, 60, 99], [0, 20, 40, 50, 60, 101], [0, 20, 40, 50, 120, 100]):
        with pytest.raises(EpsillaError) as e:
            ix.search_among(Q, ids, 10, offsets=off)
        assert e.value.code == 30000 and "cand_offsets" in str(e.value), off
        usable()
    host = [np.empty((nq, 10), np.int64), np.empty((nq, 10), F), np.empty(nq, np.int32)]
    dev = [torch.empty((nq, 10), dtype=torch.int64, device="cuda"), torch.empty((nq, 10), dtype=torch.float32, device="cuda"),
           torch.empty(nq, dtype=torch.int32, device="cuda")]
    with pytest.raises(ValueError):   # the wrapper refuses a mixed set, and so does the library
        ix.search_among(Q, ids, 10, out=(host[0], dev[1], host[2]))
    p = lambda a: a.ctypes.data   # noqa: E731
    rc = ix.L.eps_index_search_among(ix.h, p(Q), nq, p(ids), None, len(ids), 10, p(host[0]), dev[1].data_ptr(), p(host[2]))
    assert rc == 30000 and "host or all be device" in ix.L.eps_index_last_error(ix.h).decode()
    usable()
    assert ix.L.eps_index_search_among(ix.h, None, nq, p(ids), None, len(ids), 10, p(host[0]), p(host[1]), p(host[2])) == 30000   # null queries
    assert ix.L.eps_index_search_among(ix.h, p(Q), nq, None, None, len(ids), 10, p(host[0]), p(host[1]), p(host[2])) == 30000   # null list of 100
    assert ix.L.eps_index_search_among(ix.h, p(Q), nq, p(ids), None, len(ids), 10, None, p(host[1]), p(host[2])) == 30000
    assert ix.L.eps_index_search_among(ix.h, p(Q), nq, p(ids), None, -1, 10, p(host[0]), p(host[1]), p(host[2])) == 30000
    assert ix.L.eps_index_search_among(ix.h, p(Q), nq, p(ids), None, 2 ** 31, 10, p(host[0]), p(host[1]), p(host[2])) == 30000
    assert ix.L.eps_index_search_among(ix.h, p(Q), -1, p(ids), None, len(ids), 10, p(host[0]), p(host[1]), p(host[2])) == 30000
    assert ix.L.eps_index_search_among(ix.h, None, 0, None, None, 0, 10, None, None, None) == 0   # nq = 0
    doff = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    rc = ix.L.eps_index_search_among(ix.h, p(Q), nq, p(ids), doff.data_ptr(), len(ids), 10, p(host[0]), p(host[1]), p(host[2]))
    assert rc == 30000 and "host array" in ix.L.eps_index_last_error(ix.h).decode()
    usable()
    got = ix.search_among(Q, ids[:0], 10)   # an empty list, and no list entries at all behind offsets
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and (got[2] == 0).all()
    got = ix.search_among(Q, ids[:0], 10, offsets=[0] * (nq + 1))
    assert (got[0] == -1).all() and (got[2] == 0).all()
    # a sharded handle
    sh = amd.GpuIndex(X.shape[1], "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(np.zeros((300, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        sh.search_among(Q, ids, 10)
    assert e.value.code == 50002 and "shard" in str(e.value)
    sh.search(Q, 3, mode=amd.MODE_FLAT)
    sh.close()
    # stale filter state after an append
    ix2 = index(X[:100], 0)
    gone = np.zeros(13, np.uint8)
    gone[0] = 1
    ix2.set_deleted(gone)
    ix2.append_rows(np.zeros((8, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        ix2.search_among(Q, ids, 10)
    assert e.value.code == 30000 and "set_deleted" in str(e.value)
    ix2.set_deleted(np.zeros(14, np.uint8))
    assert (ix2.search_among(Q, ids, 10)[2] == 10).all()
    ix2.close()
    # an index without rows: every id names nothing
    empty = amd.GpuIndex(X.shape[1], "EUCLIDEAN", device=0)
    got = empty.search_among(Q, ids, 4)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and (got[2] == 0).all()
    empty.close()
