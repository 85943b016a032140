"""GpuIndex.select / eps_index_select on the MI355X: the visible rows in ascending row order, windowed by skip / limit - SearchByAttribute's full
scan (vec_search_executor.cpp:1016-1029) as three launches (csrc/select.hip: verdict bitset + block counts, scan, scatter).

Expected ids = flatnonzero(visible)[skip : skip + limit] * stride + base and total = visible.sum(), `visible` from the numpy evaluator of
tests/select_ref.py (checked on hand-written rows in tests/test_select_cpu.py).  Both sides compare in double: equality is exact."""
import numpy as np
import pytest

import select_ref as sr
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

DIM = 4
B = sr.SEL_ROWS                         # rows per block of the verdict / scatter launches
N_SCAN2 = sr.SEL_SCAN_THREADS * B + 1   # one block count more than the scan's workgroup takes per round: its loop runs a second time

# packed attribute rows of 8 bytes (the smallest stride that holds an I32 and an F32) and of 16 (with a BOOL and an I16 as well)
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])
ROW16 = np.dtype([("a", np.int32), ("x", np.float32), ("flag", np.uint8), ("pad", np.uint8), ("s", np.int16), ("pad2", np.int32)])
# a % 3 = 0 OR x > 0.5
PROG8 = [("i32", 0), ("const", 3), ("%",), ("const", 0), ("=",), ("f32", 4), ("const", 0.5), (">",), ("or",)]
# (flag AND NOT a % 7 < 3) OR (x * 2 - @distance > 1.5 AND @distance = 0): I32, F32, BOOL, AND / OR / NOT, MOD and @distance (which must read as 0)
PROG16 = [("bool", 8), ("i32", 0), ("const", 7), ("%",), ("const", 3), ("<",), ("not",), ("and",),
          ("f32", 4), ("const", 2), ("*",), ("dist",), ("-",), ("const", 1.5), (">",), ("dist",), ("const", 0), ("=",), ("and",), ("or",)]


def rows8(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, ROW8)
    r["a"] = rng.integers(-1000, 1000, n)
    r["x"] = rng.random(n, dtype=np.float32)
    return r


def rows16(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, ROW16)
    r["a"] = rng.integers(-1000, 1000, n)
    r["x"] = rng.random(n, dtype=np.float32)
    r["flag"] = rng.integers(0, 3, n)   # (2 is true as well: byte != 0)
    r["s"] = rng.integers(-300, 300, n)
    return r


def index(n, seed=1):
    ix = amd.GpuIndex(DIM, "EUCLIDEAN", device=0)
    ix.attach_rows(np.random.default_rng(seed).random((n, DIM), dtype=np.float32))
    return ix


def check(ix, vis, skip, limit, base=0, stride=1):
    ids, total = ix.select(skip, limit)
    want, want_total = sr.expected(vis, skip, len(vis) if limit is None else limit, base, stride)
    assert total == want_total, (skip, limit, total, want_total)
    assert ids.dtype == np.int64 and np.array_equal(ids, want), (skip, limit, len(ids), len(want), ids[:8], want[:8])


# ---- 1. row counts at the edges of wavefront, block and scan
@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 70001, N_SCAN2])
def test_row_counts_at_the_edges(n):
    rows = rows8(n, n)
    vis = sr.visible_rows(n, program=PROG8, rows=rows)
    ix = index(n)
    ix.set_filter_program(PROG8, rows)
    check(ix, vis, 0, None)
    check(ix, vis, max(int(vis.sum()) - 3, 0), 10)   # the table's last visible rows: the last block, the last offsets of the scan
    ix.close()


# ---- 2. windows
@pytest.fixture(scope="module")
def five_blocks():
    n = 4 * B + 500
    rows = rows8(n, 7)
    vis = sr.visible_rows(n, program=PROG8, rows=rows)
    ix = index(n)
    ix.set_filter_program(PROG8, rows)
    yield ix, vis
    ix.close()


def test_windows(five_blocks):
    ix, vis = five_blocks
    total = int(vis.sum())
    r1, r2 = int(vis[:B].sum()), int(vis[:2 * B].sum())   # ranks at which blocks 1 and 2 begin
    assert 3 < r1 < r2 - 3 and r2 + 3 < total
    for skip, limit in [(r1 - 3, 7), (r2 - 1, 2), (r1 - 3, r2 - r1 + 6), (r1, 1), (r1 - 1, 1),   # straddling / touching block boundaries
                        (total - 1, 1), (total - 1, 5), (total, 5), (total + 1000, 5), (2 ** 62, 5),   # skip = total - 1, skip >= total
                        (0, 0), (r1, 0), (0, total), (0, total + 1), (5, len(vis) + 100), (0, 2 ** 40)]:   # limit = 0, limit > total
        got_ids = np.full(min(limit, len(vis) + 200), -7, np.int64)
        counts = np.full(2, -7, np.int64)
        lim = len(got_ids)
        ids, tot = ix.select(skip, lim, out=(got_ids, counts))
        want, _ = sr.expected(vis, skip, lim)
        assert tot == total and counts[1] == total, (skip, limit, tot)
        assert counts[0] == len(want) == len(ids) and np.array_equal(ids, want), (skip, limit, counts, len(want))
        assert (got_ids[len(want):] == -7).all(), (skip, limit)   # nothing written beyond the count
        if limit != lim:   # a limit beyond the table: the library clamps it to the row count itself
            c = np.zeros(2, np.int64)
            big = np.full(len(vis), -7, np.int64)
            rc = ix.L.eps_index_select(ix.h, skip, limit, big.ctypes.data, c.ctypes.data, c.ctypes.data + 8)
            assert rc == 0 and c[1] == total and np.array_equal(big[:c[0]], sr.expected(vis, skip, len(vis))[0])


def test_negative_skip_or_limit_is_a_user_error(five_blocks):
    ix, _ = five_blocks
    ids, c = np.full(8, -7, np.int64), np.full(2, -7, np.int64)
    for skip, limit in ((-1, 5), (0, -1), (-2 ** 63, 5)):
        assert ix.L.eps_index_select(ix.h, skip, limit, ids.ctypes.data, c.ctypes.data, c.ctypes.data + 8) == 30000, (skip, limit)
        assert "skip and limit" in ix.L.eps_index_last_error(ix.h).decode()
    assert (ids == -7).all() and (c == -7).all()
    with pytest.raises(EpsillaError) as e:
        ix.select(-1, 5)
    assert e.value.code == 30000


def test_empty_table():
    ix = amd.GpuIndex(DIM, "EUCLIDEAN", device=0)
    ids, total = ix.select(0, 10)
    assert len(ids) == 0 and total == 0
    ix.attach_rows(np.zeros((0, DIM), np.float32))
    ids, total = ix.select(3, 10)
    assert len(ids) == 0 and total == 0
    ix.close()


# ---- 3. predicates
N3 = 2 * B + 77


@pytest.fixture(scope="module")
def table3():
    ix = index(N3)
    rng = np.random.default_rng(3)
    deleted = np.packbits(rng.random((N3 + 7) // 8 * 8) < 0.3, bitorder="little")
    yield ix, deleted, rows16(N3, 4)
    ix.close()


def reset(ix):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)


def test_no_filter_at_all(table3):
    ix, _, _ = table3
    reset(ix)
    check(ix, np.ones(N3, bool), 0, None)
    check(ix, np.ones(N3, bool), B - 2, 5)


def test_deleted_bitset_alone(table3):
    ix, deleted, _ = table3
    reset(ix)
    ix.set_deleted(deleted)
    check(ix, sr.visible_rows(N3, deleted=deleted), 0, None)


@pytest.mark.parametrize("width", [1, 2, 4, 8])
@pytest.mark.parametrize("op", ["<", ">=", "!="])
def test_int_column_alone(table3, width, op):
    ix, _, _ = table3
    reset(ix)
    dt = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[width]
    col = np.random.default_rng(width).integers(-100, 100, N3).astype(dt)
    ix.set_int_filter(col, op, 13)
    check(ix, sr.visible_rows(N3, int_filter=(col, op, 13)), 0, None)


def test_program_alone(table3):
    ix, _, rows = table3
    reset(ix)
    ix.set_filter_program(PROG16, rows)
    vis = sr.visible_rows(N3, program=PROG16, rows=rows)
    assert 0.2 * N3 < vis.sum() < 0.8 * N3
    check(ix, vis, 0, None)
    # @distance reads as 0: `@distance < 1` passes every row, `@distance <> 0` none
    ix.set_filter_program([("dist",), ("const", 1), ("<",)], rows)
    check(ix, np.ones(N3, bool), 0, None)
    ix.set_filter_program([("dist",), ("const", 0), ("<>",)], rows)
    check(ix, np.zeros(N3, bool), 0, None)


def test_deleted_bitset_and_program_together(table3):
    ix, deleted, rows = table3
    reset(ix)
    ix.set_deleted(deleted)
    ix.set_filter_program(PROG16, rows)
    vis = sr.visible_rows(N3, deleted=deleted, program=PROG16, rows=rows)
    check(ix, vis, 0, None)
    check(ix, vis, int(vis[:B].sum()) - 2, 9)


def test_all_rows_hidden(table3):
    ix, _, rows = table3
    reset(ix)
    ix.set_deleted(np.full((N3 + 7) // 8, 0xFF, np.uint8))
    check(ix, np.zeros(N3, bool), 0, None)
    check(ix, np.zeros(N3, bool), 0, 0)
    reset(ix)
    ix.set_filter_program([("const", 0)], rows)
    check(ix, np.zeros(N3, bool), 0, 5)


# ---- 4. outputs and call state
def test_id_map_is_applied(table3):
    ix, deleted, _ = table3
    reset(ix)
    ix.set_deleted(deleted)
    ix.set_id_map(3, 8)
    vis = sr.visible_rows(N3, deleted=deleted)
    check(ix, vis, 0, None, base=3, stride=8)
    check(ix, vis, 11, 40, base=3, stride=8)


def test_device_outputs_agree_with_host_outputs(table3):
    import torch
    ix, deleted, rows = table3
    reset(ix)
    ix.set_deleted(deleted)
    ix.set_filter_program(PROG16, rows)
    for skip, limit in ((0, N3), (17, 300), (N3, 4), (0, 0)):
        h_ids, h_total = ix.select(skip, limit)
        d_ids = torch.full((limit,), -7, dtype=torch.int64, device="cuda")
        d_counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        out = ix.select(skip, limit, out=(d_ids, d_counts))
        assert out[0] is d_ids and out[1] is d_counts   # asynchronous: handed back as they are
        ix.synchronize()
        c = d_counts.cpu().numpy()
        assert c[0] == len(h_ids) and c[1] == h_total, (skip, limit, c)
        got = d_ids.cpu().numpy()
        assert np.array_equal(got[:c[0]], h_ids) and (got[c[0]:] == -7).all()
    with pytest.raises(ValueError):   # one host, one device buffer
        ix.select(0, 4, out=(np.empty(4, np.int64), torch.zeros(2, dtype=torch.int64, device="cuda")))


def test_select_leaves_no_trace_in_a_search():
    n = 3 * B + 5
    rows = rows8(n, 11)
    ix = index(n, seed=12)
    ix.set_filter_program(PROG8, rows)
    Q = np.random.default_rng(13).random((3, DIM), dtype=np.float32)
    timing = ("kernel_ms", "main_kernel_ms", "filter_ms_all")
    kw = dict(mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)   # (one engine for both searches: the library's own choice may move with the calls it has seen)
    before = ix.search(Q, 10, **kw)
    stats = {k: v for k, v in ix.stats().items() if k not in timing}
    vis = sr.visible_rows(n, program=PROG8, rows=rows)
    check(ix, vis, 100, 1000)
    assert {k: v for k, v in ix.stats().items() if k not in timing} == stats   # the last SEARCH's statistics
    after = ix.search(Q, 10, **kw)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert vis[before[0][before[0] >= 0]].all()   # (the filter was live in both)
    ix.close()


def test_sharded_handle_is_refused():
    ix = amd.GpuIndex(DIM, "EUCLIDEAN", devices=[0, 0])
    ix.attach_rows(np.random.default_rng(1).random((300, DIM), dtype=np.float32))
    with pytest.raises(EpsillaError) as e:
        ix.select(0, 10)
    assert e.value.code == 50002 and "shard" in str(e.value)
    ix.close()


def test_python_mirror_of_SearchByAttribute():
    """vectordb_amd.VecSearchExecutor.SearchByAttribute: limit = min(raw_limit, record_number_), ids in search_result_ (:958-964, :1016-1029)"""
    n = 3000
    X = np.random.default_rng(5).random((n, DIM), dtype=np.float32)
    seg = amd.ANNGraphSegment()
    ex = amd.VecSearchExecutor(DIM, 0, seg, np.zeros(1, np.int64), np.zeros(0, np.int64), X, "EUCLIDEAN", L_master=50)
    ids_col = np.arange(n, dtype=np.int32)
    deleted = np.zeros((n + 7) // 8, np.uint8)
    deleted[0] = 0b101   # rows 0 and 2
    vis = sr.visible_rows(n, deleted=deleted, int_filter=(ids_col, "<", 1500))
    for skip, limit in ((0, 10), (5, 200), (1490, 100), (0, 10 ** 9)):
        rc, m = ex.SearchByAttribute(n, skip, limit, deleted=deleted, filter_spec=(ids_col, "<", 1500))
        want, _ = sr.expected(vis, skip, min(limit, n))
        assert rc == 0 and m == len(want) and np.array_equal(ex.search_result_[:m], want), (skip, limit, m)


# ---- 5. the drop-in: DBServer::Project -> VecSearchExecutor::SearchByAttribute through the reference's own DBMS layers
from oracle.pyoracle import DROPIN_SO, Ref, dropin_available, ref_available   # noqa: E402


@pytest.fixture(scope="module")
def dropin():
    import os
    if os.path.isdir("/root/reference/engine"):
        from vectordb_amd.build import build
        from oracle.pyoracle import build_dropin
        build()
        build_dropin()
    if not dropin_available():
        pytest.skip("oracle/_ref/dropin/libepsilla_dropin.so not built (needs the reference's sources: `make -C dropin OUT=$PWD/oracle/_ref/dropin`)")
    return Ref(DROPIN_SO)


@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_dropin_get_on_the_device_matches_reference(dropin, tmp_path, monkeypatch):
    """The cases of test_dropin.py::test_search_by_attribute_matches_reference on a table of a few blocks, with the crossover at 0 rows so that the
    full scans run through eps_index_select: filters (device programs), skip / limit windows, deletes; primary-key lists and a STRING filter
    keep the host loop and must still agree."""
    monkeypatch.setenv("EPS_DROPIN_SELECT_MIN_ROWS", "0")
    ref = Ref()
    n = 3 * B + 300
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "Tag", "dataType": "STRING"},
                                       {"name": "Price", "dataType": "FLOAT"},
                                       {"name": "Flag", "dataType": "BOOL"},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 4, "metricType": "EUCLIDEAN"}]}
    rng = np.random.default_rng(31)
    X = rng.random((n, 4), dtype=np.float32)
    price = rng.random(n)
    recs = [{"ID": int(i), "Tag": "t%d" % (i % 5), "Price": float(np.float32(price[i])), "Flag": bool(i % 3 == 0), "V": [float(x) for x in X[i]]}
            for i in range(n)]
    gone = [7, 8, 9, 200, B - 1, B, 2 * B + 5, n - 1]
    cases = [dict(), dict(flt="ID < 50"), dict(flt="Tag = 't3' AND ID >= 100"), dict(skip=10, limit=25), dict(flt="ID > 5", skip=3, limit=7),
             dict(pks=[5, 7, 250, 9999, 12]), dict(pks=[250, 5], flt="ID < 100"), dict(limit=0), dict(skip=1000, limit=10),
             dict(flt="ID < %d" % (n // 2), limit=n), dict(flt="ID % 7 < 3 AND (Price > 0.5 OR Flag = true)", skip=B // 2 - 20, limit=B),
             dict(flt="NOT (Price * 2 > 1.5)", skip=2 * B, limit=n), dict(flt="@distance < 1 AND ID >= %d" % (B - 3), limit=9),
             dict(flt="ID > %d" % (2 * n)), dict(skip=n - 20, limit=100), dict(skip=10 * n, limit=5), dict(limit=10 * n),
             dict(flt="Tag = 't1'", skip=40, limit=500)]
    out = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        db = lib.db(str(tmp_path / name))
        assert db.create_table(schema) == 0
        for s in range(0, n, 1000):
            assert db.insert("T", recs[s:s + 1000]) == 0
        assert db.delete("T", gone) == 0
        out.append([db.get("T", fields=("ID", "Tag"), **kw) for kw in cases])
        db.close()
    nonempty = 0
    for kw, a, b in zip(cases, out[0], out[1]):
        assert a[0] == b[0] == 0, (kw, a[0], b[0])
        assert a == b, (kw, len(a[1]), len(b[1]), a[1][:3], b[1][:3])
        nonempty += len(a[1]) > 0
    assert nonempty >= len(cases) - 5
