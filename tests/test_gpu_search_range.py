"""GpuIndex.search_range / eps_index_search_range on the MI355X: every visible row within a radius of the query, the count of them, the cap closest in
(distance, id) order - on the stream form (range_scan_kernel) and on the matrix form (one launch of the lower-bound filter + range_rerank_kernel),
ordered by range_order_kernel (csrc/range.hip).

Integer tables (coordinates -8 .. 8: every fp32 squared L2 and dot product is exact in any order; radii at half-integers, so no distance equals
one) are held to numpy's answer exactly: ids, distance bits, counts, totals - hence the three engines to each other, bit for bit.  The continuous
table is held to tests/range_ref.py (checked on the CPU in tests/test_range_ref_cpu.py, which also keeps the run that shows its radii sit in wide
enough gaps).  A batch of three queries cannot mix four kinds of radius: it takes one row / a few dozen / the whole table, and the batch of 70
all four."""
import numpy as np
import pytest

import exact_ref as er
import range_ref as rr
import select_ref as sr
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
ENGINES = ("stream", "mfma", "mfma_i8")
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
ENGINE_FIELDS = ("one_pass", "i8_rotated", "main_kernel_bits")


def same(a, b, what=""):
    """ids, distance bits, counts, totals"""
    for x, y, name in zip(a, b, ("ids", "dist", "counts", "totals")):
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


def mixed_radii(d32, kinds):
    """per query a half-integer radius of the kind asked for (cyclic); 'one' where the query's closest row is unique, else 'few'"""
    s = np.sort(d32, axis=0)
    out, got = np.empty(d32.shape[1], F), []
    for q in range(d32.shape[1]):
        kind = kinds[q % len(kinds)]
        if kind == "one" and s[0, q] == s[1, q]:
            kind = "few"
        # ("edge": an integer radius that IS the 31st distance - rows with dist == r belong to the answer)
        out[q] = {"empty": s[0, q] - F(0.5), "one": s[0, q] + F(0.5), "few": s[30, q] + F(0.5), "edge": s[30, q], "all": s[-1, q] + F(0.5)}[kind]
        got.append(kind)
    return out, got


# ---- 1. integer tables: numpy's set, order and totals exactly, on every engine
@pytest.mark.parametrize("nq", [3, 70])
@pytest.mark.parametrize("d", [19, 64])
@pytest.mark.parametrize("n,appended", [(1000, 0), (2600, 2)])
@pytest.mark.parametrize("metric", [0, 2])
def test_integer_tables_equal_numpy_on_every_engine(metric, n, appended, d, nq):
    X, Q = er.make("integers -8..8", n, d, nq, seed=metric)
    d32 = rr.dist32(X, Q, metric)
    cap = 64
    ix = index(X, metric, appended)
    for kinds in ((("one", "few", "all") if nq == 3 else ("empty", "one", "few", "all")), (("edge", "one", "few") if nq == 3 else ("empty", "one", "few", "edge"))):
        radius, got = mixed_radii(d32, kinds)
        assert set(got) == set(kinds), got
        want = rr.numpy_range(d32, radius, cap)
        assert "edge" not in kinds or (want[1][np.arange(nq), want[2] - 1] == radius)[np.array(got) == "edge"].all()   # (the last row returned lies AT the radius)
        assert ("all" in kinds) == bool((want[3] == n).any()) and (("one" not in kinds) or (want[3] == 1).any()) and (("empty" not in kinds) or (want[3] == 0).any())
        over = int((want[3] > cap).sum())
        assert (over > 0) == ("all" in kinds)
        for eng in ENGINES:
            ans = ix.search_range(Q, radius, cap, flat_engine=eng)
            same(ans, want, "%s %s" % (eng, kinds))
            st = ix.stats()
            assert st["overflow_queries"] == over, (eng, kinds, st["overflow_queries"], over)
            assert st["main_kernel_bits"] in {"stream": (32,), "mfma": (16,), "mfma_i8": (8, 16)}[eng], (eng, st)   # (8-bit may decline a table: test_uniform_rows_run_the_8_bit_form)
            assert st["main_kernel_rows"] == n and st["main_kernel_launches"] >= 1
            if eng != "stream":
                assert st["rerank_rows"] >= int(np.minimum(want[3], n).sum())   # every member was a candidate
    ix.close()


# ---- 1b. host results come back as one block [ids | totals | distances | counts]: in one page-locked copy split on the host, or - EPS_HOST_STAGING=0,
# and where page-locked memory cannot be had - in one pageable copy per array.  Both split the block the same way.
@pytest.mark.parametrize("staging", [None, "0"])
def test_host_results_with_and_without_page_locked_staging(monkeypatch, staging):
    if staging is None:
        monkeypatch.delenv("EPS_HOST_STAGING", raising=False)
    else:
        monkeypatch.setenv("EPS_HOST_STAGING", staging)
    n, d, nq, cap = 1000, 19, 3, 64
    X, Q = er.make("integers -8..8", n, d, nq, seed=0)
    d32 = rr.dist32(X, Q, 0)
    radius, got = mixed_radii(d32, ("one", "few", "all"))
    want = rr.numpy_range(d32, radius, cap)
    over = int((want[3] > cap).sum())
    assert over > 0 and (want[2] < cap).any()   # (full and partly filled lists: a part read at the wrong offset shows)
    ix = index(X, 0)
    for eng in ENGINES:
        same(ix.search_range(Q, radius, cap, flat_engine=eng), want, "%s staging=%r" % (eng, staging))
        assert ix.stats()["overflow_queries"] == over, (eng, staging)
    ix.close()


# ---- 2. the continuous table: range_ref under the 5 % cap, distances bit-equal to a flat search's
@pytest.fixture(scope="module")
def cont():
    X, Q = er.make("embedding-like", 3000, 96, 40)
    return X, Q, {m: er.Ref(X, Q, m) for m in (0, 1)}


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("cap", [64, 8])
def test_continuous_table_against_the_fp64_reference(cont, metric, cap):
    X, Q, refs = cont
    ref = refs[metric]
    radius = rr.midway_radii(ref, 20)
    ix = index(X, metric)
    flat = ix.search(Q, cap, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    first = None
    for eng in ENGINES:
        ans = ix.search_range(Q, radius, cap, flat_engine=eng)
        und, must = rr.check_range(*ans, ref, radius, cap, what="%s metric %d" % (eng, metric))
        print("%s metric %d cap %d: %d undecided rows, %d certain members" % (eng, metric, cap, und, must))
        rr.assert_cap(und, must)
        for q in range(ref.nq):   # the same rows, the same bits as the flat search returns for them
            m = int(ans[2][q])
            assert np.array_equal(ans[0][q, :m], flat[0][q, :m]) and np.array_equal(ans[1][q, :m].view(np.uint32), flat[1][q, :m].view(np.uint32)), (eng, q)
        first = first or ans
        same(ans, first, eng)
        assert ix.stats()["overflow_queries"] == int((ans[3] > cap).sum())
    ix.close()


# ---- 2b. the 8-bit form itself: U[0,1) rows, which the 8-bit mirror always serves (tests/test_gpu_mfma_i8.py) - no silent hand-over to fp16
@pytest.mark.parametrize("metric", [0, 2])
def test_uniform_rows_run_the_8_bit_form(metric):
    X, Q = er.make("uniform", 3000, 96, 40)
    ref = er.Ref(X, Q, metric)
    radius = rr.midway_radii(ref, 20)
    cap = 64
    ix = index(X, metric)
    first = None
    for eng, bits in (("stream", 32), ("mfma", 16), ("mfma_i8", 8)):
        ans = ix.search_range(Q, radius, cap, flat_engine=eng)
        st = ix.stats()
        assert st["main_kernel_bits"] == bits and st["overflow_queries"] == 0, (eng, st)
        assert eng == "stream" or 20 * ref.nq <= st["rerank_rows"] < ref.nq * ref.n, (eng, st)   # every member was a candidate, and the pass FILTERS
        und, must = rr.check_range(*ans, ref, radius, cap, what="%s metric %d" % (eng, metric))
        print("uniform %s metric %d: %d undecided rows, %d certain members, %d candidates" % (eng, metric, und, must, st["rerank_rows"]))
        rr.assert_cap(und, must)
        first = first or ans
        same(ans, first, eng)
    ix.close()


# ---- 2c. a candidate list too short for what the filter passes: the query runs again on the stream form (and, here, takes its cap closest from
# the flat scan after that); each such query is counted once, and queries answered from their lists sit in the same batch
@pytest.mark.parametrize("metric", [0, 2])
def test_candidate_overflow_is_rescanned(metric):
    n, nq, cap = 9000, 6, 64   # (cap 64: 8192 candidate slots per query, fewer than the table's rows)
    X, Q = er.make("integers -8..8", n, 19, nq, seed=20 + metric)
    d32 = rr.dist32(X, Q, metric)
    radius, got = mixed_radii(d32, ("all", "few", "edge"))
    radius[3] = np.inf
    want = rr.numpy_range(d32, radius, cap)
    big = int((want[3] == n).sum())
    assert big == 2 and int((want[3] > cap).sum()) == big and (want[3] > 0).all()
    ix = index(X, metric)
    for eng in ENGINES:
        same(ix.search_range(Q, radius, cap, flat_engine=eng), want, eng)
        st = ix.stats()
        assert st["overflow_queries"] == big, (eng, st)
        # the pass over all queries + (matrix form: the stream form again for the overflowing queries) + their flat scan
        assert st["dist_evals"] == (nq + (1 if eng == "stream" else 2) * big) * n, (eng, st)
        assert st["main_kernel_bits"] in {"stream": (32,), "mfma": (16,), "mfma_i8": (8, 16)}[eng]
    ix.close()


# ---- 3. visibility
N3, D3 = 1000, 19
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


@pytest.fixture(scope="module")
def table3():
    X, Q = er.make("integers -8..8", N3, D3, 5, seed=3)
    d32 = rr.dist32(X, Q, 0)
    radius = (np.sort(d32, axis=0)[120] + F(0.5)).astype(F)
    rng = np.random.default_rng(3)
    rows = np.zeros(N3, ROW8)
    rows["a"] = rng.integers(-100, 100, N3)
    rows["x"] = rng.random(N3, dtype=F)
    ix = index(X, 0)
    yield ix, Q, d32, radius, rows
    ix.close()


def reset(ix):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)


def check3(ix, Q, d32, radius, vis, cap=256, base=0, stride=1):
    want = rr.numpy_range(d32, radius, cap, visible=vis)
    assert 0 < want[3].min() and (want[3] < rr.numpy_range(d32, radius, cap)[3]).all()   # (the filter bites, and leaves something)
    want = (np.where(want[0] >= 0, want[0] * stride + base, -1),) + want[1:]
    for eng in ENGINES:
        same(ix.search_range(Q, radius, cap, flat_engine=eng), want, eng)


def test_deleted_bitset(table3):
    ix, Q, d32, radius, rows = table3
    reset(ix)
    deleted = np.packbits(np.random.default_rng(5).random((N3 + 7) // 8 * 8) < 0.4, bitorder="little")
    ix.set_deleted(deleted)
    check3(ix, Q, d32, radius, sr.visible_rows(N3, deleted=deleted))
    ix.set_id_map(7, 3)
    check3(ix, Q, d32, radius, sr.visible_rows(N3, deleted=deleted), base=7, stride=3)


def test_int_column(table3):
    ix, Q, d32, radius, rows = table3
    reset(ix)
    col = np.ascontiguousarray(rows["a"])
    ix.set_int_filter(col, "<", 13)
    check3(ix, Q, d32, radius, sr.visible_rows(N3, int_filter=(col, "<", 13)))


def test_program_reads_the_exact_distance_on_every_engine(table3):
    """attr_f32 > c AND @distance < r2, r2 < r: the program cuts at r2 - on the matrix engine too, where a search sends such programs to the stream engine"""
    ix, Q, d32, radius, rows = table3
    reset(ix)
    r2 = float(np.sort(d32, axis=0)[60].min()) + 0.5
    assert (r2 < radius).all()
    prog = [("f32", 4), ("const", 0.3), (">",), ("dist",), ("const", r2), ("<",), ("and",)]
    ix.set_filter_program(prog, rows)
    vis = np.stack([sr.visible_rows(N3, program=prog, rows=rows, dist=d32[:, q].astype(np.float64)) for q in range(d32.shape[1])], axis=1)
    want_d = rr.numpy_range(d32, radius, 256, visible=vis)[1]
    assert (want_d[np.isfinite(want_d)] < r2).all()
    check3(ix, Q, d32, radius, vis)
    reset(ix)


# ---- 4. the cap's edges
def test_cap_one(table3):
    ix, Q, d32, radius, rows = table3
    reset(ix)
    want = rr.numpy_range(d32, radius, 1)
    assert (want[3] > 100).all()
    for eng in ENGINES:
        same(ix.search_range(Q, radius, 1, flat_engine=eng), want, eng)
        assert ix.stats()["overflow_queries"] == len(Q)


def test_cap_8192_orders_a_full_list_and_8193_is_refused():
    X, Q = er.make("integers -8..8", 9000, 19, 2, seed=9)
    d32 = rr.dist32(X, Q, 0)
    radius = (np.sort(d32, axis=0)[7900] + F(0.5)).astype(F)
    want = rr.numpy_range(d32, radius, 8192)
    assert (want[3] > 7900).all() and (want[3] <= 8192).all()
    ix = index(X, 0)
    for eng in ENGINES:
        same(ix.search_range(Q, radius, 8192, flat_engine=eng), want, eng)
        assert ix.stats()["overflow_queries"] == 0
    for cap in (8193, 0, -1):
        with pytest.raises(EpsillaError) as e:
            ix.search_range(Q, radius, cap)
        assert e.value.code == 30000 and "cap" in str(e.value)
    ix.close()


def test_infinite_radius_no_queries_and_an_empty_table():
    X, Q = er.make("integers -8..8", 300, 19, 3, seed=4)
    ix = amd.GpuIndex(19, "EUCLIDEAN", device=0)
    ids, dist, counts, totals = ix.search_range(Q, 5.0, 4)   # no rows attached
    assert (ids == -1).all() and np.isposinf(dist).all() and (counts == 0).all() and (totals == 0).all()
    ix.attach_rows(X)
    d32 = rr.dist32(X, Q, 0)
    for eng in ENGINES:
        same(ix.search_range(Q, np.inf, 16, flat_engine=eng), rr.numpy_range(d32, np.inf, 16), eng)
        same(ix.search_range(Q, -np.inf, 16, flat_engine=eng), rr.numpy_range(d32, -np.inf, 16), eng)
    assert ix.L.eps_index_search_range(ix.h, None, 0, None, 4, None, None, None, None, None) == 0   # nq = 0
    ix.close()


# ---- 5. nothing a later search or select can observe changes
def test_search_range_leaves_no_trace_in_a_search_or_a_select(table3):
    ix, Q, d32, radius, rows = table3
    reset(ix)
    prog = [("i32", 0), ("const", 3), ("%",), ("const", 0), ("=",), ("f32", 4), ("const", 0.5), (">",), ("or",)]
    ix.set_filter_program(prog, rows)
    timing = ("kernel_ms", "main_kernel_ms", "filter_ms_all")
    for kw in (dict(flat_engine=amd.FLAT_STREAM), dict(flat_engine=amd.FLAT_MFMA), dict(flat_engine=amd.FLAT_MFMA_I8)):
        before = ix.search(Q, 10, mode=amd.MODE_FLAT, **kw)
        st_before = {k: v for k, v in ix.stats().items() if k not in timing}
        sel_before = ix.select(3, 200)
        for eng in ENGINES:
            ix.search_range(Q, radius, 64, flat_engine=eng)
        after = ix.search(Q, 10, mode=amd.MODE_FLAT, **kw)
        st_after = {k: v for k, v in ix.stats().items() if k not in timing}
        sel_after = ix.select(3, 200)
        for a, b in zip(before, after):
            assert np.array_equal(a, b), kw
        assert np.array_equal(sel_before[0], sel_after[0]) and sel_before[1] == sel_after[1]
        for f in ENGINE_FIELDS:
            assert st_before[f] == st_after[f], (kw, f, st_before[f], st_after[f])
    reset(ix)


# ---- 6. refusals, device buffers
def test_refusals(table3):
    import torch
    ix, Q, d32, radius, rows = table3
    reset(ix)
    sh = amd.GpuIndex(D3, "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(np.zeros((300, D3), F))
    with pytest.raises(EpsillaError) as e:
        sh.search_range(Q, radius, 8)
    assert e.value.code == 50002 and "shard" in str(e.value)
    sh.close()
    bad = radius.copy()
    bad[1] = np.nan
    with pytest.raises(EpsillaError) as e:
        ix.search_range(Q, bad, 8)
    assert e.value.code == 30000 and "NaN" in str(e.value)
    nq = len(Q)
    host = [np.empty((nq, 8), np.int64), np.empty((nq, 8), F), np.empty(nq, np.int32), np.empty(nq, np.int64)]
    dev = [torch.empty((nq, 8), dtype=torch.int64, device="cuda"), torch.empty((nq, 8), dtype=torch.float32, device="cuda"),
           torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty(nq, dtype=torch.int64, device="cuda")]
    with pytest.raises(ValueError):   # the wrapper refuses a mixed set, and so does the library
        ix.search_range(Q, radius, 8, out=(host[0], dev[1], host[2], host[3]))
    rad = np.ascontiguousarray(radius)
    rc = ix.L.eps_index_search_range(ix.h, Q.ctypes.data, nq, rad.ctypes.data, 8, None, host[0].ctypes.data, dev[1].data_ptr(), host[2].ctypes.data, host[3].ctypes.data)
    assert rc == 30000 and "host or all be device" in ix.L.eps_index_last_error(ix.h).decode()
    # stale filter state after an append
    ix2 = index(er.make("integers -8..8", 100, D3, 1)[0], 0)
    gone = np.zeros(13, np.uint8)
    gone[0] = 1
    ix2.set_deleted(gone)
    ix2.append_rows(np.zeros((8, D3), F))
    with pytest.raises(EpsillaError) as e:
        ix2.search_range(Q, radius, 8)
    assert e.value.code == 30000 and "set_deleted" in str(e.value)
    ix2.close()


def test_device_tensors_in_give_device_tensors_out(table3):
    import torch
    ix, Q, d32, radius, rows = table3
    reset(ix)
    want = rr.numpy_range(d32, radius, 64)
    dq = torch.from_numpy(Q).cuda()
    torch.cuda.synchronize()
    for eng in ENGINES:
        out = ix.search_range(dq, radius, 64, flat_engine=eng)
        assert all(hasattr(t, "data_ptr") for t in out)
        ix.synchronize()
        same([t.cpu().numpy() for t in out], want, eng)
    mine = (torch.full((len(Q), 64), -7, dtype=torch.int64, device="cuda"), torch.zeros((len(Q), 64), dtype=torch.float32, device="cuda"),
            torch.zeros(len(Q), dtype=torch.int32, device="cuda"), torch.zeros(len(Q), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    out = ix.search_range(Q, radius, 64, out=mine)   # host queries, device results
    assert out[0] is mine[0]
    ix.synchronize()
    same([t.cpu().numpy() for t in out], want, "host queries, device outputs")
