"""GpuIndex.search_groups / eps_index_search_groups on the MI355X: the k closest groups per query, each by its closest visible row, by the page
engine (groups_first_kernel over pages of a flat search), the scan engine (groups_min_scan_kernel: a 64-bit atomicMin per (query, group)) and
their combination (csrc/groups.hip).

Every comparison is for equality of ids, distance bits, group keys and counts.  Tables of ties (coordinates -8 .. 8, or those / 16 for COSINE:
every fp32 sum is exact in any order, and full of equal distances, so the row order decides) are held to tests/groups_ref.py, which is checked on
the CPU in tests/test_groups_ref_cpu.py.  Continuous tables are held to the device's own flat search with k = n, deduplicated in numpy: the rule
is defined on those bits, and the flat search itself is held to fp64 by the exact pins."""
import numpy as np
import pytest

import exact_ref as er
import groups_ref as gr
import select_ref as sr
import stream_gate as sg
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
ENGINES = ("auto", "pages", "scan")
KS = (1, 7, 64, 65, 1024)
NQS = (1, 3, 4, 5, 9)


def index(X, metric, keys=None):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    ix.attach_rows(X)
    if keys is not None:
        ix.set_groups(keys)
    return ix


def all_engines(ix, Q, k, want, what, **kw):
    """the three engine settings against `want`, position by position"""
    for engine in ENGINES:
        gr.same(ix.search_groups(Q, k, engine=engine, **kw), want, "%s engine %s" % (what, engine))


# ---- 1. tables of ties against the model: every metric, size, width, batch, k and layout, all three engines
@pytest.mark.parametrize("d", [8, 20, 96])   # 16-byte form G = 2 | G = 8 (20 = 5 pieces: three lanes idle in the last) | G = 32
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3000])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ties_tables_equal_the_model(metric, n, d):
    X, Q, d32 = gr.ties_table(metric, n, d, max(NQS), seed=metric)
    ix = index(X, metric)
    for name, keys in gr.layouts(n, seed=metric).items():
        ix.set_groups(keys)
        info = ix.groups_info()
        sizes = np.unique(keys, return_counts=True)[1]
        assert info["n_groups"] == len(sizes) and info["largest_group"] == sizes.max(), (name, info)
        for k in KS:
            want = gr.numpy_groups(d32, keys, k)   # (queries are answered one by one: a smaller batch is a prefix)
            for nq in NQS:
                w = tuple(a[:nq] for a in want)
                all_engines(ix, Q[:nq], k, w, "%s n %d d %d nq %d k %d" % (name, n, d, nq, k))
            if name == "every row its own":   # a cross-check that needs no model: the flat search itself, bit for bit
                ids, dist, cnt = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
                got = ix.search_groups(Q, k)
                gr.same(got, (ids, dist, np.where(ids >= 0, keys[np.maximum(ids, 0)], 0), cnt), "against eps_index_search, n %d d %d k %d" % (n, d, k))
    ix.close()


# ---- 2. continuous tables: the device's own flat search with k = n, deduplicated in numpy
def dedupe(ids, dist, keys, k):
    """the ordered walk over a flat search's full answer"""
    nq = len(ids)
    out = (np.full((nq, k), -1, np.int64), np.full((nq, k), np.inf, F), np.zeros((nq, k), np.int64), np.zeros(nq, np.int32))
    for q in range(nq):
        valid = ids[q] >= 0
        g = keys[ids[q][valid]]
        first = np.sort(np.unique(g, return_index=True)[1])[:k]   # first occurrence of every key, in answer order
        m = len(first)
        out[0][q, :m], out[1][q, :m], out[2][q, :m], out[3][q] = ids[q][valid][first], dist[q][valid][first], g[first], m
    return out


@pytest.mark.parametrize("name,metric", [("gaussian", 0), ("embedding-like", 1), ("gaussian x 3 queries", 2)])
def test_continuous_tables_equal_the_deduplicated_flat_search(name, metric):
    n, d, nq = 3000, 64, 9
    X, Q = er.make(name, n, d, nq, seed=5)
    ix = index(X, metric)
    full = ix.search(Q, n, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    assert (full[2] == n).all()
    for lname, keys in gr.layouts(n, seed=5).items():
        ix.set_groups(keys)
        for k in (1, 10, 100, 1024):
            want = dedupe(full[0], full[1], keys, k)
            all_engines(ix, Q, k, want, "%s %s k %d" % (name, lname, k))
            for fe in ("stream", "mfma", "mfma_i8"):
                for engine in ("auto", "pages"):
                    gr.same(ix.search_groups(Q, k, engine=engine, flat_engine=fe), want, "%s %s k %d flat %s engine %s" % (name, lname, k, fe, engine))
    ix.close()


# ---- 3. the adversarial table: one group owns the closest rows
def adversarial(n, near, d=20, nq=3, seed=1):
    """`near` rows with coordinates -2 .. 2 in ONE group, the others at 8 (up to two coordinates at -8) in groups of their own, queries in -1 .. 1:
    for every query the group's rows are the `near` closest of the table (<= 9 d against >= 49 d); for a query at 8 everywhere the others are
    (<= 512 against >= 36 d).  Shuffled, so that nothing is positional"""
    rng = np.random.default_rng(seed)
    X = np.full((n, d), 8, F)
    for r in range(near, n):
        X[r, rng.choice(d, size=int(rng.integers(0, 3)), replace=False)] = -8
    X[:near] = rng.integers(-2, 3, (near, d)).astype(F)
    keys = np.arange(n, dtype=np.int64) + 100
    keys[:near] = -5
    o = rng.permutation(n)
    X, keys = np.ascontiguousarray(X[o]), keys[o]
    Q = rng.integers(-1, 2, (nq, d)).astype(F)
    d32 = gr.assert_ties_table(X, Q, 0)
    assert (np.sort(d32[keys == -5], axis=0)[-1] < d32[keys != -5].min(axis=0)).all()
    return X, Q, keys, d32


def test_adversarial_table_auto_hands_the_queries_to_the_scan():
    X, Q, keys, d32 = adversarial(3000, 2900)
    ix = index(X, 0, keys)
    want = gr.numpy_groups(d32, keys, 10)
    assert (want[3] == 10).all() and (want[2][:, 0] == -5).all()
    gr.same(ix.search_groups(Q, 10, engine="auto"), want, "auto")
    info = ix.groups_info()
    assert info["last_scan_queries"] == len(Q) and info["last_engines"] == ("pages", "scan") and info["largest_group"] == 2900, info
    st = ix.stats()
    assert st["main_kernel_bits"] == 32 and st["main_kernel_rows"] == 3000 and st["main_kernel_ms"] > 0, st
    gr.same(ix.search_groups(Q, 10, engine="scan"), want, "scan")
    assert ix.groups_info()["last_engines"] == ("scan",) and ix.groups_info()["last_scan_queries"] == len(Q)
    gr.same(ix.search_groups(Q, 10, engine="pages"), want, "pages")   # 2900 / 64 pages: exact, only slow
    assert ix.groups_info()["last_engines"] == ("pages",) and ix.groups_info()["last_scan_queries"] == 0
    # a benign layout on the same rows: the page answers, the scan does not run
    ix.set_groups(np.arange(3000, dtype=np.int64) // 4)
    ix.search_groups(Q, 10, engine="auto")
    assert ix.groups_info()["last_engines"] == ("pages",) and ix.groups_info()["last_scan_queries"] == 0
    # ... and a batch of which only some queries are unfinished after the page: exactly those go to the scan
    far = np.full((1, X.shape[1]), 8, F)   # close to the rows at +-8: its page is full of distinct groups
    Q2 = np.concatenate([Q[:1], far, Q[1:]])
    ix.set_groups(keys)
    got = ix.search_groups(Q2, 10, engine="auto")
    gr.same(got, gr.numpy_groups(gr.assert_ties_table(X, Q2, 0), keys, 10), "a mixed batch")
    assert ix.groups_info()["last_scan_queries"] == 3
    ix.close()


def test_pages_of_16_rows_take_several_rounds():
    X, Q, keys, d32 = adversarial(300, 280)
    ix = index(X, 0, keys)
    want = gr.numpy_groups(d32, keys, 10)
    gr.same(ix.search_groups(Q, 10, engine="pages", page_rows=16, flat_engine="stream"), want, "pages of 16")
    assert ix.stats()["main_kernel_launches"] >= 280 // 16, ix.stats()   # one stream scan per round
    for P in (1, 7, 64, 1024):
        gr.same(ix.search_groups(Q, 10, engine="pages", page_rows=P), want, "pages of %d" % P)
        gr.same(ix.search_groups(Q, 10, engine="auto", page_rows=P), want, "auto, a page of %d" % P)
    gr.same(ix.search_groups(Q, 1024, engine="pages", page_rows=16), gr.numpy_groups(d32, keys, 1024), "k beyond the groups, pages of 16")
    ix.close()


def test_a_page_of_1024_labels_that_collide_in_the_lds_table():
    """every row its own group, label = row; the rows 4096 i are the 1024 closest (distance 0): the page holds 1024 distinct labels congruent
    modulo the table's 4096 slots - one probe chain through a quarter of the table"""
    n, d, k = 4096 * 1023 + 1, 4, 1024
    X = np.ones((n, d), F)
    X[::4096] = 0
    Q = np.zeros((1, d), F)
    keys = np.arange(n, dtype=np.int64) * 3 - 7   # (ascending: label = row)
    ix = index(X, 0, keys)
    assert ix.groups_info()["n_groups"] == n
    rows = np.arange(k, dtype=np.int64)[None, :] * 4096
    want = (rows, np.zeros((1, k), F), rows * 3 - 7, np.array([k], np.int32))
    gr.same(ix.search_groups(Q, k, engine="pages"), want, "pages")
    gr.same(ix.search_groups(Q, k, engine="pages", page_rows=512), want, "pages of 512: 512 carried labels of the same chain")
    flat = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    assert np.array_equal(flat[0], rows)
    ix.close()


# ---- 4. one table for the cases around visibility, buffers and refusals
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


@pytest.fixture(scope="module")
def table4():
    n, d, nq = 3000, 20, 9
    X, Q, d32 = gr.ties_table(0, n, d, nq, seed=4)
    keys = gr.layouts(n, seed=4)["n / 8 groups"] * 11 - 2000
    ix = index(X, 0, keys)
    yield ix, X, Q, d32, keys
    ix.close()


def reset(ix):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)


def packbits(hidden):
    return np.packbits(np.concatenate([hidden, np.zeros(-len(hidden) % 8, bool)]), bitorder="little")


def test_scratch_bytes_forcing_three_chunks_at_nine_queries(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    G = ix.groups_info()["n_groups"]
    for k in (7, 130):
        want = gr.numpy_groups(d32, keys, k)
        for scratch in (4 * G * 8, 1, 5 * G * 8, 8 * G * 8, 0):   # room for 4 (4 + 4 + 1), below one chunk (still 4), 4, 8 (8 + 1), the default
            gr.same(ix.search_groups(Q, k, engine="scan", scratch_bytes=scratch), want, "k %d scratch %d" % (k, scratch))
        assert ix.stats()["dist_evals"] == len(Q) * len(X)


def test_a_deleted_representative_and_a_group_entirely_invisible(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    free = gr.numpy_groups(d32, keys, 7)
    hidden = np.zeros(len(X), bool)
    hidden[free[0][:, :3].reshape(-1)] = True    # the first three representatives of every query: their groups' next rows take over
    hidden[keys == free[2][0, 4]] = True         # ... and one group of query 0's answer altogether
    ix.set_deleted(packbits(hidden))
    for k in (7, 64, 1024):
        want = gr.numpy_groups(d32, keys, k, visible=~hidden)
        assert not (want[2] == free[2][0, 4]).any()
        all_engines(ix, Q, k, want, "deleted k %d" % k)
    assert np.isin(free[2][0, :3], gr.numpy_groups(d32, keys, 1024, visible=~hidden)[2][0]).all()   # (the groups are still there)
    reset(ix)


def test_int_column_program_with_distance_and_id_map(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(3)
    col = rng.integers(-100, 100, n).astype(np.int32)
    ix.set_int_filter(col, "<", 13)
    vis = sr.visible_rows(n, int_filter=(col, "<", 13))
    for k in (7, 130):
        all_engines(ix, Q, k, gr.numpy_groups(d32, keys, k, visible=vis), "int column k %d" % k)
    reset(ix)
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    t = float(np.sort(d32, axis=0)[400].min())   # an integer some row's distance EQUALS: `<=` keeps it
    assert (d32 == F(t)).any()
    prog = [("dist",), ("const", t), ("<=",), ("f32", 4), ("const", 0.3), (">",), ("and",)]
    ix.set_filter_program(prog, rows)
    vis = np.stack([sr.visible_rows(n, program=prog, rows=rows, dist=d32[:, q].astype(np.float64)) for q in range(d32.shape[1])], axis=1)
    blind = gr.numpy_groups(d32, keys, 1024, visible=sr.visible_rows(n, program=prog, rows=rows, dist=np.zeros(n)))
    ix.set_id_map(3, 8)
    for k in (7, 64, 1024):
        want = gr.numpy_groups(d32, keys, k, visible=vis)
        want = (np.where(want[0] >= 0, want[0] * 8 + 3, -1),) + want[1:]
        all_engines(ix, Q, k, want, "program with @distance, id map, k %d" % k)
        if k == 1024:
            assert (want[3] < blind[3]).all()   # (@distance read as 0 would show: more groups have a visible row)
            assert (want[1][np.isfinite(want[1])] <= F(t)).all()
    reset(ix)


def test_nan_rows_sort_last_and_a_group_of_nans_is_a_group():
    n, d, nq = 300, 8, 3
    X, Q, d32 = gr.ties_table(0, n, d, nq, seed=8)
    X = X.copy()
    keys = (np.arange(n, dtype=np.int64) // 6) * 5
    X[[0, 1, 2, 3, 4, 5, 17, 40], 0] = np.nan   # group 0 entirely NaN, rows of two other groups
    d32 = d32.copy()
    d32[[0, 1, 2, 3, 4, 5, 17, 40]] = np.nan
    ix = index(X, 0, keys)
    for k in (7, 50, 64):
        want = gr.numpy_groups(d32, keys, k)
        all_engines(ix, Q, k, want, "NaN rows k %d" % k)
    want = gr.numpy_groups(d32, keys, 64)
    assert (want[3] == 50).all() and (want[0][:, 49] == 0).all() and np.isnan(want[1][:, 49]).all() and (want[0][:, 50:] == -1).all()
    ix.close()


def test_equal_distances_inside_and_across_groups():
    n, d = 512, 8
    X = np.zeros((n, d), F)
    X[:, 0] = np.arange(n) % 4   # four distances, 128 rows each
    Q = np.zeros((2, d), F)
    Q[1, 0] = 3
    keys = np.random.default_rng(2).integers(0, 40, n).astype(np.int64) - 20
    d32 = gr.assert_ties_table(X, Q, 0)
    ix = index(X, 0, keys)
    for k in (1, 7, 40, 64):
        all_engines(ix, Q, k, gr.numpy_groups(d32, keys, k), "ties k %d" % k, page_rows=16)
        all_engines(ix, Q, k, gr.numpy_groups(d32, keys, k), "ties k %d" % k)
    ix.close()


def test_device_and_host_buffers(table4):
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq = len(Q)
    for k in (7, 130):
        want = gr.numpy_groups(d32, keys, k)
        for engine in ENGINES:
            got = ix.search_groups(Q, k, engine=engine)
            assert all(isinstance(a, np.ndarray) for a in got)
            dq = torch.from_numpy(Q).cuda()
            torch.cuda.synchronize()
            out = ix.search_groups(dq, k, engine=engine)
            assert all(hasattr(t, "data_ptr") for t in out)
            ix.synchronize()
            gr.same([t.cpu().numpy() for t in out], want, "device k %d %s" % (k, engine))
    want = gr.numpy_groups(d32, keys, 10)
    mine = (np.full((nq, 10), -7, np.int64), np.zeros((nq, 10), F), np.full((nq, 10), -7, np.int64), np.zeros(nq, np.int32))
    out = ix.search_groups(Q, 10, out=mine)
    assert out[0] is mine[0]
    gr.same(out, want, "out= host")
    dmine = (torch.full((nq, 10), -7, dtype=torch.int64, device="cuda"), torch.zeros((nq, 10), dtype=torch.float32, device="cuda"),
             torch.full((nq, 10), -7, dtype=torch.int64, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    out = ix.search_groups(Q, 10, out=dmine)   # host queries, device results
    ix.synchronize()
    gr.same([t.cpu().numpy() for t in out], want, "host in, device out")
    p = lambda a: a.ctypes.data   # noqa: E731
    assert ix.L.eps_index_search_groups(ix.h, p(Q), nq, 10, None, 0, 0, 0, p(mine[0]), p(mine[1]), p(mine[2]), None) == 0   # counts_out and p may be NULL
    gr.same(mine[:3], want[:3], "no counts")
    dkeys = torch.from_numpy(keys).cuda()   # keys from device memory
    torch.cuda.synchronize()
    ix.set_groups(dkeys)
    gr.same(ix.search_groups(Q, 10), want, "device keys")
    ix.set_groups(keys)


def test_host_queries_are_consumed_when_the_call_returns(table4):
    """device outputs, the scan engine (no host sync of its own), a gate in front; straight after the call returns the page-locked query array is
    overwritten with the decoy from the host: a copy still pending then would take the decoy"""
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq, k = len(Q), 10
    decoy = er.make(gr.TIES[0], len(X), X.shape[1], nq, seed=404)[1]
    want, want_decoy = gr.numpy_groups(d32, keys, k), gr.numpy_groups(gr.assert_ties_table(X, decoy, 0), keys, k)
    sg.differ_first(want[0], want_decoy[0], "search_groups host queries")
    s = torch.cuda.Stream()
    sg.calibrate()
    ix.set_stream(s.cuda_stream)
    try:
        host = sg.pinned(Q.shape, Q.dtype)
        make_outs = lambda: (torch.full((nq, k), sg.FILL, dtype=torch.int64, device="cuda"), torch.full((nq, k), sg.FILL, dtype=torch.float32, device="cuda"),   # noqa: E731
                             torch.full((nq, k), sg.FILL, dtype=torch.int64, device="cuda"), torch.full((nq,), sg.FILL, dtype=torch.int32, device="cuda"))

        def issue(outs=None):
            host[...] = Q
            ix.search_groups(host, k, engine="scan", out=outs or make_outs())
            host[...] = decoy
        ms = sg.gate_for("search_groups, page-locked host queries", issue, s)
        outs = make_outs()
        torch.cuda.synchronize()
        sg.gate(s, ms)
        host[...] = Q
        ix.search_groups(host, k, engine="scan", out=outs)
        host[...] = decoy
        s.synchronize()
        gr.same([t.cpu().numpy() for t in outs], want, "the host array was read after the call returned")
    finally:
        ix.set_stream(None)


def test_search_groups_leaves_no_trace(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    for kw in (dict(flat_engine=amd.FLAT_STREAM), dict(flat_engine=amd.FLAT_MFMA_I8), dict(flat_engine=amd.FLAT_AUTO)):
        before = ix.search(Q, 10, mode=amd.MODE_FLAT, **kw)
        st_before = ix.stats()
        for engine in ENGINES:
            ix.search_groups(Q, 10, engine=engine)
        after = ix.search(Q, 10, mode=amd.MODE_FLAT, **kw)
        st_after = ix.stats()
        for a, b in zip(before, after):
            assert np.array_equal(a, b), kw
        for f in ("one_pass", "i8_rotated", "main_kernel_bits", "main_kernel_rows", "main_kernel_queries"):
            assert st_before[f] == st_after[f], (kw, f, st_before[f], st_after[f])


# ---- 5. refusals: each leaves the handle usable
def test_refusals(table4):
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq = len(Q)
    want = gr.numpy_groups(d32, keys, 10)

    def usable():
        gr.same(ix.search_groups(Q, 10), want, "after a refusal")

    for k in (0, 1025, -1):
        with pytest.raises(EpsillaError) as e:
            ix.search_groups(Q, k)
        assert e.value.code == 30000 and "k must be" in str(e.value)
        usable()
    for kw, text in ((dict(page_rows=1025), "page_rows"), (dict(page_rows=-1), "page_rows"), (dict(scratch_bytes=-1), "scratch_bytes"), (dict(engine=3), "engine")):
        with pytest.raises((EpsillaError, KeyError)) as e:
            ix.search_groups(Q, 10, **kw)
        assert isinstance(e.value, KeyError) or (e.value.code == 30000 and text in str(e.value)), kw
        usable()
    p = lambda a: a.ctypes.data   # noqa: E731
    host = [np.empty((nq, 10), np.int64), np.empty((nq, 10), F), np.empty((nq, 10), np.int64), np.empty(nq, np.int32)]
    dev = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):   # the wrapper refuses a mixed set, and so does the library
        ix.search_groups(Q, 10, out=(host[0], host[1], dev, host[3]))
    rc = ix.L.eps_index_search_groups(ix.h, p(Q), nq, 10, None, 0, 0, 0, p(host[0]), p(host[1]), dev.data_ptr(), p(host[3]))
    assert rc == 30000 and "host or all be device" in ix.L.eps_index_last_error(ix.h).decode()
    assert ix.L.eps_index_search_groups(ix.h, p(Q), nq, 10, None, 3, 0, 0, p(host[0]), p(host[1]), p(host[2]), p(host[3])) == 30000   # engine 3
    assert ix.L.eps_index_search_groups(ix.h, None, nq, 10, None, 0, 0, 0, p(host[0]), p(host[1]), p(host[2]), p(host[3])) == 30000   # null queries
    assert ix.L.eps_index_search_groups(ix.h, p(Q), nq, 10, None, 0, 0, 0, p(host[0]), p(host[1]), None, p(host[3])) == 30000          # null group keys
    assert ix.L.eps_index_search_groups(ix.h, None, 0, 10, None, 0, 0, 0, None, None, None, None) == 0                                  # nq = 0
    usable()
    with pytest.raises(EpsillaError) as e:
        ix.set_groups(keys[:-1])
    assert e.value.code == 30000 and "row count" in str(e.value)
    with pytest.raises(EpsillaError) as e:   # (a refused set_groups leaves no groups behind)
        ix.search_groups(Q, 10)
    assert e.value.code == 30000 and "no groups" in str(e.value)
    ix.set_groups(keys)
    usable()
    ix.set_groups(None)   # forgotten
    assert ix.groups_info()["n_groups"] == 0
    with pytest.raises(EpsillaError) as e:
        ix.search_groups(Q, 10)
    assert e.value.code == 30000 and "no groups" in str(e.value)
    ix.set_groups(keys)
    usable()
    # stale labels after an append, and after a new table
    ix2 = index(X[:100], 0, keys[:100])
    assert (ix2.search_groups(Q, 3)[3] == 3).all()
    ix2.append_rows(np.zeros((8, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        ix2.search_groups(Q, 3)
    assert e.value.code == 30000 and "set_groups" in str(e.value)
    ix2.set_groups(np.concatenate([keys[:100], keys[:8]]))
    assert (ix2.search_groups(Q, 3)[3] == 3).all()
    ix2.attach_rows(X[:108])
    with pytest.raises(EpsillaError) as e:
        ix2.search_groups(Q, 3)
    assert e.value.code == 30000 and "set_groups" in str(e.value)
    ix2.close()
    # a sharded handle: all three
    sh = amd.GpuIndex(X.shape[1], "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(np.zeros((300, X.shape[1]), F))
    for call in (lambda: sh.set_groups(np.zeros(300, np.int64)), lambda: sh.search_groups(Q, 10), lambda: sh.groups_info()):
        with pytest.raises(EpsillaError) as e:
            call()
        assert e.value.code == 50002 and "shard" in str(e.value)
    sh.search(Q, 3, mode=amd.MODE_FLAT)
    sh.close()
    # an index without rows: no group has a row
    empty = amd.GpuIndex(X.shape[1], "EUCLIDEAN", device=0)
    empty.set_groups(np.zeros(0, np.int64))
    got = empty.search_groups(Q, 4)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and (got[2] == 0).all() and (got[3] == 0).all()
    empty.close()
