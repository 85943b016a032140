"""GpuIndex.search_group_rows / eps_index_search_group_rows on the MI355X: the k closest groups per query as search_groups finds them, and of each
its m closest visible rows and the number of its visible rows (csrc/group_rows.hip: the rows by group, the work list, the segmented gather, the
merge per pair).

Every comparison is for equality of ids, distance bits, group keys, row counts, group sizes and counts.  Tables of ties are held to
tests/group_rows_ref.py, which is checked on the CPU in tests/test_group_rows_ref_cpu.py.  Continuous tables are held to the device's own flat
search with k = n, grouped in numpy: the rule is defined on those bits."""
import numpy as np
import pytest

import exact_ref as er
import group_rows_ref as grr
import groups_ref as gr
import select_ref as sr
import stream_gate as sg
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
ENGINES = ("auto", "pages", "scan")
KS = (1, 7, 65)
MS = (1, 2, 7, 64, 65, 1024)
NQS = (1, 3, 5)
CHUNK = 256   # GROUP_ROWS_CHUNK: the rows of a group one work item walks on tables this small


def index(X, metric, keys=None):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    ix.attach_rows(X)
    if keys is not None:
        ix.set_groups(keys)
    return ix


def all_engines(ix, Q, k, m, want, what, **kw):
    for engine in ENGINES:
        grr.same(ix.search_group_rows(Q, k, m, engine=engine, **kw), want, "%s engine %s" % (what, engine))


# ---- 1. tables of ties against the model
@pytest.mark.parametrize("d", [8, 20, 96])   # the three lane-group forms: G = 2 | G = 8 (20 = 5 pieces: three lanes idle in the last) | G = 32
@pytest.mark.parametrize("n", [1, 65, 3000])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ties_tables_equal_the_model(metric, n, d):
    X, Q, d32 = gr.ties_table(metric, n, d, max(NQS), seed=metric)
    ix = index(X, metric)
    for name, keys in gr.layouts(n, seed=metric).items():
        ix.set_groups(keys)
        for k in KS:
            for m in MS:
                if k * m > 65536:
                    continue
                want = grr.numpy_group_rows(d32, keys, k, m)   # (queries are answered one by one: a smaller batch is a prefix)
                if name == "every row its own":
                    assert (want[3] <= 1).all() and (want[4] <= 1).all()
                if name == "one group" and n == 3000:   # one group across 12 chunks and a merge
                    assert (want[4][:, 0] == n).all() and (want[3][:, 0] == min(m, n)).all() and (want[5] == 1).all()
                for nq in NQS:
                    all_engines(ix, Q[:nq], k, m, tuple(a[:nq] for a in want), "%s n %d d %d nq %d k %d m %d" % (name, n, d, nq, k, m))
    ix.close()


# ---- 2. m = 1 is search_groups; m at or above the largest group returns every winning group whole
@pytest.fixture(scope="module")
def table4():
    n, d, nq = 3000, 20, 5
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


def test_m_of_one_equals_search_groups(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    for k in (1, 10, 130, 1024):
        for engine in ENGINES:
            g = ix.search_groups(Q, k, engine=engine)
            info = ix.groups_info()
            r = ix.search_group_rows(Q, k, 1, engine=engine)
            assert ix.groups_info() == info, (k, engine)   # what the equivalent search_groups call leaves
            gr.same((r[0][:, :, 0], r[1][:, :, 0], r[2], r[5]), g, "m = 1 k %d %s" % (k, engine))
            assert np.array_equal(r[3], (g[0] >= 0).astype(np.int32))


def test_m_at_or_above_the_largest_group_returns_the_groups_whole(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    largest = ix.groups_info()["largest_group"]
    assert largest == np.unique(keys, return_counts=True)[1].max()
    for m in (largest, largest + 3):
        got = ix.search_group_rows(Q, 20, m)
        grr.check_group_rows(got, d32, keys, 20, m, what="m %d" % m)
        assert np.array_equal(got[3], got[4]) and (got[3] > 0).all()
        for q in range(len(Q)):
            for s in range(20):
                rows = got[0][q, s, :got[3][q, s]]
                assert np.array_equal(np.sort(rows), np.flatnonzero(keys == got[2][q, s]))   # the whole group ...
                assert np.array_equal(gr.key_order(d32[rows, q], rows), np.arange(len(rows)))   # ... in key order


# ---- 3. chunk boundaries: the largest group just below, at and just above a multiple of the chunk
@pytest.mark.parametrize("size", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_groups_around_a_multiple_of_the_chunk(size):
    n, d, nq = size + 90, 8, 3
    X, Q, d32 = gr.ties_table(0, n, d, nq, seed=size)
    rng = np.random.default_rng(size)
    keys = np.concatenate([np.full(size, 77, np.int64), rng.integers(100, 130, 90)])[rng.permutation(n)]
    ix = index(X, 0, keys)
    assert ix.groups_info()["largest_group"] == size
    for k in (1, 5, 31):
        for m in (1, 2, 7, 64, size - 1, size, min(size + 1, 1024)):
            want = grr.numpy_group_rows(d32, keys, k, m)
            if m > CHUNK and k == 31:   # the big group's rows come from two chunks at least, whatever the order inside it
                assert (want[3][want[2] == 77] == min(m, size)).all() and (want[2] == 77).any(axis=1).all()
            all_engines(ix, Q, k, m, want, "size %d k %d m %d" % (size, k, m))
    ix.close()


# ---- 4. continuous tables: the device's own flat search with k = n, grouped in numpy
def grouped(ids, dist, keys, k, m):
    """the ordered walk over a flat search's full answer"""
    nq = len(ids)
    out = (np.full((nq, k, m), -1, np.int64), np.full((nq, k, m), np.inf, F), np.zeros((nq, k), np.int64), np.zeros((nq, k), np.int32),
           np.zeros((nq, k), np.int64), np.zeros(nq, np.int32))
    for q in range(nq):
        valid = ids[q] >= 0
        rows, dd = ids[q][valid], dist[q][valid]
        g = keys[rows]
        first = np.sort(np.unique(g, return_index=True)[1])[:k]   # first occurrence of every key, in answer order
        out[5][q] = len(first)
        for s, f in enumerate(first):
            mine = np.flatnonzero(g == g[f])
            c = min(m, len(mine))
            out[0][q, s, :c], out[1][q, s, :c] = rows[mine[:c]], dd[mine[:c]]
            out[2][q, s], out[3][q, s], out[4][q, s] = g[f], c, len(mine)
    return out


@pytest.mark.parametrize("name,metric", [("gaussian", 0), ("embedding-like", 1), ("gaussian x 3 queries", 2)])
def test_continuous_tables_equal_the_grouped_flat_search(name, metric):
    n, d, nq = 3000, 64, 5
    X, Q = er.make(name, n, d, nq, seed=5)
    ix = index(X, metric)
    full = ix.search(Q, n, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    assert (full[2] == n).all()
    for lname, keys in gr.layouts(n, seed=5).items():
        ix.set_groups(keys)
        for k, m in ((1, 1), (10, 3), (10, 300), (100, 7), (64, 1024)):
            all_engines(ix, Q, k, m, grouped(full[0], full[1], keys, k, m), "%s %s k %d m %d" % (name, lname, k, m))
    ix.close()


# ---- 5. visibility
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


def test_a_deleted_representative_and_a_group_entirely_invisible(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    free = grr.numpy_group_rows(d32, keys, 7, 3)
    hidden = np.zeros(len(X), bool)
    hidden[free[0][:, :3, 0].reshape(-1)] = True   # the first three representatives of every query: their groups' next rows take over
    hidden[keys == free[2][0, 4]] = True           # ... and one group of query 0's answer altogether
    ix.set_deleted(packbits(hidden))
    for k, m in ((7, 3), (64, 1), (130, 20)):
        want = grr.numpy_group_rows(d32, keys, k, m, visible=~hidden)
        assert not (want[2] == free[2][0, 4]).any()
        all_engines(ix, Q, k, m, want, "deleted k %d m %d" % (k, m))
    want = grr.numpy_group_rows(d32, keys, 375, 20, visible=~hidden)
    full = grr.numpy_group_rows(d32, keys, 375, 20)
    assert (want[4].sum(axis=1) == (~hidden).sum()).all() and (full[4].sum(axis=1) == len(X)).all()   # sizes count the visible rows, and only them
    reset(ix)


def test_int_column_program_with_distance_and_id_map(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(3)
    col = rng.integers(-100, 100, n).astype(np.int32)
    ix.set_int_filter(col, "<", 13)
    vis = sr.visible_rows(n, int_filter=(col, "<", 13))
    for k, m in ((7, 3), (130, 9)):
        all_engines(ix, Q, k, m, grr.numpy_group_rows(d32, keys, k, m, visible=vis), "int column k %d m %d" % (k, m))
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    t = float(np.sort(d32, axis=0)[400].min())   # an integer some row's distance EQUALS: `<=` keeps it
    assert (d32 == F(t)).any()
    prog = [("dist",), ("const", t), ("<=",), ("i32", 0), ("const", 13), ("<",), ("and",), ("f32", 4), ("const", 0.3), (">",), ("and",)]
    ix.set_filter_program(prog, rows)   # (it replaces the single comparison: the int column is now the program's own)
    both = np.stack([sr.visible_rows(n, program=prog, rows=rows, dist=d32[:, q].astype(np.float64)) for q in range(d32.shape[1])], axis=1)
    assert (both.sum(axis=0) > 10).all() and len(set(both.sum(axis=0).tolist())) > 1
    ix.set_id_map(3, 8)
    for k, m in ((7, 3), (64, 20), (375, 9)):
        want = grr.numpy_group_rows(d32, keys, k, m, visible=both)
        all_engines(ix, Q, k, m, grr.mapped(want, 3, 8), "program on an int column and @distance, id map, k %d m %d" % (k, m))
    assert len({tuple(np.sort(want[4][q])) for q in range(len(Q))}) > 1   # the sizes differ per query
    assert (want[1][np.isfinite(want[1])] <= F(t)).all()
    reset(ix)


def test_nan_rows_sort_last_inside_a_group_and_a_group_of_nans_counts():
    n, d, nq = 300, 8, 3
    X, Q, d32 = gr.ties_table(0, n, d, nq, seed=8)
    X = X.copy()
    keys = (np.arange(n, dtype=np.int64) // 6) * 5
    X[[0, 1, 2, 3, 4, 5, 17, 40], 0] = np.nan   # group 0 entirely NaN, rows of two other groups
    d32 = d32.copy()
    d32[[0, 1, 2, 3, 4, 5, 17, 40]] = np.nan
    ix = index(X, 0, keys)
    for k, m in ((7, 6), (50, 4), (64, 7)):
        all_engines(ix, Q, k, m, grr.numpy_group_rows(d32, keys, k, m), "NaN rows k %d m %d" % (k, m))
    want = grr.numpy_group_rows(d32, keys, 64, 7)
    assert (want[5] == 50).all() and (want[2][:, 49] == 0).all() and np.isnan(want[1][:, 49, :6]).all() and (want[3][:, 49] == 6).all()
    s17 = np.argwhere(want[2][0] == 10)[0, 0]   # row 17's group: its NaN row is the group's last
    assert want[0][0, s17, 5] == 17 and np.isnan(want[1][0, s17, 5]) and np.isfinite(want[1][0, s17, :5]).all()
    ix.close()


def test_duplicate_rows_inside_and_across_groups():
    n, d = 512, 8
    X = np.zeros((n, d), F)
    X[:, 0] = np.arange(n) % 4   # four distances, 128 identical rows each
    Q = np.zeros((2, d), F)
    Q[1, 0] = 3
    keys = np.random.default_rng(2).integers(0, 40, n).astype(np.int64) - 20
    d32 = gr.assert_ties_table(X, Q, 0)
    ix = index(X, 0, keys)
    for k, m in ((1, 1), (7, 2), (40, 5), (64, 30)):
        all_engines(ix, Q, k, m, grr.numpy_group_rows(d32, keys, k, m), "ties k %d m %d" % (k, m))
    ix.close()


# ---- 6. buffers and stream order
def test_device_and_host_buffers(table4):
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq, k, m = len(Q), 10, 4
    want = grr.numpy_group_rows(d32, keys, k, m)
    for engine in ENGINES:
        got = ix.search_group_rows(Q, k, m, engine=engine)
        assert all(isinstance(a, np.ndarray) for a in got)
        dq = torch.from_numpy(Q).cuda()
        torch.cuda.synchronize()
        out = ix.search_group_rows(dq, k, m, engine=engine)
        assert all(hasattr(t, "data_ptr") for t in out)
        ix.synchronize()
        grr.same([t.cpu().numpy() for t in out], want, "device %s" % engine)
    shapes = (((nq, k, m), np.int64), ((nq, k, m), F), ((nq, k), np.int64), ((nq, k), np.int32), ((nq, k), np.int64), ((nq,), np.int32))
    mine = tuple(np.full(s, -7, t) for s, t in shapes)
    out = ix.search_group_rows(Q, k, m, out=mine)
    assert out[0] is mine[0]
    grr.same(out, want, "out= host")
    dmine = tuple(torch.full(s, -7, dtype=getattr(torch, np.dtype(t).name), device="cuda") for s, t in shapes)
    torch.cuda.synchronize()
    out = ix.search_group_rows(Q, k, m, out=dmine)   # host queries, device results
    ix.synchronize()
    grr.same([t.cpu().numpy() for t in out], want, "host in, device out")
    p = lambda a: a.ctypes.data   # noqa: E731
    mine = tuple(np.full(s, -7, t) for s, t in shapes)
    assert ix.L.eps_index_search_group_rows(ix.h, p(Q), nq, k, m, None, 0, 0, 0, p(mine[0]), p(mine[1]), p(mine[2]), p(mine[3]), None, None) == 0   # sizes, counts, p: NULL
    grr.same(mine[:4] + want[4:], want, "no sizes, no counts")
    assert (mine[4] == -7).all() and (mine[5] == -7).all()


def test_statistics_report_the_call_like_a_search(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    hidden = np.zeros(len(X), bool)
    hidden[::3] = True
    ix.set_deleted(packbits(hidden))
    got = ix.search_group_rows(Q, 10, 4, engine="scan")
    st = ix.stats()
    whole = sum(int((keys == g).sum()) for g in got[2].reshape(-1))   # the second phase walks every row of a winning group, visible or not
    assert st["dist_evals"] == len(Q) * len(X) + whole, (st["dist_evals"], len(Q) * len(X), whole)
    assert st["main_kernel_ms"] > 0 and st["main_kernel_launches"] == 1 and st["main_kernel_bits"] == 32 and st["kernel_ms"] >= st["main_kernel_ms"], st
    reset(ix)


def test_host_queries_are_consumed_when_the_call_returns(table4):
    """device outputs, the scan engine (no host sync in either phase), a gate in front; straight after the call returns the page-locked query array
    is overwritten with the decoy from the host: a copy still pending then would take the decoy"""
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq, k, m = len(Q), 10, 4
    decoy = er.make(gr.TIES[0], len(X), X.shape[1], nq, seed=404)[1]
    want, want_decoy = grr.numpy_group_rows(d32, keys, k, m), grr.numpy_group_rows(gr.assert_ties_table(X, decoy, 0), keys, k, m)
    sg.differ_first(want[0][:, 0], want_decoy[0][:, 0], "search_group_rows host queries")
    shapes = (((nq, k, m), torch.int64), ((nq, k, m), torch.float32), ((nq, k), torch.int64), ((nq, k), torch.int32), ((nq, k), torch.int64), ((nq,), torch.int32))
    make_outs = lambda: tuple(torch.full(s, sg.FILL, dtype=t, device="cuda") for s, t in shapes)   # noqa: E731
    s = torch.cuda.Stream()
    sg.calibrate()
    ix.search_group_rows(Q, k, m)   # (the rows by group are built: a set-up step, with its sync)
    ix.set_stream(s.cuda_stream)
    try:
        host = sg.pinned(Q.shape, Q.dtype)

        def issue(outs=None):
            host[...] = Q
            ix.search_group_rows(host, k, m, engine="scan", out=outs or make_outs())
            host[...] = decoy
        ms = sg.gate_for("search_group_rows, page-locked host queries", issue, s)
        outs = make_outs()
        torch.cuda.synchronize()
        sg.gate(s, ms)
        issue(outs)
        s.synchronize()
        grr.same([t.cpu().numpy() for t in outs], want, "the host array was read after the call returned")
    finally:
        ix.set_stream(None)


def test_device_outputs_on_a_callers_stream_keep_their_place(table4):
    """the queries are valid only at the call's place in the stream: the decoy before the gate, the real ones behind it, the decoy again after the
    call.  With the scan engine neither phase waits for the device, so the call returns while the gate is still running"""
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq, k, m = len(Q), 10, 4
    decoy = er.make(gr.TIES[0], len(X), X.shape[1], nq, seed=404)[1]
    want, want_decoy = grr.numpy_group_rows(d32, keys, k, m), grr.numpy_group_rows(gr.assert_ties_table(X, decoy, 0), keys, k, m)
    sg.differ_first(want[0][:, 0], want_decoy[0][:, 0], "search_group_rows device queries")
    shapes = (((nq, k, m), torch.int64), ((nq, k, m), torch.float32), ((nq, k), torch.int64), ((nq, k), torch.int32), ((nq, k), torch.int64), ((nq,), torch.int32))
    make_outs = lambda: tuple(torch.full(s, sg.FILL, dtype=t, device="cuda") for s, t in shapes)   # noqa: E731
    s = torch.cuda.Stream()
    sg.calibrate()
    ix.search_group_rows(Q, k, m)   # (the rows by group are built)
    ix.set_stream(s.cuda_stream)
    try:
        dq, real, dec = (torch.from_numpy(a).cuda() for a in (decoy, Q, decoy))
        torch.cuda.synchronize()
        ms = sg.gate_for("search_group_rows, device queries", lambda: ix.search_group_rows(dq, k, m, engine="scan", out=make_outs()), s)
        outs = make_outs()
        torch.cuda.synchronize()
        with sg.window(s, dq, real, dec, ms) as w:
            ix.search_group_rows(dq, k, m, engine="scan", out=outs)
            w.returned(*outs)
        s.synchronize()
        assert w.behind, "the call returned only after the gate (%.1f ms) had run: it waited for the device" % ms
        grr.same(w.numpy(), want, "the call read its queries outside its place in the stream")
    finally:
        ix.set_stream(None)


# ---- 7. no trace
def test_search_group_rows_leaves_no_trace(table4):
    ix, X, Q, d32, keys = table4
    reset(ix)
    cand = np.arange(0, len(X), 3, dtype=np.int64)
    calls = (lambda: ix.search(Q, 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM), lambda: ix.search(Q, 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_AUTO),
             lambda: ix.search_groups(Q, 10), lambda: ix.search_groups(Q, 130, engine="scan"), lambda: ix.search_among(Q, cand, 10))
    before = [c() for c in calls]
    for engine in ENGINES:
        ix.search_group_rows(Q, 10, 4, engine=engine)
        ix.search_group_rows(Q, 130, 300, engine=engine)
    for b, c in zip(before, calls):
        for x, y in zip(b, c()):
            assert np.array_equal(x, y, equal_nan=True)
    # new keys: the rows by group follow them
    keys2 = gr.layouts(len(X), seed=9)["zipf"]
    ix.set_groups(keys2)
    for k, m in ((10, 4), (7, 300)):
        all_engines(ix, Q, k, m, grr.numpy_group_rows(d32, keys2, k, m), "new keys k %d m %d" % (k, m))
    ix.set_groups(keys)
    grr.check_group_rows(ix.search_group_rows(Q, 10, 4), d32, keys, 10, 4, what="the first keys again")


# ---- 8. refusals: each gives its error code and leaves the handle usable
def test_refusals(table4):
    import torch
    ix, X, Q, d32, keys = table4
    reset(ix)
    nq = len(Q)
    want = grr.numpy_group_rows(d32, keys, 10, 4)
    groups = ix.search_groups(Q, 10)

    def usable():
        grr.same(ix.search_group_rows(Q, 10, 4), want, "after a refusal")
        gr.same(ix.search_groups(Q, 10), groups, "search_groups after a refusal")

    for k, m, text in ((10, 0, "m must be"), (10, 1025, "m must be"), (10, -1, "m must be"), (1, 65537, "m must be"), (65537, 1, "k must be"), (0, 4, "k must be"),
                       (1024, 65, "k * m"), (257, 256, "k * m")):
        with pytest.raises(EpsillaError) as e:
            ix.search_group_rows(Q, k, m)
        assert e.value.code == 30000 and text in str(e.value), (k, m, str(e.value))
    usable()
    assert ix.search_group_rows(Q, 1024, 64)[0].shape == (nq, 1024, 64)   # k * m = 65536 is served
    for kw, text in ((dict(page_rows=1025), "page_rows"), (dict(scratch_bytes=-1), "scratch_bytes"), (dict(engine=3), "engine")):
        with pytest.raises((EpsillaError, KeyError)) as e:
            ix.search_group_rows(Q, 10, 4, **kw)
        assert isinstance(e.value, KeyError) or (e.value.code == 30000 and text in str(e.value)), kw
    p = lambda a: a.ctypes.data   # noqa: E731
    h = [np.empty((nq, 10, 4), np.int64), np.empty((nq, 10, 4), F), np.empty((nq, 10), np.int64), np.empty((nq, 10), np.int32), np.empty((nq, 10), np.int64),
         np.empty(nq, np.int32)]
    dev = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):   # the wrapper refuses a mixed set, and so does the library
        ix.search_group_rows(Q, 10, 4, out=(h[0], h[1], h[2], h[3], dev, h[5]))
    call = lambda q, *o, engine=0: ix.L.eps_index_search_group_rows(ix.h, q, nq, 10, 4, None, engine, 0, 0, *o)   # noqa: E731
    assert call(p(Q), p(h[0]), p(h[1]), p(h[2]), p(h[3]), dev.data_ptr(), p(h[5])) == 30000 and "host or all be device" in ix.L.eps_index_last_error(ix.h).decode()
    assert call(p(Q), p(h[0]), p(h[1]), dev.data_ptr(), p(h[3]), p(h[4]), p(h[5])) == 30000
    assert call(p(Q), p(h[0]), p(h[1]), p(h[2]), p(h[3]), p(h[4]), p(h[5]), engine=3) == 30000
    assert call(None, p(h[0]), p(h[1]), p(h[2]), p(h[3]), p(h[4]), p(h[5])) == 30000 and "null buffer" in ix.L.eps_index_last_error(ix.h).decode()   # null queries
    assert call(p(Q), p(h[0]), p(h[1]), p(h[2]), None, p(h[4]), p(h[5])) == 30000          # null row counts
    assert call(p(Q), None, p(h[1]), p(h[2]), p(h[3]), p(h[4]), p(h[5])) == 30000          # null ids
    assert ix.L.eps_index_search_group_rows(ix.h, None, 0, 10, 4, None, 0, 0, 0, None, None, None, None, None, None) == 0   # nq = 0
    usable()
    ix.set_groups(None)   # no groups set
    with pytest.raises(EpsillaError) as e:
        ix.search_group_rows(Q, 10, 4)
    assert e.value.code == 30000 and "no groups" in str(e.value)
    ix.set_groups(keys)
    usable()
    # stale labels after an append, and after a new table
    ix2 = index(X[:100], 0, keys[:100])
    assert (ix2.search_group_rows(Q, 3, 2)[5] == 3).all()
    ix2.append_rows(np.zeros((8, X.shape[1]), F))
    for _ in range(2):
        with pytest.raises(EpsillaError) as e:
            ix2.search_group_rows(Q, 3, 2)
        assert e.value.code == 30000 and "set_groups" in str(e.value)
    keys108 = np.concatenate([keys[:100], keys[:8]])
    ix2.set_groups(keys108)
    X108 = np.concatenate([X[:100], np.zeros((8, X.shape[1]), F)])
    grr.check_group_rows(ix2.search_group_rows(Q, 3, 2), gr.assert_ties_table(X108, Q, 0), keys108, 3, 2, what="after the append and new keys")
    ix2.attach_rows(X[:108])
    with pytest.raises(EpsillaError) as e:
        ix2.search_group_rows(Q, 3, 2)
    assert e.value.code == 30000 and "set_groups" in str(e.value)
    ix2.close()
    # a sharded handle
    sh = amd.GpuIndex(X.shape[1], "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(np.zeros((300, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        sh.search_group_rows(Q, 10, 4)
    assert e.value.code == 50002 and "shard" in str(e.value)
    sh.search(Q, 3, mode=amd.MODE_FLAT)
    sh.close()
    # an index without rows: no group has a row
    empty = amd.GpuIndex(X.shape[1], "EUCLIDEAN", device=0)
    empty.set_groups(np.zeros(0, np.int64))
    got = empty.search_group_rows(Q, 4, 3)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and all((got[i] == 0).all() for i in (2, 3, 4, 5))
    empty.close()
