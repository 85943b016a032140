"""GpuIndex.search_filters / eps_index_search_filters on the MI355X (csrc/filters.hip): n = 3001 rows (no multiple of 64 or 1024, three verdict
workgroups).  Integer tables (every fp32 distance exact in any order, full of ties) are held to numpy's answer exactly: ids, distance bits, counts,
visible.  Continuous tables: tests/filters_ref.py under exact_ref's tree bound, and the bits of set_filter_program + search(FLAT_STREAM)."""
import numpy as np
import pytest

import exact_ref as er
import filters_ref as fr
import range_ref as rr
import select_ref as sr
import vectordb_amd as amd
from helpers import bitset
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
INT_TABLE = {0: "integers -8..8", 1: "integers / 16", 2: "integers -8..8"}
N, CH = 3001, fr.FILTERS_CHUNK
ENGINES = ("lists", "planes", "auto")
FLAT = dict(mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
DT, OFF = sr.row_layout([("flag", "bool"), ("tenant", "i32"), ("score", "f64")])   # the reference's packing: the double at byte 5
ROWS = np.zeros(N, DT)
# tenant 1: one row, 2: exactly one gather chunk, 3: one chunk + 1, 4: the rest (several chunks); in no row order
ROWS["tenant"] = np.random.default_rng(1).permutation(np.repeat([1, 2, 3, 4], [1, CH, CH + 1, N - 2 * CH - 2])).astype(np.int32)
ROWS["score"] = np.random.default_rng(2).random(N)


def tenant(c):
    return [("i32", OFF["tenant"]), ("const", c), ("=",)]


# 0: empty, 1: no row, 6: the text of 3 once more, 7: a range on the f64 column, 8: no query
PROGRAMS = [[], [("const", 0)], tenant(1), tenant(2), tenant(3), tenant(4), tenant(2),
            [("f64", OFF["score"]), ("const", 0.25), (">=",), ("f64", OFF["score"]), ("const", 0.75), ("<",), ("and",)], tenant(9)]
QUERY_PROG = np.array([5, 0, 4, 5, 1, 7, 5, 2, 4, 5, 3, 4, 5, 6, 4], np.int32)   # programs with 5, 4 and 1 queries, scattered through the batch
NQ = len(QUERY_PROG)


def same(got, want, what=""):
    for x, y, name in zip(got, want, ("ids", "dist", "counts", "visible")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "dist":
            x, y = (x + F(0)).view(np.uint32), (y + F(0)).view(np.uint32)
        bad = np.argwhere(x != y)
        assert x.shape == y.shape and len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def index(X, metric):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    ix.attach_rows(X)
    return ix


@pytest.fixture(scope="module")
def masks():
    m = fr.program_masks(N, PROGRAMS, ROWS)
    assert m.sum(0).tolist()[:7] == [N, 0, 1, CH, CH + 1, N - 2 * CH - 2, CH] and N - 2 * CH - 2 > 3 * CH
    assert sorted(np.bincount(QUERY_PROG, minlength=9).tolist()) == [0, 1, 1, 1, 1, 1, 1, 4, 5]
    return m


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("d", [7, 64])   # the scalar and the 16-byte form
def test_integer_tables_equal_numpy(masks, d, metric, engine):
    X, Q = er.make(INT_TABLE[metric], N, d, NQ, seed=metric)
    d32 = rr.dist32(X, Q, metric)
    assert np.array_equal(d32.astype(np.float64), er.dist64(X, Q, metric))
    ix = index(X, metric)
    for k in (1, 10, 100):
        want = fr.numpy_filters(d32, masks, QUERY_PROG, k)
        assert want[2].tolist() == np.minimum(k, want[3]).tolist() and {0, 1, CH, CH + 1}.issubset(want[3].tolist())   # k above the visible count too
        same(ix.search_filters(Q, k, PROGRAMS, QUERY_PROG, ROWS, engine=engine), want, "%s k %d" % (engine, k))
        engines, visible = ix.filters_info()
        assert visible.tolist() == masks.sum(0).tolist() and engines[8] == 0 and engines[3] == engines[6]
        assert engine == "auto" or set(engines[:8].tolist()) == {amd.index.FILTERS_ENGINES[engine]}
        st = ix.stats()
        assert engine != "lists" or (st["main_kernel_bits"] == 32 and st["main_kernel_queries"] == NQ and st["dist_evals"] == int(want[3].sum())), st
    ix.close()


@pytest.mark.parametrize("P", [1, 3, 64])   # a tenant per program; 64: 41 instructions each, two verdict passes; k = 130: one query per workgroup
def test_program_counts(P):
    X, Q = er.make(INT_TABLE[0], N, 64, 70, seed=3)
    d32 = rr.dist32(X, Q, 0)
    rows = np.zeros(N, DT)
    rows["tenant"] = np.random.default_rng(P).integers(0, P, N)
    progs = [tenant(c) + [("const", 1), ("and",)] * (19 if P == 64 else 0) for c in range(P)]
    qp = np.random.default_rng(P + 1).integers(0, P, 70).astype(np.int32)
    m = fr.program_masks(N, progs, rows)
    ix = index(X, 0)
    for k, engine in ((10, "lists"), (10, "auto"), (130, "lists"), (10, "planes")):
        same(ix.search_filters(Q, k, progs, qp, rows, engine=engine), fr.numpy_filters(d32, m, qp, k), "P %d k %d %s" % (P, k, engine))
    ix.close()


@pytest.mark.parametrize("name,metric", [("gaussian", 0), ("embedding-like", 1), ("uniform", 2)])
def test_continuous_tables(masks, name, metric):
    X, Q = er.make(name, N, 64, NQ, seed=7)
    ref = er.Ref(X, Q, metric)
    ix = index(X, metric)
    got = {e: ix.search_filters(Q, 10, PROGRAMS, QUERY_PROG, ROWS, engine=e) for e in ENGINES}
    for e in ENGINES:
        fr.check_filters(*got[e], ref, masks, QUERY_PROG, 10, what="%s %s" % (name, e))
        same(got[e], got["lists"], "%s against lists" % e)
    for q in range(NQ):
        ix.set_filter_program(PROGRAMS[QUERY_PROG[q]], ROWS)
        same([a[q:q + 1] for a in got["lists"][:3]], ix.search(Q[q], 10, **FLAT), "query %d against set_filter_program + search" % q)
    ix.close()


def test_standing_state_and_device_outputs(masks):
    import torch
    X, Q = er.make(INT_TABLE[0], N, 64, NQ, seed=5)
    d32 = rr.dist32(X, Q, 0)
    gone = bitset(N, np.random.default_rng(4).choice(N, 700, replace=False).tolist())
    col = np.random.default_rng(5).integers(0, 10, N).astype(np.int32)
    prog = [("f64", OFF["score"]), ("const", 0.5), ("<",)]
    ix = index(X, 0)
    ix.set_id_map(3, 5)
    ix.set_deleted(gone)
    dQ, dR = torch.from_numpy(Q).cuda(), torch.from_numpy(ROWS.view(np.uint8).reshape(N, -1)).cuda()
    for install, state in ((lambda: ix.set_int_filter(col, "<", 7), dict(int_filter=(col, "<", 7))), (lambda: ix.set_filter_program(prog, ROWS), dict(program=prog, rows=ROWS))):
        install()
        before = ix.search(Q, 10, **FLAT)
        ids, dist, counts, visible = fr.numpy_filters(d32, masks & sr.visible_rows(N, deleted=gone, **state)[:, None], QUERY_PROG, 10)
        want = (np.where(ids >= 0, ids * 5 + 3, -1), dist, counts, visible)
        for engine in ENGINES:
            same(ix.search_filters(Q, 10, PROGRAMS, QUERY_PROG, ROWS, engine=engine), want, "host %s" % engine)
            out = ix.search_filters(dQ, 10, PROGRAMS, QUERY_PROG, dR, stride=DT.itemsize, engine=engine)
            ix.synchronize()
            same([o.cpu().numpy() for o in out], want, "device %s" % engine)
            same(ix.search(Q, 10, **FLAT), before, "a plain search after %s" % engine)
    ix.close()


def test_refusals_leave_a_plain_search_unchanged():
    X, Q = er.make(INT_TABLE[0], N, 7, 3, seed=6)
    ix = index(X, 0)
    before = ix.search(Q, 10, **FLAT)
    USER, UNSUPPORTED = 30000, 50002
    ok = dict(k=10, programs=[tenant(2), []], query_prog=[0, 1, 0], rows=ROWS)

    def refused(ix, code, **change):
        with pytest.raises(EpsillaError) as e:
            ix.search_filters(Q, **dict(ok, **change))
        assert e.value.code == code, (change, e.value)
    for change, code in [(dict(query_prog=[0, 2, 0]), USER), (dict(query_prog=[0, -1, 0]), USER), (dict(programs=[[("dist",), ("const", 1.0), ("<",)], []]), USER),
                         (dict(programs=[[("const", 1), ("and",)], []]), USER), (dict(programs=[[("i32", DT.itemsize - 3)], []]), USER),
                         (dict(rows=ROWS[:N - 1]), USER), (dict(k=0), USER), (dict(k=1025), USER),
                         (dict(programs=[[("const", 1)] + [("not",)] * 64, []]), UNSUPPORTED)]:
        refused(ix, code, **change)
        same(ix.search(Q, 10, **FLAT), before, "after %s" % (change,))
    ptr = amd.index._ptr   # a malformed prog_offsets and an unknown engine cannot be written through the wrapper: the C entry itself
    qp, out = np.zeros(3, np.int32), (np.empty((3, 10), np.int64), np.empty((3, 10), F))
    for off, engine in (([0, 2, 1], 0), ([0, 3, 3], 3)):
        off = np.array(off, np.int32)
        assert ix.L.eps_index_search_filters(ix.h, ptr(Q), 3, 10, None, amd.index._filter_ops(tenant(2)), ptr(off), 2, ptr(qp), ptr(ROWS), DT.itemsize, N, 0, engine,
                                             ptr(out[0]), ptr(out[1]), None, None) == USER
        same(ix.search(Q, 10, **FLAT), before, "after offsets %s engine %d" % (off, engine))
    assert ix.search_filters(Q[:0], **dict(ok, query_prog=[]))[0].shape == (0, 10)   # nq = 0: EPS_OK
    ix.set_filter_program([("dist",), ("const", 1e9), ("<",)], ROWS)   # an installed program that reads @distance
    before = ix.search(Q, 10, **FLAT)
    refused(ix, USER)
    same(ix.search(Q, 10, **FLAT), before, "after the installed @distance program")
    ix.set_filter_program(None)
    ix.append_rows(X[:2])   # the attribute rows are two short now
    before = ix.search(Q, 10, **FLAT)
    refused(ix, USER)
    same(ix.search(Q, 10, **FLAT), before, "after stale rows")
    ix.close()
    sh = amd.GpuIndex(7, "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(X)
    before = sh.search(Q, 10, **FLAT)
    refused(sh, UNSUPPORTED)
    same(sh.search(Q, 10, **FLAT), before, "after the sharded refusal")
    sh.close()
