"""The filter-program evaluator of the device (eval_filter_program / row_visible, csrc/device_common.hpp) held to the numpy evaluator of
tests/select_ref.py (checked on hand-written rows in tests/test_select_cpu.py), opcode by opcode and judging site by judging site.

 (a) GpuIndex.select(0, None) returns the verdict of EVERY row: one program per opcode and a dozen composites over attribute rows in the
     reference's packed layout - {BOOL, DOUBLE, TINYINT, BIGINT, SMALLINT, FLOAT}: the double at byte 1, the int64 at byte 10 - and over the same
     fields naturally aligned.  The first rows hold the edge values (NaN, +-inf, a zero divisor, -0.0, an fp32 denormal, int64 beyond 2^53,
     type minima, bool bytes 0 / 1 / 2 / 255).
 (b) the same verdicts where a SEARCH judges: stream scan, matrix engines, one-pass form (mask launch), graph traversal's result walk, pre-filter
     call, two shards - on a table of small integers, whose fp32 distances are the fp64 ones bit for bit, so that `@distance > c` at an exact
     distance value has no boundary band.
 (c) what Index::set_filter_program_pitched refuses; the evaluator drops a push at depth 16 silently, which is right only while such a program
     cannot be installed.
 (d) the k-way merge of shard lists orders NaN distances as the shards' own keys do.

Nothing here is a tolerance: verdicts and exact-table answers are compared for equality."""
import ctypes as C
import os

import numpy as np
import pytest

import exact_ref as xr
import select_ref as sr
import vectordb_amd as amd
from helpers import bitset, data
from test_select_cpu import ACCEPTS, DENORM, FIELDS, REJECTS, STRIDE
from vectordb_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
DIM = 4
N = 2 * sr.SEL_ROWS + 77
NAN, INF = float("nan"), float("inf")

LAYOUTS = {"packed": sr.row_layout(FIELDS), "aligned": sr.row_layout(FIELDS, align=True)}
assert LAYOUTS["packed"][0].itemsize == STRIDE and LAYOUTS["packed"][1] == dict(b=0, w=1, t=9, big=10, s=18, x=20)

# one edge value per row; every other field of the row keeps an ordinary value
EDGES = ([dict(w=v) for v in (NAN, -NAN, INF, -INF, 0.0, -0.0, 5e-324, 1.7976931348623157e308, 0.25, 7.5)]
         + [dict(x=v) for v in (NAN, INF, -INF, 0.0, -0.0, DENORM, -DENORM, 3.4028234663852886e38, 0.25, 1.1754943508222875e-38)]
         + [dict(big=v) for v in (2 ** 53 + 1, 2 ** 53, 2 ** 53 - 1, -(2 ** 53) - 1, 2 ** 53 + 3, -2 ** 63, 2 ** 63 - 1, 2 ** 40 + 1, 0, -1)]
         + [dict(t=v) for v in (-128, 127, 0, -7, 7, -3, -1)] + [dict(s=v) for v in (-32768, 32767, 0, -3, 1000)]
         + [dict(b=v) for v in (0, 1, 2, 255, 128)]
         + [dict(w=0.0, t=0), dict(w=0.0, t=-1), dict(w=-0.0, t=1), dict(t=7, s=-3), dict(t=-7, s=3), dict(w=NAN, x=NAN), dict(w=INF, x=INF)])


def make_rows(n, seed, edges=True):
    """field values of n rows: the edges first, the rest drawn so that every comparison of the matrix parts the rows"""
    rng = np.random.default_rng(seed)
    v = dict(b=rng.integers(0, 3, n).astype(np.uint8), w=rng.standard_normal(n), t=rng.integers(-128, 128, n).astype(np.int8),
             s=rng.integers(-32768, 32768, n).astype(np.int16), x=rng.standard_normal(n).astype(F))
    # int64: a third within +-2^16 of 2^40 (a conversion through fp32 moves them across 2^40), a third beyond 2^53, a third small
    kind = rng.integers(0, 3, n)
    v["big"] = np.where(kind == 0, 2 ** 40 + rng.integers(-2 ** 16, 2 ** 16, n),
                        np.where(kind == 1, rng.integers(-2 ** 62, 2 ** 62, n), rng.integers(-1000, 1000, n))).astype(np.int64)
    if edges:
        for i, e in enumerate(EDGES):
            for name, val in e.items():
                v[name][i] = np.array(val).astype(v[name].dtype) if name != "b" else val
    return v


def pack(values, layout):
    dt = LAYOUTS[layout][0]
    rows = np.zeros(len(values["b"]), dt)
    for name, _ in FIELDS:
        rows[name] = values[name]
    return rows


def prog_for(layout, program):
    """a program written over field NAMES -> over the layout's byte offsets"""
    off = LAYOUTS[layout][1]
    return [(ins[0], off[ins[1]]) if len(ins) > 1 and isinstance(ins[1], str) else ins for ins in program]


B_, W_, T_, BIG_, S_, X_ = ("bool", "b"), ("f64", "w"), ("i8", "t"), ("i64", "big"), ("i16", "s"), ("f32", "x")


def c(v):
    return ("const", v)


# the opcode whose name a case carries decides its verdict; (PUSH_I32 is not a field of this layout: tests/test_gpu_select.py loads one in every program)
MATRIX = {
    "const": [c(0.25), X_, (">",)],
    "dist": [("dist",), X_, ("+",), c(0.25), ("<",)],            # a select reads @distance as 0
    "i8": [T_, c(-3), ("<=",)],
    "i16": [S_, c(1000), (">",)],
    "i64": [BIG_, c(2 ** 40), ("<",)],
    "f32": [X_, c(0.25), ("<",)],
    "f64": [W_, c(0.25), (">",)],
    "bool": [B_],
    "+": [T_, S_, ("+",), c(0), (">",)],
    "-": [W_, X_, ("-",), c(0), (">",)],
    "*": [T_, X_, ("*",), c(0), (">",)],
    "/": [W_, T_, ("/",), c(0.01), (">",)],
    "%": [BIG_, c(7), ("%",), c(2), (">=",)],
    "<": [T_, c(10), ("<",)],
    "<=": [T_, c(10), ("<=",)],
    "=": [T_, c(4), ("%",), c(0), ("=",)],
    "<>": [T_, c(4), ("%",), c(0), ("<>",)],
    ">=": [T_, c(10), (">=",)],
    ">": [T_, c(10), (">",)],
    "and": [B_, X_, c(0), (">",), ("and",)],
    "or": [X_, c(0.8), (">",), W_, c(0.8), (">",), ("or",)],
    "not": [B_, ("not",)],
    "=b": [B_, S_, c(0), (">",), ("=b",)],
    "<>b": [B_, S_, c(0), (">",), ("<>b",)],
}
# P1 of part (b): attributes only - the misaligned double, the int64 and MOD
P1 = [W_, c(-0.25), (">",), BIG_, c(7), ("%",), c(3), ("<",), ("and",), T_, c(100), (">",), ("or",)]
FIELD_LOADS = [B_, W_, T_, BIG_, S_, X_]
COMPOSITES = {
    # 16 values on the stack (every field, ten more loads), 15 additions, one comparison
    "depth 16": FIELD_LOADS + [T_, S_, X_, W_, T_, S_, X_, W_, T_, c(0.5)] + [("+",)] * 15 + [c(2 ** 40), ("<",)],
    # 64 instructions: ((t + s) * x > 0) xor-ed eleven times with b, then AND-ed with big % 3 <> 0 ...
    "64 instructions": [T_, S_, ("+",), X_, ("*",), c(0), (">",)] + [B_, ("<>b",)] * 11 + [W_, c(0), ("<",), ("=b",)] * 6
                       + [BIG_, c(3), ("%",), c(0), ("<>",), ("or",), S_, c(-20000), (">",), ("and",), ("not",)],
    "=b over comparisons": [W_, c(0), (">",), X_, c(0), (">",), ("=b",)],
    "<>b of a bool and a comparison": [B_, T_, c(0), ("<",), ("<>b",)],
    "=b of two numbers": [T_, S_, ("=b",), B_, ("and",)],
    "not of a number": [T_, c(3), ("%",), ("not",)],
    "not of a product": [X_, T_, ("*",), ("not",), B_, ("or",)],
    "chained / and %": [BIG_, T_, ("/",), c(7), ("%",), c(1.5), (">",)],
    "% of doubles": [W_, c(0.5), ("%",), X_, c(0.25), ("%",), (">",)],
    "/ by a field that may be 0": [S_, T_, ("/",), W_, ("<",)],
    "NaN and inf through arithmetic": [W_, X_, ("*",), W_, X_, ("*",), ("-",), c(0), ("=",), B_, ("and",)],
    "mixed widths": [T_, S_, ("*",), BIG_, c(1e-9), ("*",), ("-",), X_, ("<",), W_, c(1), ("<",), ("or",), B_, ("and",)],
    "P1": P1,
}
assert len(COMPOSITES["64 instructions"]) == 64 and set(MATRIX) == set(_lib.FOP) - {"i32"}
PROGRAMS = [("op " + k, v) for k, v in MATRIX.items()] + [(k, v) for k, v in COMPOSITES.items()]


def index(n, seed=1, dim=DIM):
    ix = amd.GpuIndex(dim, "EUCLIDEAN", device=0)
    ix.attach_rows(np.random.default_rng(seed).random((n, dim), dtype=F))
    return ix


def verdicts(ix, n):
    ids, total = ix.select(0, None)
    assert total == len(ids)
    v = np.zeros(n, bool)
    v[ids] = True
    assert v.sum() == len(ids)
    return ids, v


# ---- (a) the opcode matrix.  The aligned control is the first thing this module asks of the device, one misaligned double on 65 rows the second
@pytest.fixture(scope="module")
def table():
    values = make_rows(N, 21)
    rows = {name: pack(values, name) for name in LAYOUTS}
    ix = index(N)
    yield ix, rows
    ix.close()


def test_aligned_control_comes_first(table):
    ix, rows = table
    prog = prog_for("aligned", [W_, c(0.25), (">",)])
    vis = sr.visible_rows(N, program=prog, rows=rows["aligned"])
    ix.set_filter_program(prog, rows["aligned"])
    ids, _ = verdicts(ix, N)
    assert np.array_equal(ids, np.flatnonzero(vis))


def test_one_misaligned_double_on_65_rows():
    """{BOOL, DOUBLE}: the double at byte 1 of a 9-byte row - what the drop-in hands over for any such schema"""
    dt, off = sr.row_layout([("b", "bool"), ("w", "f64")])
    assert off["w"] == 1 and dt.itemsize == 9
    rows = np.zeros(65, dt)
    rows["w"] = np.random.default_rng(5).standard_normal(65)
    rows["w"][:4] = [NAN, 0.25, -0.0, INF]
    prog = [("f64", 1), c(0.25), (">",)]
    vis = sr.visible_rows(65, program=prog, rows=rows)
    assert 0.2 * 65 < vis.sum() < 0.8 * 65
    ix = index(65)
    ix.set_filter_program(prog, rows)
    ids, _ = verdicts(ix, 65)
    assert np.array_equal(ids, np.flatnonzero(vis)), (ids[:8], np.flatnonzero(vis)[:8])
    ix.close()


@pytest.mark.parametrize("name,program", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_opcode_matrix(table, name, program):
    ix, rows = table
    got = {}
    for layout in ("aligned", "packed"):
        prog = prog_for(layout, program)
        vis = sr.visible_rows(N, program=prog, rows=rows[layout])
        share = vis[len(EDGES):].mean()
        assert 0.2 <= share <= 0.8, "%s: %.1f %% of the random rows pass: change the rows, not the bounds" % (name, 100 * share)
        ix.set_filter_program(prog, rows[layout])
        ids, got[layout] = verdicts(ix, N)
        bad = np.flatnonzero(got[layout] != vis)
        assert np.array_equal(ids, np.flatnonzero(vis)), "%s, %s rows: %d verdicts differ, first at row %d (%s): device %s, reference %s" % (
            name, layout, len(bad), bad[0], rows[layout][bad[0]], got[layout][bad[0]], vis[bad[0]])
    assert np.array_equal(got["aligned"], got["packed"])


def test_edge_rows_one_by_one(table):
    """the final stack value itself, not a comparison of it, decides: NaN passes, -0.0 does not, the denormal does"""
    ix, rows = table
    for load in FIELD_LOADS:
        for layout in LAYOUTS:
            prog = prog_for(layout, [load])
            ix.set_filter_program(prog, rows[layout])
            ids, _ = verdicts(ix, N)
            assert np.array_equal(ids, np.flatnonzero(sr.visible_rows(N, program=prog, rows=rows[layout]))), (load, layout)
    vis = sr.visible_rows(N, program=prog_for("packed", [X_]), rows=rows["packed"])
    assert EDGES[14] == dict(x=-0.0) and EDGES[15] == dict(x=DENORM) and EDGES[10]["x"] != EDGES[10]["x"]
    assert not vis[14] and vis[15] and vis[10]   # -0.0 is false; the denormal and the NaN are true


# ---- (c) the validator, through the C ABI
def raw_ops(program):
    ops = (_lib.FilterOp * len(program))()
    for i, ins in enumerate(program):
        ops[i].op = _lib.FOP[ins[0]] if isinstance(ins[0], str) else int(ins[0])
        if ins[0] == "const":
            ops[i].dval = float(ins[1])
        elif len(ins) > 1:
            ops[i].arg = int(ins[1])
    return ops


def test_validator(table):
    ix, rows = table
    packed = rows["packed"]
    live = prog_for("packed", MATRIX["f64"])
    want = np.flatnonzero(sr.visible_rows(N, program=live, rows=packed))
    install = lambda program, n_rows: ix.L.eps_index_set_filter_program(ix.h, raw_ops(program), len(program), C.c_void_p(packed.ctypes.data), STRIDE, n_rows)
    for what, program in ACCEPTS:
        assert install(program, N) == 0, (what, ix.L.eps_index_last_error(ix.h).decode())
        ids, _ = verdicts(ix, N)
        assert np.array_equal(ids, np.flatnonzero(sr.visible_rows(N, program=program, rows=packed))), what
    ix.set_filter_program(live, packed)
    for what, program, rows_delta, code, words in REJECTS:
        rc = install(program, N + rows_delta)
        msg = ix.L.eps_index_last_error(ix.h).decode()
        assert rc == code and words in msg, (what, rc, msg)
        ids, _ = verdicts(ix, N)
        assert np.array_equal(ids, want), "%s: the refused program replaced the installed one" % what


# ---- (b) the same verdicts wherever a search judges a row
D = 32
P2_RANKS = (40, 4000)


def p2(ref, ranks=P2_RANKS):
    """@distance > c1 AND @distance <= c2, c1 and c2 two of query 0's own fp64 distances: rows AT c1 are out, rows AT c2 are in"""
    u = np.sort(ref.d64[:, 0])
    c1, c2 = float(u[ranks[0]]), float(u[min(ranks[1], len(u) - 1)])
    assert c1 < c2 and (ref.d64[:, 0] == c1).sum() >= 1 and (ref.d64[:, 0] == c2).sum() >= 1
    return [("dist",), c(c1), (">",), ("dist",), c(c2), ("<=",), ("and",)], c1


def p3(c1):
    """P1 OR @distance * x < c: the distance in arithmetic with a misaligned attribute"""
    return P1 + [("dist",), X_, ("*",), c(0.5 * c1), ("<",), ("or",)]


class Exact:
    """an exact table with attribute rows, its fp64 reference and the programs over it"""

    def __init__(self, n, nq, seed):
        self.n, self.nq = n, nq
        self.X, self.Q = xr.make("integers -8..8", n, D, nq, seed=seed)
        self.ref = xr.Ref(self.X, self.Q, 0)
        assert np.array_equal(self.ref.d64.astype(F).astype(np.float64), self.ref.d64)   # check_exact's own precondition
        self.rows = pack(make_rows(n, seed + 1, edges=False), "packed")
        self.deleted_rows = np.arange(3, n, 11)
        self.deleted = bitset(n, self.deleted_rows)
        prog2, c1 = p2(self.ref)
        self.programs = {"P1": prog_for("packed", P1), "P2": prog_for("packed", prog2), "P3": prog_for("packed", p3(c1))}

    def visible(self, name, q, deleted=False, dist=True):
        d = self.ref.d64[:, q].astype(F).astype(np.float64) if dist else None
        return sr.visible_rows(self.n, deleted=self.deleted if deleted else None, program=self.programs[name], rows=self.rows, dist=d)

    def check(self, res, name, k, queries, deleted=False, dist=True, what=""):
        ids, dist_, cnt = (np.asarray(a)[list(queries)] for a in res) if len(res[0]) != len(queries) else res   # (res: of all queries, or of `queries`)
        for i, q in enumerate(queries):
            vis = self.visible(name, q, deleted, dist)
            assert 2 * k < vis.sum() < self.n - 2 * k, (name, q, vis.sum())   # (k results exist, and the filter hides rows)
            xr.check_exact(ids[i:i + 1], dist_[i:i + 1], cnt[i:i + 1], self.X, None, 0, k, visible=vis, ref=self.ref.take([q]),
                           what="%s %s%s q%d" % (what, name, " + deleted" if deleted else "", q))


@pytest.fixture(scope="module")
def small():
    """20 001 rows: several blocks of the stream scan per query group; beyond 4 x 4096 rows the matrix engine's chain is seeded (plan_chain), so
    its seed stage (merge_lists) judges too.  An explicit engine request has no row minimum of its own."""
    t = Exact(20_001, 40, 2100)
    ix = amd.GpuIndex(D, 0)
    ix.attach_rows(t.X)
    yield t, ix
    ix.close()


def install(ix, t, name, deleted):
    ix.set_deleted(t.deleted if deleted else None)
    ix.set_filter_program(t.programs[name], t.rows)


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_stream_scan(small, name, k):
    t, ix = small
    for deleted in (False, True):
        install(ix, t, name, deleted)
        res = ix.search(t.Q[:6], k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
        t.check(res, name, k, range(6), deleted, what="stream k %d" % k)


@pytest.mark.parametrize("engine", ["FLAT_MFMA", "FLAT_MFMA_I8"])
def test_matrix_engines(small, engine):
    t, ix = small
    for deleted in (False, True):
        install(ix, t, "P1", deleted)
        res = ix.search(t.Q, 10, mode=amd.MODE_FLAT, flat_engine=getattr(amd, engine))
        st = ix.stats()
        assert st["rerank_rows"] > 0 and st["main_kernel_bits"] in (8, 16), st
        t.check(res, "P1", 10, range(0, t.nq, 3), deleted, what=engine)
    for name in ("P2", "P3"):   # a program that reads @distance is served by the exact stream engine, whatever was asked for
        install(ix, t, name, True)
        res = ix.search(t.Q, 10, mode=amd.MODE_FLAT, flat_engine=getattr(amd, engine))
        st = ix.stats()
        assert st["main_kernel_bits"] == 32 and st["rerank_rows"] == 0, st
        t.check(res, name, 10, range(0, t.nq, 3), True, what=engine + " -> stream")


def test_prefilter_call_reads_distance_as_zero(small):
    """eps_search_params.prefilter (PreFilterBruteForceSearch, vec_search_executor.cpp:795): the filter is evaluated without a distance"""
    t, ix = small
    install(ix, t, "P2", True)
    res = ix.search(t.Q[:4], 10, mode=amd.MODE_REFERENCE, prefilter=1)
    assert not t.visible("P2", 0, dist=False).any()   # 0 > c1 is false for every row
    assert (res[2] == 0).all() and (res[0] == -1).all()
    # a program whose verdict with @distance = 0 parts the rows: @distance * x < c  <=>  0 < c
    prog = prog_for("packed", P1 + [("dist",), X_, ("*",), c(-1.0), ("<",), ("or",)])
    t.programs["P1 or 0 < -1"] = prog
    ix.set_filter_program(prog, t.rows)
    for engine in (amd.FLAT_STREAM, amd.FLAT_MFMA):
        res = ix.search(t.Q[:4], 10, mode=amd.MODE_REFERENCE, prefilter=1, flat_engine=engine)
        t.check(res, "P1 or 0 < -1", 10, range(4), True, dist=False, what="prefilter call")
    assert np.array_equal(t.visible("P1 or 0 < -1", 0, True, dist=False), t.visible("P1", 0, True))


def test_two_shards(small):
    t, one = small
    grp = amd.GpuIndex(D, 0, devices=[0, 0])
    grp.attach_rows(t.X)
    for name in ("P1", "P3"):
        for ix in (one, grp):
            install(ix, t, name, True)
        a = one.search(t.Q[:8], 10, mode=amd.MODE_FLAT)
        b = grp.search(t.Q[:8], 10, mode=amd.MODE_FLAT)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        t.check(b, name, 10, range(8), True, what="two shards")
    grp.close()


@pytest.fixture(scope="module")
def big():
    """65 537 rows: the one-pass form's entry rule wants n >= 65 536 (one_pass_fits, csrc/one_pass.hip)"""
    t = Exact(65_537, 16, 2200)
    ix = amd.GpuIndex(D, 0)
    ix.attach_rows(t.X)
    yield t, ix
    ix.close()


@pytest.mark.parametrize("nq", [1, 4, 16])
def test_one_pass_form(big, nq):
    t, ix = big
    for deleted in (False, True):
        install(ix, t, "P1", deleted)
        res = ix.search(t.Q[:nq], 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_MFMA_I8)
        st = ix.stats()
        assert st["one_pass"] == 1, st      # the mask launch (filter_mask_kernel) judged
        t.check(res, "P1", 10, range(nq), deleted, what="one pass nq %d" % nq)
    install(ix, t, "P2", True)
    res = ix.search(t.Q[:nq], 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_MFMA_I8)
    st = ix.stats()
    assert st["one_pass"] == 0 and st["main_kernel_bits"] == 32, st
    t.check(res, "P2", 10, range(nq), True, what="one pass asked, nq %d" % nq)


def test_graph_result_walk():
    """MODE_GRAPH on the committed graph: the traversal is approximate, its result walk is not - the answer is the visible subset, in order, of
    the candidates the unfiltered walk returns, each judged with its OWN distance"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph2000x32.npz"))
    n, L, k = 2000, 500, 10
    X, Q = data(n, 32, 42), data(16, 32, 43)
    rows = pack(make_rows(n, 77, edges=False), "packed")
    deleted = bitset(n, range(5, n, 9))
    ix = amd.GpuIndex(32, 0)
    ix.attach_rows(X)
    ix.set_graph(z["off"].astype(np.int64), z["nbr"].astype(np.int64), int(z["nav"]))
    for T in (1, 4):
        kw = dict(mode=amd.MODE_GRAPH, intra_threads=T, master_queue=L, local_queue=L)
        ix.set_deleted(None)
        ix.set_filter_program(None)
        wi, wd, wc = ix.search_walk(Q, k, L, **kw)
        assert (wc == L).all()
        d200 = np.sort(wd[0])[[20, 200]]
        programs = {"P1": prog_for("packed", P1),
                    "P2": prog_for("packed", [("dist",), c(float(d200[0])), (">",), ("dist",), c(float(d200[1])), ("<=",), ("and",)]),
                    "P3": prog_for("packed", p3(float(d200[1])))}
        for name, prog in programs.items():
            ix.set_deleted(deleted)
            ix.set_filter_program(prog, rows)
            ids, dist, cnt = ix.search(Q, k, **kw)
            for q in range(len(Q)):
                cand = wi[q]
                vis = sr.visible_rows(L, deleted=None, program=prog, rows=rows[cand], dist=wd[q].astype(np.float64))
                vis &= sr.visible_rows(n, deleted=deleted)[cand]
                want = np.flatnonzero(vis)[:k]
                m = int(cnt[q])
                assert m == len(want) and np.array_equal(ids[q, :m], cand[want]), (name, T, q, ids[q], cand[want])
                assert np.array_equal(dist[q, :m].view(np.uint32), wd[q][want].view(np.uint32)), (name, T, q)
                assert (ids[q, m:] == -1).all()
            if name == "P2":
                assert 0 < sum(int(x) for x in cnt) and (dist[:1, :int(cnt[0])] > d200[0]).all()
    ix.close()


# ---- (d) NaN distances across shards: the merge orders heads as make_key orders keys
def test_two_shards_with_nan_rows_equal_the_single_index():
    """about 200 rows, one NaN-holding row per shard, a program that hides most rows, k beyond the visible numbers"""
    n, d = 203, 8
    rng = np.random.default_rng(2300)
    X = rng.integers(-8, 9, (n, d)).astype(F)
    Q = rng.integers(-8, 9, (3, d)).astype(F)
    X[150, 2] = NAN      # shard 0 (even rows)
    X[31, 5] = NAN       # shard 1
    X[77, 1] = INF       # shard 1: (inf - q)^2 = +inf
    rows = pack(make_rows(n, 2301, edges=False), "packed")
    prog = prog_for("packed", [T_, c(100), (">",)])
    rows["t"][[150, 31, 77]] = 127
    vis = sr.visible_rows(n, program=prog, rows=rows)
    k = 40
    assert 8 <= vis.sum() <= k - 5 and vis[[150, 31, 77]].all()
    one, grp = amd.GpuIndex(d, 0), amd.GpuIndex(d, 0, devices=[0, 0])
    out = []
    for ix in (one, grp):
        ix.attach_rows(X)
        ix.set_filter_program(prog, rows)
        out.append(ix.search(Q, k, mode=amd.MODE_FLAT))
        ix.close()
    (ai, ad, ac), (bi, bd, bc) = out
    m = int(vis.sum())
    finite = np.flatnonzero(vis & np.isfinite(X).all(1))
    with np.errstate(invalid="ignore"):
        d64 = xr.dist64(np.where(np.isfinite(X), X, 0), Q, 0)
    for q in range(3):
        want = list(finite[np.lexsort((finite, d64[finite, q]))]) + [77, 31, 150]
        assert int(ac[q]) == m and list(ai[q, :m]) == want and (ai[q, m:] == -1).all(), (q, ai[q])
        assert ad[q, m - 3] == INF and np.isnan(ad[q, m - 2:m]).all() and np.isposinf(ad[q, m:]).all()
    assert np.array_equal(ai, bi) and np.array_equal(ac, bc) and np.array_equal(ad, bd, equal_nan=True), (ai[0], bi[0], ac, bc)


# ---- the drop-in: the reference's own parser and ExprEvaluator against Compiler (dropin/vec_search_executor.cpp: ExprNode tree -> postfix) + the device
from oracle.pyoracle import DROPIN_SO, Ref, dropin_available, ref_available   # noqa: E402

DROPIN_FILTERS = [
    "T <= -3", "S > 1000 AND T < 10", "S >= 1000 OR T > 100", "Big < 1099511627776.0", "B = (S > 0)", "X < 0.25", "W >= 0.25", "B = true", "B <> true AND X > 0",
    "T + S > 0", "W - X > 0", "T * X > 0", "T / W > 0.01", "S / T < W", "Big % 7 >= 2", "T % 4 = 0", "T % 4 <> 0", "NOT (W > 0) OR X > 0.8",
    "NOT (T % 3 = 0) AND (Big % 5 < 2 OR W * 2 - X > 1.5)",
]
DROPIN_DISTANCE_FILTERS = ["@distance > 0.8 AND @distance <= 1.5", "@distance * X < 0.2", "@distance + W > 1 AND B = true", "T <= -3 OR @distance < 0.4"]


def dropin_records(n):
    v = make_rows(n, 41, edges=False)
    v["w"][:8] = [0.0, -0.0, 0.25, 1e300, -1e300, 5e-324, 0.0, 0.0]
    v["t"][:8] = [0, -128, 127, -7, 7, 0, -1, 1]
    v["big"][:8] = [2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 62, -2 ** 62, 2 ** 40 + 1, 2 ** 40, 0, -1]
    v["x"][:8] = [1e-40, -1e-40, 0.25, 0.0, 3e38, -3e38, 1e-30, 0.8]
    v["s"][:8] = [-32768, 32767, 0, 1000, 999, 1001, -3, 3]
    X = data(n, 8, 42)
    recs = [{"ID": i, "B": bool(v["b"][i]), "W": float(v["w"][i]), "T": int(v["t"][i]), "Big": int(v["big"][i]), "S": int(v["s"][i]),
             "X": float(v["x"][i]), "V": [float(a) for a in X[i]]} for i in range(n)]
    return recs


@pytest.fixture(scope="module")
def dropin():
    if os.path.isdir("/root/reference/engine"):
        from vectordb_amd.build import build
        from oracle.pyoracle import build_dropin
        build()
        build_dropin()
    if not dropin_available():
        pytest.skip("oracle/_ref/dropin/libepsilla_dropin.so not built (needs the reference's sources: `make -C dropin OUT=$PWD/oracle/_ref/dropin`)")
    return Ref(DROPIN_SO)


@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_dropin_filters_match_the_reference_evaluator(dropin, tmp_path, monkeypatch):
    """{ID INT, B BOOL, W DOUBLE, T TINYINT, Big BIGINT, S SMALLINT, X FLOAT, V}: behind the 4-byte key the reference packs W at byte 5 and Big at
    byte 14 - the misaligned layout through the real path.  2 500 records (above the select crossover of 2 048): filtered vector searches, and
    filter-only gets served by the device (EPS_DROPIN_SELECT_MIN_ROWS=0) and by the host loop; the reference DBServer is the expectation."""
    n = 2500
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True}, {"name": "B", "dataType": "BOOL"},
                                       {"name": "W", "dataType": "DOUBLE"}, {"name": "T", "dataType": "TINYINT"}, {"name": "Big", "dataType": "BIGINT"},
                                       {"name": "S", "dataType": "SMALLINT"}, {"name": "X", "dataType": "FLOAT"},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 8, "metricType": "EUCLIDEAN"}]}
    recs = dropin_records(n)
    Q = data(5, 8, 43)
    windows = [dict(limit=n), dict(skip=100, limit=200), dict(skip=300, limit=1000)]   # (every filter leaves more than 400 rows)
    runs = {}
    for lib, name, min_rows in ((Ref(), "ref", None), (dropin, "device", "0"), (dropin, "host", str(10 ** 9))):
        if min_rows is not None:
            monkeypatch.setenv("EPS_DROPIN_SELECT_MIN_ROWS", min_rows)
        db = lib.db(str(tmp_path / name))
        assert db.create_table(schema) == 0
        for s in range(0, n, 500):
            assert db.insert("T", recs[s:s + 500]) == 0
        assert db.delete("T", [3, 700, 2047, 2048, n - 1]) == 0
        out = {}
        for flt in DROPIN_FILTERS + ["@distance < 1 AND T > 0"]:
            for wi, w in enumerate(windows):
                out[("get", flt, wi)] = db.get("T", fields=("ID",), flt=flt, **w)
        if name != "host":
            for flt in DROPIN_FILTERS + DROPIN_DISTANCE_FILTERS:
                for qi, q in enumerate(Q):
                    out[("search", flt, qi)] = db.search("T", "V", q, 20, fields=("ID",), flt=flt)
        db.close()
        runs[name] = out
    for name in ("device", "host"):
        nonempty = 0
        for key, (rc, got) in runs[name].items():
            rc_r, want = runs["ref"][key]
            assert rc == rc_r == 0, (name, key, rc, rc_r, got if rc else want)
            assert [x["ID"] for x in got] == [x["ID"] for x in want], (name, key, [x["ID"] for x in got][:10], [x["ID"] for x in want][:10])
            if key[0] == "search":
                assert np.allclose([x["@distance"] for x in got], [x["@distance"] for x in want], rtol=1e-4), (name, key)
            nonempty += len(want) > 0
        assert nonempty >= 0.9 * len(runs[name]), (name, nonempty, len(runs[name]))
