"""GpuIndex.search_hybrid / eps_index_search_hybrid on the MI355X (csrc/hybrid.hip): ids, score words, dense words, sparse words and counts are compared
for EQUALITY with tests/hybrid_ref.py everywhere - there is no tolerance in this file but exact_ref's derived bound on the continuous dense term.
Tables of ties (small integers, power-of-two weights: every sum is exact in fp32 in any order) get their two distance tables from numpy alone;
continuous tables get them from the two handles' own searches with k = n, which pins the bits the call promises to keep."""
import numpy as np
import pytest

import exact_ref as er
import hybrid_ref as hr
import select_ref as sel
import sparse_inv_ref as si
import sparse_ref as sr
import vectordb_amd as amd
from test_hybrid_ref_cpu import host_constant
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu
F = np.float32
T, QMAX = host_constant("HYB_TILE_ROWS"), host_constant("HYB_MAX_QUERY_NNZ")
SDIM = 2 ** 24
L2, COS, DOT = 0, 1, 2


def ints(rng, n, dim):
    return rng.integers(-3, 4, size=(n, dim)).astype(F)


def pair(X, S, dm, sm, sdim=SDIM):
    ix, sx = amd.GpuIndex(X.shape[1], sr.METRIC_NAMES[dm]), amd.GpuSparseIndex(sdim, sr.METRIC_NAMES[sm])
    ix.attach_rows(X)
    sx.attach_csr(*S)
    sx.build_inverted()
    return ix, sx


def tables(X, Q, S, SQ, dm, sm):
    """D, S [nq][n] of a ties table, from the raw arrays: fp64 (exact on integers), the sparse COSINE epilogue through sparse_ref"""
    return er.dist64(X, Q, dm).T.astype(F), np.ascontiguousarray(sr.dist_dense(S, SQ, sm, F).T)


# ---- 1. tables of ties at the kernel's edges: 3 dense x 2 sparse metrics; scalar path, G < 64, three pieces per lane; every KPL; NQ 1, 2, 4
@pytest.mark.parametrize("n,dim,nq,k,dm,sm", [
    (1, 1, 1, 1, L2, DOT), (T - 1, 3, 3, 10, COS, COS), (T, 4, 4, 64, DOT, DOT), (T + 1, 770, 5, 65, L2, COS), (T + 1, 768, 5, 129, COS, DOT),
    (2 * T + 3, 4, 2, 1024, L2, DOT),
    (3 * (2 * T + 64) + 2 * T + 1, 1, 2048, 129, DOT, COS)])   # 2048 one-query tiles leave 4 wavefronts: the last walks two tiles plus one row
def test_tables_of_ties(n, dim, nq, k, dm, sm):
    rng = np.random.default_rng(n + dim)
    m = min(nq, 8)   # (the long batch repeats 8 queries)
    X, Q = ints(rng, n, dim), ints(rng, m, dim)
    S, SQ = sr.ties_table(n, m, seed=n, dim=SDIM)
    want = hr.topk(*tables(X, Q, S, SQ, dm, sm), 0.5, 2.0, k)
    rep = np.arange(nq) % m
    SQr = sr.csr([sr.row(SQ, j) for j in rep])
    ix, sx = pair(X, S, dm, sm)
    got = ix.search_hybrid(sx, Q[rep], SQr, k, 0.5, 2.0)
    hr.same(got, tuple(a[rep] for a in want), "ties n %d dim %d" % (n, dim))
    st = ix.stats()
    assert st["dist_evals"] == n * nq and st["main_kernel_bits"] == 32 and st["main_kernel_rows"] == n and st["main_kernel_queries"] == nq


# ---- 2. sparse tile edges: a column in every row, one on rows T - 1 and T only, one in no row; queries of 0 / 1 / 64 / 65 / QMAX terms
@pytest.mark.parametrize("sm", [COS, DOT])
def test_sparse_tile_edges(sm):
    S, SQ4, (A, B, C) = si.tile_table(T + 1, T)
    rows = sr.rows_of(SQ4)
    keep = np.isin(rows[4][0], [A, B, C])
    some = np.flatnonzero(keep | (np.cumsum(~keep) <= QMAX - 3))   # A, B, C and enough of the others
    SQ = sr.csr(rows[:4] + [(rows[4][0][some], rows[4][1][some])])
    assert np.diff(SQ[0]).tolist() == [0, 1, 64, 65, QMAX] and {A, B, C} <= set(sr.row(SQ, 4)[0].tolist())
    rng = np.random.default_rng(2)
    X, Q = ints(rng, T + 1, 4), ints(rng, 5, 4)
    ix, sx = pair(X, S, L2, sm)
    got = ix.search_hybrid(sx, Q, SQ, T + 1, 1.0, 0.25)
    hr.same(got, hr.topk(*tables(X, Q, S, SQ, L2, sm), 1.0, 0.25, T + 1), "tile edges")
    if sm == COS:   # the empty query: every score NaN, returned in id order
        assert np.isnan(got[1][0]).all() and got[0][0].tolist() == list(range(T + 1)) and got[4][0] == T + 1
    over = sr.csr([(rows[4][0][:QMAX + 1], rows[4][1][:QMAX + 1])])
    with pytest.raises(EpsillaError) as e:
        ix.search_hybrid(sx, Q[:1], over, 10)
    assert e.value.code == 50002 and "at most %d" % QMAX in str(e.value)


# ---- 3 / 4. continuous tables: the two handles' own bits, combined by the model; degenerate weights need no model
def cont_sparse(rng, m, dim=400):
    out = []
    for _ in range(m):   # (no empty row or query: COSINE stays finite, so a zero weight leaves the other term alone)
        c = np.sort(rng.choice(dim, size=int(rng.integers(1, 41)), replace=False))
        out.append((c, (rng.uniform(0.25, 4, len(c)) * rng.choice([-1, 1], len(c))).astype(F)))
    return sr.csr(out)


@pytest.fixture(scope="module", params=[(L2, DOT, 96), (COS, COS, 770), (DOT, COS, 768)])
def cont(request):
    dm, sm, dim = request.param
    rng = np.random.default_rng(dim)
    n, nq = 1000, 5
    X, Q = rng.standard_normal((n, dim)).astype(F), rng.standard_normal((nq, dim)).astype(F)
    if dm == COS:
        X, Q = er.unit(X).astype(F), er.unit(Q).astype(F)
    S, SQ = cont_sparse(rng, n), cont_sparse(rng, nq)
    ix, sx = pair(X, S, dm, sm, sdim=400)
    dense = ix.search(Q, n, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    sparse = sx.search(SQ, n)
    D, Sd = np.empty((nq, n), F), np.empty((nq, n), F)
    for j in range(nq):
        assert dense[2][j] == n == sparse[2][j]
        D[j, dense[0][j]], Sd[j, sparse[0][j]] = dense[1][j], sparse[1][j]
    return ix, sx, X, Q, SQ, D, Sd, dm, (dense, sparse)


@pytest.mark.parametrize("k", [10, 130])
def test_continuous_tables_keep_both_handles_bits(cont, k):
    ix, sx, X, Q, SQ, D, Sd, dm, _ = cont
    got = ix.search_hybrid(sx, Q, SQ, k, 0.7, 0.3)
    hr.same(got, hr.topk(D, Sd, 0.7, 0.3, k), "continuous")
    ref = er.Ref(X, Q, dm)
    for j in range(len(Q)):   # the returned dense term against fp64, within the documented tree's bound
        assert (np.abs(got[2][j].astype(np.float64) - ref.d64[got[0][j], j]) <= ref.bound("tree")[got[0][j], j]).all()


def test_degenerate_weights(cont):
    ix, sx, X, Q, SQ, D, Sd, dm, (dense, sparse) = cont
    ids, score, _, _, counts = ix.search_hybrid(sx, Q, SQ, 100, 1.0, 0.0)
    sr.same_answer((ids, score, counts), (dense[0][:, :100], dense[1][:, :100], np.full(len(Q), 100, np.int32)), "w_sparse = 0")
    ids, score, _, _, counts = ix.search_hybrid(sx, Q, SQ, 100, 0.0, 1.0)
    sr.same_answer((ids, score, counts), (sparse[0][:, :100], sparse[1][:, :100], np.full(len(Q), 100, np.int32)), "w_dense = 0")


# ---- 5 - 7. visibility, buffers, refusals on one ties table
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(9)
    n, nq = T + 1, 5
    X, Q = ints(rng, n, 4), ints(rng, nq, 4)
    S, SQ = sr.ties_table(n, nq, seed=4, dim=SDIM)
    ix, sx = pair(X, S, L2, DOT)
    return ix, sx, X, Q, S, SQ, tables(X, Q, S, SQ, L2, DOT)


def reset(ix, sx):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)
    sx.set_deleted(None)
    sx.set_id_map(0, 1)


def test_visibility_and_id_maps(small):
    ix, sx, X, Q, S, SQ, (D, Sd) = small
    n, rng = len(X), np.random.default_rng(1)
    dh, ds = (np.packbits(rng.random((n + 7) // 8 * 8) < p, bitorder="little") for p in (0.4, 0.3))
    gone = lambda b: np.unpackbits(b, bitorder="little")[:n].astype(bool)   # noqa: E731
    col = rng.integers(-100, 100, n).astype(np.int32)
    attr = np.zeros(n, ROW8)
    attr["a"], attr["x"] = rng.integers(-100, 100, n), rng.random(n, dtype=F)
    prog = [("i32", 0), ("const", 3), ("%",), ("const", 0), ("=",), ("f32", 4), ("const", 0.5), (">",), ("or",)]
    most = np.packbits(np.arange((n + 7) // 8 * 8) >= 7, bitorder="little")   # 7 rows stay: k above the visible count
    cases = [("bitset on h", lambda: ix.set_deleted(dh), ~gone(dh)), ("bitset on s", lambda: sx.set_deleted(ds), ~gone(ds)),
             ("both bitsets", lambda: (ix.set_deleted(dh), sx.set_deleted(ds)), ~gone(dh) & ~gone(ds)),
             ("int column", lambda: ix.set_int_filter(col, "<", 13), sel.visible_rows(n, int_filter=(col, "<", 13))),
             ("program and s's bitset", lambda: (ix.set_filter_program(prog, attr), sx.set_deleted(ds)), sel.visible_rows(n, program=prog, rows=attr) & ~gone(ds)),
             ("seven rows", lambda: sx.set_deleted(most), ~gone(most))]
    for what, install, vis in cases:
        reset(ix, sx)
        install()
        ix.set_id_map(7, 3)
        sx.set_id_map(100, 5)   # (never read)
        for k in (10, 130):
            hr.same(ix.search_hybrid(sx, Q, SQ, k, 2.0, 1.0), hr.topk(D, Sd, 2.0, 1.0, k, vis, base=7, stride=3), what)
    reset(ix, sx)


def test_buffers(small):
    import torch
    ix, sx, X, Q, S, SQ, (D, Sd) = small
    reset(ix, sx)
    want = hr.topk(D, Sd, 1.0, 1.0, 10)
    got = ix.search_hybrid(sx, Q, SQ, 10, parts=False)   # host outputs, dense_out = sparse_out = NULL
    assert got[2] is None and got[3] is None
    hr.same(got, want, "no parts")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ix.use_torch_stream()
        dq = torch.from_numpy(Q).cuda()
        dsq = (SQ[0], torch.from_numpy(SQ[1]).cuda(), torch.from_numpy(SQ[2]).cuda())
        out = ix.search_hybrid(sx, dq, dsq, 10)   # device queries on the caller's stream give device results on it
        assert all(hasattr(t, "data_ptr") for t in out)
        stream.synchronize()
        hr.same(out, want, "device")
        mine = (out[0], out[1], None, out[3], out[4])
        hr.same(ix.search_hybrid(sx, Q, SQ, 10, out=mine), want, "host in, device out, no dense_out")
    ix.set_stream(None)


def test_refusals(small):
    import torch
    ix, sx, X, Q, S, SQ, (D, Sd) = small
    reset(ix, sx)
    nq = len(Q)
    want = hr.topk(D, Sd, 1.0, 1.0, 10)
    want_d, want_s = sr.topk(D.T, 10), sr.topk(Sd.T, 10)
    out = [np.full((nq, 10), -7, np.int64)] + [np.full((nq, 10), -7, F) for _ in range(3)] + [np.full(nq, -7, np.int32)]

    def refused(code, text, s=None, q=Q, k=10, w=(1.0, 1.0), bufs=out, index=None):
        with pytest.raises(EpsillaError) as e:
            (index or ix).search_hybrid(s or sx, q, SQ, k, *w, out=bufs)
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert all((np.asarray(b) == -7).all() for b in out)   # untouched
        hr.same(ix.search_hybrid(sx, Q, SQ, 10), want, "after a refusal")
        sr.same_answer(ix.search(Q, 10, mode=amd.MODE_FLAT), want_d, "dense search after a refusal")
        sr.same_answer(sx.search(SQ, 10), want_s, "sparse search after a refusal")

    short = amd.GpuSparseIndex(SDIM, "DOT_PRODUCT")
    short.attach_csr(*sr.csr(sr.rows_of(S)[:-1]))
    short.build_inverted()
    refused(30000, "same record", s=short)
    plain, l2 = amd.GpuSparseIndex(SDIM, "DOT_PRODUCT"), amd.GpuSparseIndex(SDIM, "EUCLIDEAN")
    plain.attach_csr(*S)
    l2.attach_csr(*S)
    refused(50002, "build_inverted", s=plain)
    refused(50002, "EUCLIDEAN", s=l2)
    for k in (0, 1025):
        bufs = [np.full((nq, k), -7, a.dtype) for a in out[:4]] + out[4:]
        with pytest.raises(EpsillaError) as e:
            ix.search_hybrid(sx, Q, SQ, k, out=bufs)
        assert e.value.code == 30000 and "k must be" in str(e.value) and all((b == -7).all() for b in bufs)
    for w in ((np.nan, 1.0), (1.0, np.inf), (-np.inf, 1.0)):
        refused(30000, "finite", w=w)
    attr = np.zeros(len(X), ROW8)
    ix.set_filter_program([("dist",), ("const", 3.0), ("<",)], attr)
    with pytest.raises(EpsillaError) as e:
        ix.search_hybrid(sx, Q, SQ, 10, out=out)
    assert e.value.code == 30000 and "@distance" in str(e.value) and all((b == -7).all() for b in out)
    reset(ix, sx)
    sharded = amd.GpuIndex(4, "EUCLIDEAN", devices=[0])
    sharded.attach_rows(X)
    refused(50002, "sharded", index=sharded)
    mixed = [out[0], torch.full((nq, 10), -7.0, device="cuda")] + out[2:]
    refused(30000, "host or all be device", bufs=mixed)
    assert (mixed[1].cpu().numpy() == -7).all()
    assert ix.L.eps_index_search_hybrid(ix.h, sx.h, None, None, None, None, 0, 10, 1.0, 1.0, None, None, None, None, None) == 0   # nq = 0
