"""The inverted lists of GpuSparseIndex on the device (eps_sparse_index_build_inverted; csrc/sparse_inverted.hip) against tests/sparse_inv_ref.py and
tests/sparse_ref.py: the layout equals the model's exactly; ids, distance bits after + 0.0f and counts of every search are compared for EQUALITY
(sparse_ref.same_answer) - there is no tolerance in this file.  Tables of ties go through their exact dense image, the continuous table through the
sequential model: a fused product or a wrong term order fails that one.

k is at most 1024, so where a table has more rows than that "every distance is compared" is done in windows: all rows but 1024 consecutive ones are
deleted, k = 1024, and the windows cover the table."""
import os

import numpy as np
import pytest

import sparse_inv_ref as si
import sparse_ref as sr
from helpers import bitset

pytestmark = pytest.mark.gpu
F = np.float32
METRICS = (sr.COSINE, sr.DOT)
T = si.inv_constant("SPARSE_INV_TILE_ROWS")
DIM = 2 ** 24
QMAX = sr.host_constant("SPARSE_MAX_QUERY_NNZ")


def index(metric, dim=DIM):
    from vectordb_amd import GpuSparseIndex
    return GpuSparseIndex(dim, sr.METRIC_NAMES[metric])


def head(t, m):
    e = t[0][m]
    return t[0][:m + 1].copy(), t[1][:e].copy(), t[2][:e].copy()


def dev(t):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in t)


def same_layout(ix, X, dim, what=""):
    got, want = ix.inverted_arrays(), si.transpose(X, dim)
    for g, w, name in zip(got, want, ("col_offsets", "rows", "values")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32) if name == "values" else g, w.view(np.uint32) if name == "values" else w), (what, name)
    info = ix.inverted_info()
    assert info["built"] and info["columns"] == dim and info["postings"] == len(X[1])
    assert info["longest_column"] == (int(np.diff(want[0]).max()) if len(X[1]) else 0)


class Pair:
    """the same table, bitset and id map on two handles: `inv` holds inverted lists, `scan` holds none - the A/B of the two engines"""

    def __init__(self, metric, dim=DIM):
        self.inv, self.scan = index(metric, dim), index(metric, dim)

    def attach(self, X):
        for ix in (self.inv, self.scan):
            ix.attach_csr(*X)
        self.inv.build_inverted()

    def set_deleted(self, bits):
        for ix in (self.inv, self.scan):
            ix.set_deleted(bits)

    def set_id_map(self, base, stride):
        for ix in (self.inv, self.scan):
            ix.set_id_map(base, stride)

    def close(self):
        for ix in (self.inv, self.scan):
            ix.close()


def both_engines(p, Q, k, want, what):
    """the search on the inverted lists equals the model; the same call on the scan's handle equals it too, so the two engines equal each other"""
    got = p.inv.search(Q, k)
    assert p.inv.inverted_info()["last_engine"] == 2, what
    sr.same_answer(got, want, what + " (inverted)")
    scan = p.scan.search(Q, k)
    assert p.scan.inverted_info()["last_engine"] == 1 and not p.scan.inverted_info()["built"], what
    sr.same_answer(scan, want, what + " (scan)")
    sr.same_answer(got, scan, what + " (inverted against scan)")


# ---- 1. the layout
@pytest.fixture(scope="module")
def ties():
    X, Q = sr.ties_table(1000, 33, seed=1, dim=DIM)
    return X, Q, {m: sr.dist_dense(X, Q, m, F) for m in METRICS}


def test_layout_equals_the_stable_transpose(ties):
    X, Q, _ = ties
    assert X[1].min() == 0 and X[1].max() == DIM - 1   # columns 0 and dim - 1 are in the pool
    ix = index(sr.DOT)
    ix.attach_csr(*X)
    assert not ix.inverted_info()["built"] and ix.inverted_info()["last_engine"] == 0
    ix.build_inverted()
    same_layout(ix, X, DIM, "ties")
    ix.close()
    Xc, _ = sr.cont_table()
    ix = index(sr.COSINE, dim=400)   # two sort passes
    ix.attach_csr(*Xc)
    ix.build_inverted()
    same_layout(ix, Xc, 400, "continuous")
    Xd = dev(Xc)                     # borrowed device arrays: the image is the handle's own
    ix.attach_csr(*Xd)
    assert not ix.inverted_info()["built"]
    ix.build_inverted()
    same_layout(ix, Xc, 400, "borrowed")
    ix.close()
    ix = index(sr.DOT, dim=200)      # one sort pass
    small = sr.csr([([1, 5, 199], [1, 2, 3]), ([], []), ([0, 5], [4, -1]), ([5], [0])])
    for t, what in ((small, "an empty row"), (sr.csr([]), "an empty table"), (sr.csr([([], [])] * 5), "only empty rows")):
        ix.attach_csr(*t)
        ix.build_inverted()
        same_layout(ix, t, 200, what)
        ids, dist, counts = ix.search(sr.csr([([5], [2])]), 3)
        assert ix.inverted_info()["last_engine"] == 2 and counts.tolist() == [min(3, sr.n_rows(t))], what
    # a table long enough for several sort blocks and a second step inside a block
    Xb, _ = sr.ties_table(20000, 1, seed=2, max_nz=16, dim=DIM)
    big = index(sr.DOT)
    big.attach_csr(*Xb)
    big.build_inverted()
    same_layout(big, Xb, DIM, "20000 rows")
    big.close()
    ix.close()
    del Xd


# ---- 2. tables of ties, both engines
@pytest.mark.parametrize("metric", METRICS)
def test_ties_tables_on_both_engines(ties, metric):
    X, Q, D = ties
    assert np.isnan(D[sr.COSINE]).any()   # empty rows: NaN rows rank last under COSINE
    p = Pair(metric)
    for n in (1, 63, 64, 65, 257, 1000):
        p.attach(head(X, n))
        for nq in (1, 3, 33):
            for k in (1, 10, 64, 65, 1024):
                both_engines(p, head(Q, nq), k, sr.topk(D[metric][:n, :nq], k), "n %d nq %d k %d" % (n, nq, k))
    # and on ONE handle: the image answers, then - dropped - the scan, with the same answer
    want = sr.topk(D[metric], 10)
    sr.same_answer(p.inv.search(Q, 10), want)
    assert p.inv.inverted_info()["last_engine"] == 2
    p.inv.drop_inverted()
    sr.same_answer(p.inv.search(Q, 10), want)
    assert p.inv.inverted_info()["last_engine"] == 1
    p.close()


# ---- 3. tile edges
def windows(n):
    return [(b, min(n, b + si.MAX_K)) for b in range(0, n, si.MAX_K)]


@pytest.mark.parametrize("metric", METRICS)
def test_tile_edges(metric):
    Xfull, Q, (A, B, Cc) = si.tile_table(2 * T + 1, T)
    assert np.diff(Q[0]).tolist() == [0, 1, 64, 65, QMAX]
    Dfull = sr.dist_dense(Xfull, Q, metric, F)   # the ties model, once
    p = Pair(metric)
    ix = p.inv
    for n in (T - 1, T, T + 1, 2 * T + 1):
        X, D = head(Xfull, n), Dfull[:n]
        off, rows, _ = si.transpose(X, DIM)
        assert off[A + 1] - off[A] == n and rows[off[B]:off[B + 1]].tolist() == [r for r in (T - 1, T) if r < n] and off[Cc] == off[Cc + 1]
        p.attach(X)
        both_engines(p, Q, 10, sr.topk(D, 10), "n %d k 10" % n)
        for lo, hi in windows(n):   # "k = n": every row's distance, 1024 visible rows at a time
            vis = np.zeros(n, bool)
            vis[lo:hi] = True
            ix.set_deleted(bitset(n, np.flatnonzero(~vis)))
            got = ix.search(Q, si.MAX_K)
            assert ix.inverted_info()["last_engine"] == 2
            sr.same_answer(got, sr.topk(D, si.MAX_K, visible=vis), "n %d rows %d .. %d" % (n, lo, hi))
        ix.set_deleted(None)
    p.close()


@pytest.mark.parametrize("metric", METRICS)
def test_many_workgroups_and_a_real_merge(metric):
    X, Q = sr.ties_table(20000, 33, seed=2, max_nz=16, dim=DIM)
    D = sr.dist_dense(X, Q, metric, F)
    p = Pair(metric)
    p.attach(X)
    for k in (10, 1024):
        both_engines(p, Q, k, sr.topk(D, k), "k %d" % k)
    p.close()


# ---- 4. the continuous table: the test a fused product or a wrong term order fails
@pytest.mark.parametrize("metric", METRICS)
def test_continuous_table_against_the_sequential_model(metric):
    X, Q = sr.cont_table()
    D = sr.dist_table(X, Q, metric)
    assert si.changed_words(si.dist_terms(X, Q, metric, 400), D) == 0
    # the table is the golden fixture's first 300 x 7 pairs: the model's words are the reference's recorded ones
    z = np.load(os.path.join(sr.ROOT, "tests", "golden", "sparse_reference_distances.npz"))
    assert np.array_equal(z["x_indices"][:len(X[1])], X[1]) and si.changed_words(z["bits"][:300, :7, metric].view(F), D) == 0
    n = sr.n_rows(X)
    p = Pair(metric, dim=400)
    p.attach(X)
    both_engines(p, Q, 10, sr.topk(D, 10), "k 10")
    both_engines(p, Q, n, sr.topk(D, n), "k n")   # every distance
    ids, dist, counts = p.inv.search(Q, n)
    assert (counts == n).all()
    for j in range(sr.n_rows(Q)):
        assert np.array_equal(np.sort(ids[j]), np.arange(n)) and np.array_equal(sr.bits(dist[j]), sr.bits(D[ids[j], j]))
    p.close()


# ---- 5. visibility and ids
@pytest.mark.parametrize("metric", METRICS)
def test_visibility_and_ids(ties, metric):
    import torch
    X, Q, D = ties
    n, d = 257, D[metric][:257]
    p = Pair(metric)
    p.attach(head(X, n))
    gone = list(range(0, n, 3)) + [n - 1]
    vis = np.ones(n, bool)
    vis[gone] = False
    for k in (10, 1024):
        p.set_deleted(bitset(n, gone))                                  # a host bitset, set after the build without a rebuild
        both_engines(p, Q, k, sr.topk(d, k, visible=vis), "host bitset")
        bits_dev = torch.from_numpy(bitset(n, gone)).cuda()              # a device bitset
        p.set_deleted(bits_dev)
        both_engines(p, Q, k, sr.topk(d, k, visible=vis), "device bitset")
        p.set_deleted(None)
        both_engines(p, Q, k, sr.topk(d, k), "cleared")
    two = np.zeros(n, bool)
    two[[5, n // 2]] = True                                              # all but two rows deleted (one of them the empty row)
    p.set_deleted(bitset(n, np.flatnonzero(~two)))
    both_engines(p, Q, 10, sr.topk(d, 10, visible=two), "two rows left")
    p.set_deleted(bitset(n, range(n)))                                  # everything deleted
    ids, dist, counts = p.inv.search(Q, 10)
    assert (counts == 0).all() and (ids == -1).all() and np.isposinf(dist).all() and p.inv.inverted_info()["last_engine"] == 2
    p.set_deleted(bitset(n, gone))
    p.set_id_map(3, 8)
    both_engines(p, Q, 10, sr.topk(d, 10, visible=vis, base=3, stride=8), "id map")
    assert p.inv.inverted_info()["built"]                                   # neither call touched the image
    p.close()


def test_device_queries_and_outputs(ties):
    import torch
    X, Q, D = ties
    n, k = 257, 10
    for metric in METRICS:
        want = sr.topk(D[metric][:n], k)
        ix = index(metric)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ix.use_torch_stream()
            Xd = dev(head(X, n))
            ix.attach_csr(*Xd)
            ix.build_inverted()
            q_off, q_idx, q_val = Q[0], *dev(Q[1:])
            got = ix.search((q_off, q_idx, q_val), k)                    # device queries, device results, on the torch stream
            assert all(hasattr(a, "data_ptr") for a in got)
            ix.synchronize()
            stream.synchronize()
        assert ix.inverted_info()["last_engine"] == 2
        sr.same_answer(got, want, "device")
        out = (np.full((33, k), 7, np.int64), np.full((33, k), 7, F), np.full(33, 7, np.int32))
        ix.search(Q, k, out=out)
        sr.same_answer(out, want, "out=")
        s = ix.stats()
        assert s["dist_evals"] == n * 33 and s["main_kernel_rows"] == n and s["main_kernel_queries"] == 33 and s["main_kernel_bits"] == 32
        assert s["main_kernel_launches"] == 1 and s["main_kernel_ms"] > 0 and s["kernel_ms"] >= s["main_kernel_ms"]
        ix.close()
        del Xd


# ---- 6. lifecycle and refusals
def test_lifecycle_and_refusals(ties):
    from vectordb_amd import EpsillaError, GpuSparseIndex
    X, Q, D = ties
    n = 100

    def refused(code, text, call, *a, **kw):
        with pytest.raises(EpsillaError) as e:
            call(*a, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    # an EUCLIDEAN handle: refused, and the next search is the scan's, unchanged
    l2 = index(sr.L2)
    l2.attach_csr(*head(X, n))
    want = sr.topk(sr.dist_dense(X, Q, sr.L2, F)[:n], 10)
    refused(50002, "no term-at-a-time form", l2.build_inverted)
    sr.same_answer(l2.search(Q, 10), want, "EUCLIDEAN after the refusal")
    assert l2.inverted_info() == {"built": False, "columns": 0, "postings": 0, "longest_column": 0, "last_engine": 1}
    l2.drop_inverted()
    l2.close()
    # dim above the limit
    wide = GpuSparseIndex(DIM + 1, "DOT_PRODUCT")
    wide.attach_csr(*head(X, n))
    refused(50002, str(DIM), wide.build_inverted)
    sr.same_answer(wide.search(Q, 10), sr.topk(D[sr.DOT][:n], 10), "dim 2^24 + 1 after the refusal")
    assert not wide.inverted_info()["built"] and wide.inverted_info()["last_engine"] == 1
    wide.close()
    ix = index(sr.DOT)
    refused(30000, "no table", ix.build_inverted)                        # build without a table
    ix.drop_inverted()                                                   # nothing to drop: fine
    with pytest.raises(ValueError, match="build_inverted first"):
        ix.inverted_arrays()
    assert ix.L.eps_sparse_index_get_inverted(ix.h, None, None, None) == 30000
    ix.attach_csr(*head(X, n))
    ix.build_inverted()
    ix.build_inverted()                                                  # twice: rebuilt
    same_layout(ix, head(X, n), DIM, "built twice")
    sr.same_answer(ix.search(Q, 10), sr.topk(D[sr.DOT][:n], 10))
    assert ix.inverted_info()["last_engine"] == 2
    # a malformed query is refused with the scan's message; so is a query of 4097 terms
    refused(30000, "query 1: indices must be strictly increasing", ix.search, sr.csr([([1], [1]), ([5, 3], [1, 1])]), 3)
    refused(30000, "query 0: an index outside [0, dim)", ix.search, sr.csr([([DIM], [1])]), 3)
    bad_q = sr.csr([([1], [1]), ([5, 3], [1, 1])])
    refused(30000, "query 1: indices must be strictly increasing", ix.search, (bad_q[0], *dev(bad_q[1:])), 3)
    over = (np.array([0, 2, 2 + QMAX + 1], np.int64), np.arange(QMAX + 3, dtype=np.int32), np.ones(QMAX + 3, F))
    refused(50002, "query 1 has %d non-zeros; at most %d per query" % (QMAX + 1, QMAX), ix.search, over, 3)
    for k in (0, 1025):
        q = sr.csr([([1, 7], [1, 1])])
        ids, dist = np.empty((1, 3), np.int64), np.empty((1, 3), F)
        rc = ix.L.eps_sparse_index_search(ix.h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, 1, k, ids.ctypes.data, dist.ctypes.data, None)
        assert rc == 30000 and b"k must be in [1, 1024]" in ix.L.eps_sparse_index_last_error(ix.h)
    # attach_csr forgets the image
    ix.attach_csr(*head(X, 65))
    assert ix.inverted_info()["built"] is False and ix.inverted_info()["postings"] == 0
    sr.same_answer(ix.search(Q, 10), sr.topk(D[sr.DOT][:65], 10), "re-attached")
    assert ix.inverted_info()["last_engine"] == 1
    ix.build_inverted()
    ix.drop_inverted()
    ix.drop_inverted()                                                   # twice
    sr.same_answer(ix.search(Q, 10), sr.topk(D[sr.DOT][:65], 10), "dropped")
    assert ix.inverted_info()["last_engine"] == 1 and not ix.inverted_info()["built"]
    ix.close()
