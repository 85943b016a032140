"""GpuSparseIndex on the device (eps_sparse_index_*; csrc/sparse.hip) against tests/sparse_ref.py: ids, distance bits after + 0.0f and counts are
compared for EQUALITY everywhere - there is no tolerance in this file.  Tables of ties go through their exact dense image, the continuous table
and the golden fixture through the sequential model and the reference's recorded bits: a fused multiply-add in the scan fails those two."""
import numpy as np
import pytest

import sparse_ref as sr
from helpers import bitset

pytestmark = pytest.mark.gpu
F = np.float32
METRICS = (sr.L2, sr.COSINE, sr.DOT)
PIECE = sr.host_constant("SPARSE_PIECE")
QMAX = sr.host_constant("SPARSE_MAX_QUERY_NNZ")


def index(metric, dim=sr.DIM_MAX):
    from vectordb_amd import GpuSparseIndex
    return GpuSparseIndex(dim, sr.METRIC_NAMES[metric])


def head(t, m):
    """the first m rows of a CSR table"""
    e = t[0][m]
    return t[0][:m + 1].copy(), t[1][:e].copy(), t[2][:e].copy()


def dev(t):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in t)


# ---- 1. tables of ties
@pytest.fixture(scope="module")
def ties():
    X, Q = sr.ties_table(1000, 33, seed=1)
    return X, Q, {m: sr.dist_dense(X, Q, m, F) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_ties_tables(ties, metric):
    X, Q, D = ties
    assert np.isnan(D[sr.COSINE]).any()   # empty rows: NaN rows rank last under COSINE
    ix = index(metric)
    for n in (1, 63, 64, 65, 257, 1000):
        ix.attach_csr(*head(X, n))
        assert ix.row_count == n
        for nq in (1, 3, 5, 9, 33):
            for k in (1, 10, 64, 65, 1024):
                got = ix.search(head(Q, nq), k)
                sr.same_answer(got, sr.topk(D[metric][:n, :nq], k), "n %d nq %d k %d" % (n, nq, k))
    ix.close()


# ---- 2. piece edges
@pytest.fixture(scope="module")
def pieces():
    X, Q = sr.piece_table()
    return X, Q, {m: sr.dist_dense(X, Q, m, F) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_piece_edges(pieces, metric):
    X, Q, D = pieces
    lens = np.diff(X[0])
    assert sr.n_rows(X) == 130 and {PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3} <= set(lens.tolist()) and np.diff(Q[0]).tolist() == [0, 1, QMAX, 37]
    ix = index(metric)
    ix.attach_csr(*X)
    for k in (1, 10, 200):
        sr.same_answer(ix.search(Q, k), sr.topk(D[metric], k), "k %d" % k)
    for j in range(4):   # each query alone: one staged query, another kernel form
        one = (Q[0][j:j + 2] - Q[0][j], *sr.row(Q, j))
        sr.same_answer(ix.search(one, 130), sr.topk(D[metric][:, j:j + 1], 130), "query %d" % j)
    ix.close()


# ---- 3. more than one workgroup, a real merge
@pytest.fixture(scope="module")
def big():
    X, Q = sr.ties_table(20000, 33, seed=2, max_nz=16)
    return X, Q, {m: sr.dist_dense(X, Q, m, F) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_many_workgroups_and_a_real_merge(big, metric):
    X, Q, D = big
    assert np.diff(X[0]).max() <= 16
    ix = index(metric)
    ix.attach_csr(*X)
    for k in (10, 1024):
        sr.same_answer(ix.search(Q, k), sr.topk(D[metric], k), "k %d" % k)
    ix.close()


# ---- 4. the continuous table: the test a fused multiply-add fails
@pytest.mark.parametrize("metric", METRICS)
def test_continuous_table_against_the_sequential_model(metric):
    X, Q = sr.cont_table()
    want = sr.topk(sr.dist_table(X, Q, metric), 10)
    ix = index(metric, dim=400)
    ix.attach_csr(*X)
    sr.same_answer(ix.search(Q, 10), want)
    sr.same_answer(ix.search([{"indices": i.tolist(), "values": v.tolist()} for i, v in sr.rows_of(Q)], 10), want, "dict queries")
    ix.close()


# ---- 5. the golden fixture: the reference's recorded bits
@pytest.mark.parametrize("metric", METRICS)
def test_golden_fixture_through_the_device(metric):
    import os
    z = np.load(os.path.join(sr.ROOT, "tests", "golden", "sparse_reference_distances.npz"))
    X = (z["x_offsets"], z["x_indices"], z["x_values"])
    Q = (z["q_offsets"], z["q_indices"], z["q_values"])
    ref = z["bits"][:, :, metric].view(F)
    n = sr.n_rows(X)
    ix = index(metric)
    ix.attach_csr(*X)
    ids, dist, counts = ix.search(Q, n)
    sr.same_answer((ids, dist, counts), sr.topk(ref, n))
    # k = n: every row is returned, so every distance is compared with the recorded one
    assert (counts == n).all()
    for j in range(sr.n_rows(Q)):
        assert np.array_equal(np.sort(ids[j]), np.arange(n))
        assert np.array_equal(sr.bits(dist[j]), sr.bits(ref[ids[j], j]))
    ix.close()


# ---- 6. visibility and ids
def test_visibility_and_ids(ties):
    import torch
    X, Q, D = ties
    n, d = 257, D[sr.L2][:257]
    ix = index(sr.L2)
    ix.attach_csr(*head(X, n))
    gone = list(range(0, n, 3)) + [n - 1]
    vis = np.ones(n, bool)
    vis[gone] = False
    for k in (10, 1024):
        ix.set_deleted(bitset(n, gone))                                  # a host bitset
        sr.same_answer(ix.search(Q, k), sr.topk(d, k, visible=vis), "host bitset")
        bits_dev = torch.from_numpy(bitset(n, gone)).cuda()              # a device bitset
        ix.set_deleted(bits_dev)
        sr.same_answer(ix.search(Q, k), sr.topk(d, k, visible=vis), "device bitset")
        ix.set_deleted(None)                                             # NULL clears
        sr.same_answer(ix.search(Q, k), sr.topk(d, k), "cleared")
    ix.set_deleted(bitset(n, range(n)))                                  # everything deleted
    ids, dist, counts = ix.search(Q, 10)
    assert (counts == 0).all() and (ids == -1).all() and np.isposinf(dist).all()
    ix.set_deleted(bitset(n, gone))
    ix.set_id_map(3, 8)
    sr.same_answer(ix.search(Q, 10), sr.topk(d, 10, visible=vis, base=3, stride=8), "id map")
    ix.attach_csr(*head(X, n))                                           # re-attaching forgets the bitset (the id map stays)
    sr.same_answer(ix.search(Q, 10), sr.topk(d, 10, base=3, stride=8), "re-attached")
    ix.attach_csr(*head(X, 0))                                           # an empty table
    ids, dist, counts = ix.search(Q, 10)
    assert ix.row_count == 0 and (counts == 0).all() and (ids == -1).all() and np.isposinf(dist).all()
    ix.close()


# ---- 7. buffers
def test_device_buffers_and_out(ties):
    import torch
    X, Q, D = ties
    n, k = 257, 10
    for metric in METRICS:
        want = sr.topk(D[metric][:n], k)
        host = index(metric)
        host.attach_csr(*head(X, n))
        host_answer = host.search(Q, k)
        sr.same_answer(host_answer, want)
        ix = index(metric)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ix.use_torch_stream()
            Xd = dev(head(X, n))
            ix.attach_csr(*Xd)                                           # device-resident CSR is borrowed
            q_off, q_idx, q_val = Q[0], *dev(Q[1:])
            got = ix.search((q_off, q_idx, q_val), k)                    # device queries, device results, on the torch stream
            assert all(hasattr(a, "data_ptr") for a in got)
            ix.synchronize()
            stream.synchronize()
        sr.same_answer(got, want, "device")
        sr.same_answer(got, host_answer, "host and device answers")       # ... are identical
        out = (np.full((33, k), 7, np.int64), np.full((33, k), 7, F), np.full(33, 7, np.int32))
        back = ix.search(Q, k, out=out)                                  # out= with host queries on the borrowed table
        assert back[0] is out[0] and back[1] is out[1] and back[2] is out[2]
        sr.same_answer(out, want, "out=")
        with torch.cuda.stream(stream):
            out_dev = (torch.empty((33, k), dtype=torch.int64, device="cuda"), torch.empty((33, k), dtype=torch.float32, device="cuda"),
                       torch.empty(33, dtype=torch.int32, device="cuda"))
            ix.search((q_off, q_idx, q_val), k, out=out_dev)
            ix.synchronize()
        sr.same_answer(out_dev, want, "device out=")
        ix.close()
        host.close()
        del Xd


# ---- 8. refusals
def test_refusals(ties):
    import torch
    from vectordb_amd import EpsillaError
    X, Q, D = ties
    n = 100
    good = head(X, n)
    want = sr.topk(D[sr.L2][:n], 10)
    ix = index(sr.L2, dim=sr.DIM_MAX - 1)   # (the ties table's largest index, 2^31 - 2, is then EQUAL to dim: used below)
    small = sr.csr([([1, 5, 9], [1, 2, 3]), ([], []), ([0, 7], [1, 1])])
    ix.attach_csr(*small)

    def refused(code, text, call, *a, **kw):
        with pytest.raises(EpsillaError) as e:
            call(*a, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    def bad_rows(rows):
        return sr.csr(rows)

    refused(30000, "row 1: indices must be strictly increasing", ix.attach_csr, *bad_rows([([1], [1]), ([5, 3], [1, 1]), ([2], [1])]))       # unsorted
    refused(30000, "row 2: indices must be strictly increasing", ix.attach_csr, *bad_rows([([1], [1]), ([3, 5], [1, 1]), ([2, 2], [1, 1])]))  # repeated
    refused(30000, "row 0: an index outside [0, dim)", ix.attach_csr, *bad_rows([([1, sr.DIM_MAX - 1], [1, 1]), ([3], [1])]))                # index == dim
    refused(30000, "row 1: an index outside [0, dim)", ix.attach_csr, *bad_rows([([1], [1]), ([-1, 3], [1, 1])]))                             # negative
    off, idx, val = small
    refused(30000, "row 1: offsets must be non-decreasing", ix.attach_csr, np.array([0, 3, 2, 5], np.int64), idx, val)
    refused(30000, "offsets[0] must be 0", ix.attach_csr, np.array([1, 3, 3, 5], np.int64), idx, val)
    # the same through device-resident arrays: the offsets are judged before anything indexes with them
    refused(30000, "row 1: offsets must be non-decreasing", ix.attach_csr, *dev((np.array([0, 3, -2 ** 40, 5], np.int64), idx, val)))
    refused(30000, "row 0: offsets must be non-decreasing", ix.attach_csr, *dev((np.array([0, 2 ** 40, 2 ** 40, 5], np.int64), idx, val)))
    refused(30000, "all be host or all be device", ix.attach_csr, off, torch.from_numpy(idx).cuda(), val)                                   # a mixed set
    assert ix.row_count == 3
    # after a refused attach the previous table still answers
    q = sr.csr([([1, 7], [1, 1])])
    ids, dist, counts = ix.search(q, 3)
    assert ids.tolist() == [[1, 2, 0]] and dist.tolist() == [[2.0, 2.0, 14.0]] and counts.tolist() == [3]
    # queries
    refused(30000, "query 1: indices must be strictly increasing", ix.search, sr.csr([([1], [1]), ([5, 3], [1, 1])]), 3)
    refused(30000, "query 0: an index outside [0, dim)", ix.search, sr.csr([([sr.DIM_MAX - 1], [1])]), 3)
    refused(30000, "query 1: offsets must be non-decreasing", ix.search, (np.array([0, 2, 1], np.int64), idx[:1], val[:1]), 3)
    refused(30000, "offsets[0] must be 0", ix.search, (np.array([1, 1], np.int64), idx[:1], val[:1]), 3)
    bad_q = sr.csr([([1], [1]), ([5, 3], [1, 1])])
    refused(30000, "query 1: indices must be strictly increasing", ix.search, (bad_q[0], *dev(bad_q[1:])), 3)                                  # device queries
    over = (np.array([0, 2, 2 + QMAX + 1], np.int64), np.arange(QMAX + 3, dtype=np.int32), np.ones(QMAX + 3, F))
    refused(50002, "query 1 has %d non-zeros; at most %d per query" % (QMAX + 1, QMAX), ix.search, over, 3)                                    # over the limit
    for k in (0, 1025):   # (past the wrapper: the library's own refusal)
        rc = ix.L.eps_sparse_index_search(ix.h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, 1, k, ids.ctypes.data, dist.ctypes.data, None)
        assert rc == 30000 and b"k must be in [1, 1024]" in ix.L.eps_sparse_index_last_error(ix.h)
    rc = ix.L.eps_sparse_index_search(ix.h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, 1, 3, ids.ctypes.data,
                                      torch.empty(3, dtype=torch.float32, device="cuda").data_ptr(), None)
    assert rc == 30000 and b"all be host or all be device" in ix.L.eps_sparse_index_last_error(ix.h)
    assert ix.L.eps_sparse_index_search(ix.h, None, None, None, 0, 3, None, None, None) == 0                                                  # nq = 0 touches nothing
    ix2 = index(sr.L2)
    ix2.attach_csr(*good)
    refused(30000, "bitset shorter", ix2.set_deleted, np.zeros(12, np.uint8))                                                                 # 100 rows: 13 bytes
    sr.same_answer(ix2.search(head(Q, 5), 10), (want[0][:5], want[1][:5], want[2][:5]))
    ix.close()
    ix2.close()


# ---- 9. stats
def test_stats(ties):
    X, Q, D = ties
    ix = index(sr.DOT)
    ix.attach_csr(*head(X, 1000))
    ix.search(head(Q, 9), 10)
    s = ix.stats()
    assert s["dist_evals"] == 1000 * 9 and s["main_kernel_rows"] == 1000 and s["main_kernel_queries"] == 9 and s["main_kernel_bits"] == 32
    assert s["main_kernel_launches"] == 1 and s["main_kernel_ms"] > 0 and s["kernel_ms"] >= s["main_kernel_ms"]
    assert all(s[f] == 0 for f in ("expansions", "rerank_rows", "overflow_queries", "filter_ms_all", "filter_rows_all", "i8_folded", "i8_declined", "one_pass",
                                   "i8_rotated"))
    ix.close()
