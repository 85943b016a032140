"""GpuBinaryIndex on the device (eps_binary_index_*, csrc/binary.hip) against plain NumPy: Hamming distances of unpacked bits in int64, the expected
answer by a stable sort on (distance, row).  Ids, distances and counts are compared for equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW = int(re.search(r"constexpr int BIN_CW = (\d+);", open(os.path.join(ROOT, "vectordb_amd", "csrc", "binary_host.hpp")).read()).group(1))
EDGE = CW * 32   # bits of a chunk: the kernel's edge between whole chunks and the chunk of the last word
INT32_MAX = 2 ** 31 - 1


def unpack(words, dim):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[:, :dim]


def reference(rows, queries, dim, k, visible=None, base=0, stride=1):
    """(ids int64[nq, k], dist int32[nq, k], counts int32[nq]) of the k smallest (distance, row) keys over the visible rows"""
    R, Q = unpack(rows, dim), unpack(queries, dim)
    nq, n = len(Q), len(R)
    ids, dist, counts = np.full((nq, k), -1, np.int64), np.full((nq, k), INT32_MAX, np.int32), np.zeros(nq, np.int32)
    vis = np.arange(n) if visible is None else np.flatnonzero(visible)
    for j in range(nq):
        D = (R != Q[j]).sum(-1).astype(np.int64)
        order = vis[np.argsort(D[vis], kind="stable")][:k]   # (vis ascends: the stable sort breaks ties by row)
        c = len(order)
        ids[j, :c], dist[j, :c], counts[j] = order * stride + base, D[order], c
    return ids, dist, counts


def same(got, want):
    for g, w, what in zip(got, want, ("ids", "dist", "counts")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, np.argwhere(g != w)[:5])


def words(rng, m, dim):
    """m random vectors as uint32[m, W]: random garbage in the pad bits too"""
    return rng.integers(0, 2 ** 32, (m, (dim + 31) // 32), dtype=np.uint64).astype(np.uint32)


def index(dim):
    import vectordb_amd as amd
    return amd.GpuBinaryIndex(dim)


def bitset(hidden):
    return np.packbits(hidden, bitorder="little")


# every (NQ, KPL) form and each edge between forms, every dim around a word and around a chunk, one slice and several, k > n; the last shape has
# slices of 128 rows (k = 1024 caps the grid at 64 workgroups): two rounds per wavefront, and a last slice of one whole round and one of 38 rows
SHAPES = [(1, 1000, 5, 10), (31, 63, 1, 1), (32, 64, 4, 64), (33, 65, 33, 65), (33, 1000, 16, 10), (EDGE - 1, 1000, 32, 128), (EDGE, 1, 1, 10),
          (EDGE + 1, 1000, 33, 10), (EDGE + 1, 1000, 5, 256), (EDGE + 1, 1000, 4, 256), (EDGE - 1, 1000, 4, 512), (768, 1000, 32, 64),
          (768, 1000, 32, 65), (768, 1000, 5, 128), (768, 1000, 5, 1024), (768, 65, 4, 128), (768, 1000, 4, 1), (65536, 130, 5, 10),
          (EDGE + 1, 20070, 5, 1024)]


@pytest.mark.parametrize("dim,n,nq,k", SHAPES)
def test_shapes(dim, n, nq, k):
    rng = np.random.default_rng(dim * 7 + n + nq + k)
    X, Q = words(rng, n, dim), words(rng, nq, dim)
    if n > 20:
        X[n // 2], X[n - 1] = Q[0], Q[nq - 1]   # exact hits, one in the last row
        X[7] = Q[0] ^ np.uint32(1)              # ... and a row one bit away (dim = 1: the complement)
    ix = index(dim)
    ix.attach_rows(X)
    assert ix.row_count == n
    same(ix.search(Q, k), reference(X, Q, dim, k))
    s = ix.stats()
    assert (s["dist_evals"], s["main_kernel_rows"], s["main_kernel_queries"], s["main_kernel_bits"]) == (n * nq, n, nq, 1)
    assert s["main_kernel_launches"] == 1 and s["kernel_ms"] > 0 and s["main_kernel_ms"] > 0
    ix.close()


def test_rounds_under_a_bitset():
    """the grid at its cap, 8192 slices of 128 rows: two rounds per wavefront (the last slice: 64 rows and 10), a tile that is not full, a bitset"""
    rng = np.random.default_rng(40)
    dim, n, nq, k = 40, 600010, 5, 10
    X, Q, hidden = words(rng, n, dim), words(rng, nq, dim), rng.random(n) < 0.5
    X[n - 1], X[n - 70], hidden[[n - 1, n - 70]] = Q[0], Q[1], False   # exact hits in the last slice's second round and in its first
    ix = index(dim)
    ix.attach_rows(X)
    ix.set_deleted(bitset(hidden))
    same(ix.search(Q, k), reference(X, Q, dim, k, ~hidden))
    ix.close()


@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(8)
    return words(rng, 1000, 8), words(rng, 5, 8), rng.random(1000) < 0.5


@pytest.mark.parametrize("k", (10, 600))
@pytest.mark.parametrize("id_map", (None, (3, 8)))
def test_ties(ties, k, id_map):
    """dim = 8: at most 9 distinct distances, every list is decided by the id rule; half the rows hidden: k = 600 finds fewer than k"""
    X, Q, hidden = ties
    base, stride = id_map or (0, 1)
    ix = index(8)
    ix.attach_rows(X)
    if id_map:
        ix.set_id_map(base, stride)
    same(ix.search(Q, k), reference(X, Q, 8, k, None, base, stride))
    ix.set_deleted(bitset(hidden))
    got = ix.search(Q, k)
    same(got, reference(X, Q, 8, k, ~hidden, base, stride))
    assert k < 500 or (got[2] < k).all()
    ix.set_deleted(None)
    same(ix.search(Q, k), reference(X, Q, 8, k, None, base, stride))
    ix.attach_rows(X[:0])   # an empty table
    same(ix.search(Q, k), reference(X[:0], Q, 8, k))
    ix.close()


@pytest.mark.parametrize("dim,stride", ((768, 24), (768, 27), (768, 28), (70, 3), (70, 8)))
def test_buffers(dim, stride):
    """host words (copied) and borrowed device rows `stride` words apart - multiples of four words (16-byte loads) and not - give one answer; device
    queries give device results on a torch stream; out= buffers of both kinds"""
    import torch
    rng = np.random.default_rng(stride)
    n, nq, k, W = 333, 7, 20, (dim + 31) // 32
    X, Q = words(rng, n, dim), words(rng, nq, dim)
    want = reference(X, Q, dim, k)
    wide = rng.integers(0, 2 ** 32, (n, stride), dtype=np.uint64).astype(np.uint32)
    wide[:, :W] = X
    dX = torch.from_numpy(wide.view(np.int32)).cuda()[:, :W]
    dQ = torch.from_numpy(Q.view(np.int32)).cuda()
    ix = index(dim)
    with torch.cuda.stream(torch.cuda.Stream()):
        ix.use_torch_stream()
        ix.attach_rows(dX)
        got = ix.search(dQ, k)
        assert all(g.is_cuda for g in got)
        out = (torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.int32, device="cuda"),
               torch.empty(nq, dtype=torch.int32, device="cuda"))
        assert ix.search(dQ, k, out=out)[0] is out[0]
        ix.synchronize()
        same(got, want)
        same(out, want)
        same(ix.search(Q, k), want)   # host queries on the borrowed table
    ix.attach_rows(X)
    out = (np.empty((nq, k), np.int64), np.empty((nq, k), np.int32), np.empty(nq, np.int32))
    ix.search(Q, k, out=out)
    same(out, want)
    ix.close()


@pytest.mark.parametrize("dim", (1, 63, 64, 65, 100, 2049 + 33))   # (the last: 66 words, past the 64 words a wavefront packs per step)
def test_signs(dim):
    import torch
    rng = np.random.default_rng(dim)
    n = 70
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 1.0, -1.0], np.float32)
    x = special[rng.integers(0, len(special), (n, dim))]
    want = np.zeros((n, (dim + 31) // 32 * 32), np.uint8)
    want[:, :dim] = x > 0
    want = np.packbits(want, axis=-1, bitorder="little").view(np.uint32)
    ix = index(dim)
    assert np.array_equal(ix.pack_signs(x), want)
    dx = torch.from_numpy(x).cuda()
    packed = ix.pack_signs(dx)
    ix.synchronize()
    assert packed.is_cuda and np.array_equal(packed.cpu().numpy().view(np.uint32), want)
    Q = words(rng, 3, dim)
    for rows in (x, dx):   # the owned table of attach_signs is the packed table
        ix.attach_signs(rows)
        assert ix.row_count == n
        same(ix.search(Q, 5), reference(want, Q, dim, 5))
    ix.close()


def test_the_dense_engine_agrees():
    """the route a caller had: +-1 floats in an EUCLIDEAN flat search - the same ids, distances 4 x Hamming exactly"""
    import vectordb_amd as amd
    rng = np.random.default_rng(96)
    n, dim, nq, k = 1000, 96, 5, 10
    X, Q = words(rng, n, dim), words(rng, nq, dim)
    ix = index(dim)
    ix.attach_rows(X)
    ids, dist, counts = ix.search(Q, k)
    dense = amd.GpuIndex(dim, "EUCLIDEAN")
    dense.attach_rows(unpack(X, dim).astype(np.float32) * 2 - 1)
    d_ids, d_dist, d_counts = dense.search(unpack(Q, dim).astype(np.float32) * 2 - 1, k, mode=amd.MODE_FLAT)
    assert np.array_equal(d_ids, ids) and np.array_equal(d_dist, 4.0 * dist) and np.array_equal(d_counts, counts)
    dense.close()
    ix.close()


def test_refusals():
    from vectordb_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    for dim in (0, 65537):
        assert L.eps_binary_index_create(dim, 0, C.byref(h)) == _lib.EPS_USER_ERROR and not h.value
    rng = np.random.default_rng(1)
    X, Q = words(rng, 100, 40), words(rng, 2, 40)
    ix = index(40)
    ix.attach_rows(X)
    want = reference(X, Q, 40, 3)
    ids, dist, counts = np.empty((2, 3), np.int64), np.empty((2, 3), np.int32), np.empty(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, text):
        assert rc == _lib.EPS_USER_ERROR and text in L.eps_binary_index_last_error(ix.h).decode()
        same(ix.search(Q, 3), want)   # the handle goes on answering

    refused(L.eps_binary_index_search(ix.h, p(Q), 2, 0, p(ids), p(dist), p(counts)), "k must be")
    refused(L.eps_binary_index_search(ix.h, p(Q), 2, 1025, p(ids), p(dist), p(counts)), "k must be")
    refused(L.eps_binary_index_search(ix.h, None, 2, 3, p(ids), p(dist), p(counts)), "null buffer")
    refused(L.eps_binary_index_search(ix.h, p(Q), 2, 3, None, p(dist), p(counts)), "null buffer")
    refused(L.eps_binary_index_search(ix.h, p(Q), 2, 3, p(ids), None, p(counts)), "null buffer")
    refused(L.eps_binary_index_attach_rows(ix.h, None, 5, 2), "null buffer")
    refused(L.eps_binary_index_attach_rows(ix.h, p(X), 100, 1), "stride_words")
    refused(L.eps_binary_index_set_deleted(ix.h, p(np.zeros(12, np.uint8)), 12), "shorter")
    refused(L.eps_binary_index_set_id_map(ix.h, 0, 0), "stride must be positive")
    import torch
    d_ids = torch.empty((2, 3), dtype=torch.int64, device="cuda")
    refused(L.eps_binary_index_search(ix.h, p(Q), 2, 3, C.c_void_p(d_ids.data_ptr()), p(dist), p(counts)), "all be host or all be device")
    refused(L.eps_binary_index_pack_signs(ix.h, p(np.zeros((1, 40), np.float32)), 1, C.c_void_p(d_ids.data_ptr())), "both be host or both be device")
    assert L.eps_binary_index_search(ix.h, None, 0, 3, None, None, None) == 0   # nq = 0
    assert L.eps_binary_index_search(None, p(Q), 2, 3, p(ids), p(dist), p(counts)) == _lib.EPS_USER_ERROR
    ix.close()
