"""GpuByteIndex (csrc/byte.hip) against plain NumPy on int64, a stable sort on (distance, row); ids, distances and counts compared for equality."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
KINDS = [("EUCLIDEAN", False), ("DOT_PRODUCT", False), ("EUCLIDEAN", True), ("DOT_PRODUCT", True)]


def reference(rows, queries, metric, k, visible=None, base=0, stride=1):
    """(ids int64[nq, k], dist int32[nq, k], counts int32[nq]) of the k smallest (distance, row) keys over the visible rows"""
    R, Q = rows.astype(np.int64), queries.astype(np.int64)
    nq, n = len(Q), len(R)
    D = -(Q @ R.T)
    if metric == "EUCLIDEAN":
        D = (Q * Q).sum(-1)[:, None] + (R * R).sum(-1)[None, :] + 2 * D   # sum (x - q)^2, exact in int64
    ids, dist, counts = np.full((nq, k), -1, np.int64), np.full((nq, k), INT32_MAX, np.int32), np.zeros(nq, np.int32)
    vis = np.arange(n) if visible is None else np.flatnonzero(visible)
    for j in range(nq):
        order = vis[np.argsort(D[j, vis], kind="stable")][:k]   # (vis ascends: the stable sort breaks ties by row)
        c = len(order)
        ids[j, :c], dist[j, :c], counts[j] = order * stride + base, D[j, order], c
    return ids, dist, counts


def same(got, want):
    for g, w, what in zip(got, want, ("ids", "dist", "counts")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, np.argwhere(g != w)[:5])


def full_range(rng, m, dim, unsigned):
    return rng.integers(0, 256, (m, dim)).astype(np.uint8) if unsigned else rng.integers(-128, 128, (m, dim)).astype(np.int8)


def index(dim, metric, unsigned):
    import vectordb_amd as amd
    return amd.GpuByteIndex(dim, metric, unsigned)


def form(dim, nq, k):
    """(live columns, KPL) the plan must choose: 32 columns need k <= 64, more than 16 queries and 32 padded rows within 64 KB of LDS"""
    kpl = 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16
    return (32 if kpl == 1 and nq > 16 and (dim + 63) // 64 * 64 <= 2048 else min(16, 64 // kpl)), kpl


# dim around a K-step, one and many K-steps, the LDS rule at 2048 | 2049; n around a 16-row block and a round; nq around a column block and many
# tiles; k at every edge between forms.  (64, 20000, k = 1024): the merge cap leaves 256 slices of 128 rows, two rounds per wavefront
SHAPES = [(1, 1000, 1, 10), (63, 1, 15, 1), (64, 15, 16, 64), (65, 17, 17, 65), (100, 63, 33, 128), (768, 65, 5, 129), (2048, 1000, 33, 10),
          (2049, 1000, 33, 10), (4096, 1000, 17, 256), (100, 1000, 1100, 10), (768, 1000, 9, 257), (768, 1000, 5, 1024), (768, 1000, 33, 64),
          (64, 20000, 5, 1024), (192, 60000, 3, 1024)]   # (the last: four rounds per wavefront of three K-steps each)


@pytest.mark.parametrize("case", range(len(SHAPES)))
@pytest.mark.parametrize("pair", (0, 1))
def test_shapes(case, pair):
    """full-range bytes; every shape under two of the four (metric, signedness) kinds, so that every kind meets every other shape"""
    dim, n, nq, k = SHAPES[case]
    metric, unsigned = KINDS[(case + pair * (1 + case // 4 % 3)) % 4]
    rng = np.random.default_rng(dim * 7 + n + nq + k)
    X, Q = full_range(rng, n, dim, unsigned), full_range(rng, nq, dim, unsigned)
    if n > 20:
        X[n // 2], X[n - 1] = Q[0], Q[nq - 1]   # exact hits, one in the last row
    ix = index(dim, metric, unsigned)
    ix.attach_rows(X)
    assert ix.row_count == n
    same(ix.search(Q, k), reference(X, Q, metric, k))
    s = ix.stats()
    assert (s["live_columns"], s["kpl"]) == form(dim, nq, k)
    assert (s["dist_evals"], s["main_kernel_rows"], s["main_kernel_queries"], s["main_kernel_bits"]) == (n * nq, n, nq, 8)
    assert s["main_kernel_launches"] == 1 and s["kernel_ms"] > 0 and 0 < s["hit_rounds"] <= s["rounds"]
    ix.close()


def test_rounds_under_a_bitset(metric="EUCLIDEAN", unsigned=True):
    """the grid at its cap, 8192 slices of 128 rows, two rounds per wavefront, the last slice ragged; half the rows hidden.  49 rows of 50 are one
    vector: a slice's second round of nothing else only ties with the k-th distance, so the common path must end it at the vote"""
    rng = np.random.default_rng(40)
    dim, n, nq, k = 64, 600010, 5, 10
    X, Q = np.repeat(full_range(rng, 1, dim, unsigned), n, 0), full_range(rng, nq, dim, unsigned)
    other = rng.random(n) < 0.02
    X[other] = full_range(rng, int(other.sum()), dim, unsigned)
    X[1], X[n - 1], X[n - 70] = Q[0], Q[0], Q[1]   # exact hits in the first slice, in the last slice's second round and in its first
    hidden = rng.random(n) < 0.5
    hidden[[n - 1, n - 70]] = False
    ix = index(dim, metric, unsigned)
    ix.attach_rows(X)
    ix.set_deleted(np.packbits(hidden, bitorder="little"))
    same(ix.search(Q, k), reference(X, Q, metric, k, ~hidden))
    s = ix.stats()
    assert s["rounds"] == (n + 63) // 64 and 0 < s["hit_rounds"] < s["rounds"]
    ix.close()


@pytest.mark.parametrize("metric", ("EUCLIDEAN", "DOT_PRODUCT"))
@pytest.mark.parametrize("values", ("extreme_signed", "extreme_unsigned", "ties"))
@pytest.mark.parametrize("dim", (100, 4096))
def test_values(metric, values, dim):
    """all -128 against all 127, all 255 against all 255: the largest distances of either sign; values in {-1, 0, 1}: the row order decides"""
    rng = np.random.default_rng(dim)
    n, nq, k = 300, 3, 70
    unsigned = values == "extreme_unsigned"
    if values == "ties":
        X, Q = rng.integers(-1, 2, (n, dim)).astype(np.int8), rng.integers(-1, 2, (nq, dim)).astype(np.int8)
        X[:, 2:], Q[:, 2:] = 0, 0   # nine distinct rows
    elif unsigned:
        X, Q = np.full((n, dim), 255, np.uint8), np.full((nq, dim), 255, np.uint8)
        X[::3], Q[1] = 0, 0
    else:
        X, Q = np.full((n, dim), -128, np.int8), np.full((nq, dim), 127, np.int8)
        X[::3], Q[1] = 127, -128
    ix = index(dim, metric, unsigned)
    ix.attach_rows(X)
    same(ix.search(Q, k), reference(X, Q, metric, k))
    ix.close()


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(8)
    return full_range(rng, 1000, 100, False), full_range(rng, 7, 100, False), rng.random(1000) < 0.9


@pytest.mark.parametrize("k", (10, 600))
@pytest.mark.parametrize("id_map", (None, (3, 8)))
def test_bitset_id_map_and_a_second_table(table, k, id_map):
    """a bitset that hides most of the table (k = 600 finds fewer than k), an id map, the bitset forgotten with the table, an empty table"""
    X, Q, hidden = table
    base, stride = id_map or (0, 1)
    ix = index(100, "EUCLIDEAN", False)
    ix.attach_rows(X)
    if id_map:
        ix.set_id_map(base, stride)
    ix.set_deleted(np.packbits(hidden, bitorder="little"))
    got = ix.search(Q, k)
    same(got, reference(X, Q, "EUCLIDEAN", k, ~hidden, base, stride))
    assert k < 500 or (got[2] < k).all()
    Y = X[::-1][:333]
    ix.attach_rows(Y)   # a second table replaces the first and its bitset
    assert ix.row_count == 333
    same(ix.search(Q, k), reference(Y, Q, "EUCLIDEAN", k, None, base, stride))
    ix.attach_rows(X[:0])
    same(ix.search(Q, k), reference(X[:0], Q, "EUCLIDEAN", k))
    ix.close()


@pytest.mark.parametrize("dim,stride,unsigned", ((768, 768, False), (100, 117, True), (70, 128, False)))
def test_buffers(dim, stride, unsigned):
    """host bytes and device rows `stride` bytes apart give one answer; device queries give device results on a torch stream"""
    import torch
    rng = np.random.default_rng(stride)
    n, nq, k = 333, 7, 20
    X, Q = full_range(rng, n, dim, unsigned), full_range(rng, nq, dim, unsigned)
    want = reference(X, Q, "DOT_PRODUCT", k)
    wide = full_range(rng, n, stride, unsigned)
    wide[:, :dim] = X
    dX, dQ = torch.from_numpy(wide).cuda()[:, :dim], torch.from_numpy(Q).cuda()
    ix = index(dim, "DOT_PRODUCT", unsigned)
    with torch.cuda.stream(torch.cuda.Stream()):
        ix.use_torch_stream()
        ix.attach_rows(dX)
        got = ix.search(dQ, k)
        assert all(g.is_cuda for g in got)
        ix.synchronize()
        same(got, want)
        same(ix.search(Q, k), want)   # host queries on the table that came from the device
    ix.attach_rows(X)
    same(ix.search(Q, k), want)
    ix.close()


def test_refusals():
    from vectordb_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    for dim, metric in ((0, 0), (4097, 0), (64, 1), (64, 7)):   # (metric 1: COSINE)
        assert L.eps_byte_index_create(dim, metric, 0, 0, C.byref(h)) == _lib.EPS_USER_ERROR and not h.value
    rng = np.random.default_rng(1)
    X, Q = full_range(rng, 100, 40, False), full_range(rng, 2, 40, False)
    ix = index(40, "EUCLIDEAN", False)
    ix.attach_rows(X)
    want = reference(X, Q, "EUCLIDEAN", 3)
    ids, dist, counts = np.empty((2, 3), np.int64), np.empty((2, 3), np.int32), np.empty(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, text):
        assert rc == _lib.EPS_USER_ERROR and text in L.eps_byte_index_last_error(ix.h).decode()
        same(ix.search(Q, 3), want)   # the handle goes on answering

    refused(L.eps_byte_index_search(ix.h, p(Q), 2, 0, p(ids), p(dist), p(counts)), "k must be")
    refused(L.eps_byte_index_search(ix.h, p(Q), 2, 1025, p(ids), p(dist), p(counts)), "k must be")
    for bufs in ((None, p(ids), p(dist)), (p(Q), None, p(dist)), (p(Q), p(ids), None)):
        refused(L.eps_byte_index_search(ix.h, bufs[0], 2, 3, bufs[1], bufs[2], p(counts)), "null buffer")
    refused(L.eps_byte_index_attach_rows(ix.h, None, 5, 40), "null buffer")
    refused(L.eps_byte_index_attach_rows(ix.h, p(X), 100, 39), "stride")
    refused(L.eps_byte_index_set_deleted(ix.h, p(np.zeros(12, np.uint8)), 12), "shorter")
    refused(L.eps_byte_index_set_id_map(ix.h, 0, 0), "stride must be positive")
    import torch
    d_ids = torch.empty((2, 3), dtype=torch.int64, device="cuda")
    refused(L.eps_byte_index_search(ix.h, p(Q), 2, 3, C.c_void_p(d_ids.data_ptr()), p(dist), p(counts)), "all be host or all be device")
    assert L.eps_byte_index_search(ix.h, None, 0, 3, None, None, None) == 0   # nq = 0
    assert L.eps_byte_index_search(None, p(Q), 2, 3, p(ids), p(dist), p(counts)) == _lib.EPS_USER_ERROR
    ix.close()
