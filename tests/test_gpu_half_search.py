"""GpuHalfIndex (csrc/half.hip) against NumPy fp64 through exact_ref: tables of ties bit for bit (check_exact), continuous tables within the
order-free bound  B = gamma'(d + 4) mag,  gamma'(m) = m u' / (1 - m u'),  u' = 2^-23 - twice the unit roundoff, so that it holds whether the
matrix cores' internal adds round to nearest or truncate - stated before any device is asked (check_topk)."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as xr

pytestmark = pytest.mark.gpu

METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
DTYPES = ("float16", "bfloat16")
U2 = 2.0 ** -23


def to_half(a, dtype):
    """float32 -> the host form of a half array, rounded to nearest even: np.float16, or np.uint16 bf16 patterns (through torch on the CPU)"""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16)
    import torch
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def widen(h, dtype):
    return h.astype(np.float32) if dtype == "float16" else (h.astype(np.uint32) << 16).view(np.float32)


def index(dim, metric, dtype):
    import vectordb_amd as amd
    return amd.GpuHalfIndex(dim, METRIC[metric], dtype)


def form(dim, nq, k):
    kpl = 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16
    d_pad = (dim + 31) // 32 * 32
    nb = min(4 if k <= 64 else 2 if k <= 128 else 1, 4 if d_pad <= 1024 else 2 if d_pad <= 2048 else 1, 4 if nq > 32 else 2 if nq > 16 else 1)
    return min(16 * nb, 64 // kpl), kpl


def ties(rng, n, dim, metric, dtype):
    s = np.float32(1 / 16 if metric == 1 else 1)
    return to_half(rng.integers(-8, 9, (n, dim)).astype(np.float32) * s, dtype)


def np_(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def exact(ix, X, Q, metric, dtype, k, visible=None, id_map=(0, 1), what=""):
    ids, dist, cnt = (np_(a) for a in ix.search(Q, k))
    rows = np.where(ids >= 0, (ids - id_map[0]) // id_map[1], -1)
    assert ((ids < 0) | ((ids - id_map[0]) % id_map[1] == 0)).all()
    xr.check_exact(rows, dist, cnt, widen(X, dtype), widen(Q, dtype), metric, k, visible, what=what)


DIMS, NS, NQS, KS = (1, 31, 32, 33, 1024, 1056, 2048, 2080, 4096), (1, 63, 64, 65, 257), (1, 15, 17, 64, 65), (64, 65, 128, 129, 256, 257, 512, 513, 1024)
# every dim, n, nq and (metric, dtype) pair; then every k edge on a table that fills the lists, 70 queries (two tiles at k <= 64)
SHAPES = [(DIMS[i % 9], NS[i % 5], NQS[(2 * i) % 5], 10, i % 3, DTYPES[(i // 3) % 2]) for i in range(18)] + \
         [(72, 1500, 70, k, j % 3, DTYPES[j % 2]) for j, k in enumerate(KS)]


@pytest.mark.parametrize("dim,n,nq,k,metric,dtype", SHAPES)
def test_ties(dim, n, nq, k, metric, dtype):
    rng = np.random.default_rng([dim, n, nq, k])
    X, Q = ties(rng, n, dim, metric, dtype), ties(rng, nq, dim, metric, dtype)
    ix = index(dim, metric, dtype)
    ix.attach_rows(X)
    assert ix.row_count == n
    exact(ix, X, Q, metric, dtype, k)
    s = ix.stats()
    assert (s["live_columns"], s["kpl"]) == form(dim, nq, k) and not s["seeded"] and s["main_kernel_bits"] == 16
    assert s["rounds"] == (n + 63) // 64 * -(-nq // s["live_columns"]) and 0 < s["hit_rounds"] <= s["rounds"] and s["kernel_ms"] > 0
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitset_id_map_second_table_and_buffers(dtype):
    """a bitset with a whole round hidden and fewer than k rows visible, an id map, a second table that forgets the bitset, strided device rows,
    device queries on a torch stream, attach_floats"""
    import torch
    rng = np.random.default_rng(3)
    dim, n, nq, metric = 40, 300, 7, 0
    X, Q = ties(rng, n, dim, metric, dtype), ties(rng, nq, dim, metric, dtype)
    hidden = rng.random(n) < 0.5
    hidden[64:128] = True
    ix = index(dim, metric, dtype)
    ix.attach_rows(X)
    ix.set_id_map(3, 8)
    ix.set_deleted(np.packbits(hidden, bitorder="little"))
    for k in (10, 200):
        exact(ix, X, Q, metric, dtype, k, ~hidden, (3, 8))
    ix.attach_rows(X[::-1][:130])
    exact(ix, X[::-1][:130], Q, metric, dtype, 10, None, (3, 8))
    ix.set_id_map(0, 1)
    tdt = getattr(torch, dtype)
    as_dev = lambda h: torch.from_numpy(h.view(np.int16)).cuda().view(tdt)
    wide = np.concatenate([X, ties(rng, n, 13, metric, dtype)], axis=1)
    with torch.cuda.stream(torch.cuda.Stream()):
        ix.use_torch_stream()
        ix.attach_rows(as_dev(wide)[:, :dim])
        got = ix.search(as_dev(Q), 10)
        assert all(g.is_cuda for g in got)
        ix.synchronize()
        xr.check_exact(*(np_(g) for g in got), widen(X, dtype), widen(Q, dtype), metric, 10)
    ix.attach_floats(widen(X, dtype))
    exact(ix, X, Q, metric, dtype, 10)
    ix.attach_floats(torch.from_numpy(widen(X, dtype)).cuda())
    exact(ix, X, Q, metric, dtype, 10)
    ix.attach_rows(X[:0])
    exact(ix, X[:0], Q, metric, dtype, 10)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_floats_rounds_to_nearest_even(dtype):
    """against NumPy's (bf16: torch's CPU) rounding bit for bit: halfway cases both ways, overflow to infinity, results below the normal range,
    NaN stays NaN"""
    import torch
    rng = np.random.default_rng(5)
    step = 2.0 ** -10 if dtype == "float16" else 2.0 ** -7
    base = 1 + step * np.arange(8)
    special = np.concatenate([base + step / 2, base + step / 2 + 2.0 ** -20, -(base + step / 2), [65504, 65519.9, 65520, 70000, -1e30, 3.3e38, 3.4e38, np.inf, -np.inf, 0.0, -0.0,
                              np.nan, 2.0 ** -14, 2.0 ** -15 * 1.0005, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.01, 1e-40]]).astype(np.float32)
    x = np.concatenate([special, rng.standard_normal(600 - len(special)).astype(np.float32) * 100]).reshape(15, 40)
    want = to_half(x, dtype)
    ix = index(40, 0, dtype)
    got_host, got_dev = ix.convert_floats(x), ix.convert_floats(torch.from_numpy(x).cuda())
    ix.synchronize()
    assert got_host.dtype == want.dtype and got_dev.dtype == getattr(torch, dtype)
    for got in (got_host.view(np.uint16), got_dev.view(torch.int16).cpu().numpy().view(np.uint16)):
        nan = np.isnan(x)
        assert np.array_equal(got[~nan], want.view(np.uint16)[~nan]) and np.isnan(widen(got.view(want.dtype), dtype)[nan]).all() and nan.sum() == 1
    ix.close()


@pytest.mark.parametrize("metric", (0, 2))
def test_nan_and_infinite_rows_order_as_in_the_flat_search(metric, dtype="float16"):
    rng = np.random.default_rng(9)
    n, dim, nq = 100, 40, 3
    X, Q = ties(rng, n, dim, metric, dtype), ties(rng, nq, dim, metric, dtype)
    Q[:, 3] = 2
    X[5, 7] = np.nan
    if metric == 2:
        X[9, 3], X[11, 3] = np.inf, -np.inf   # -x.q: -inf and +inf
    ix = index(dim, metric, dtype)
    ix.attach_rows(X)
    ids, dist, cnt = ix.search(Q, n)
    d64 = xr.dist64(widen(X, dtype), widen(Q, dtype), metric)
    for q in range(nq):
        fin = np.flatnonzero(np.isfinite(d64[:, q]))
        want = ([9] if metric == 2 else []) + list(fin[np.lexsort((fin, d64[fin, q]))]) + ([11] if metric == 2 else []) + [5]
        assert cnt[q] == n and list(ids[q]) == want and np.isnan(dist[q, -1]) and np.array_equal(dist[q, :-1].astype(np.float64), d64[want[:-1], q])
    ix.close()


@pytest.mark.parametrize("n,visible_in_prefix,seeded", ((32767, None, False), (40000, 5, True), (40000, 400, True), (40000, None, True)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_side_of_the_seed_rule(n, visible_in_prefix, seeded, dtype):
    """tables of ties on each side of half_seed_rows; the seeded one also under a bitset that hides most of the prefix - 5 visible rows of it: no
    k-th distance, the seed is open; 400: a loose one"""
    rng = np.random.default_rng(n)
    dim, nq, k, metric = 40, 20, 10, 2 * (n % 2)
    X, Q = ties(rng, n, dim, metric, dtype), ties(rng, nq, dim, metric, dtype)
    ix = index(dim, metric, dtype)
    ix.attach_rows(X)
    visible = None
    if visible_in_prefix:
        visible = rng.random(n) < 0.7
        visible[:4096] = False
        visible[rng.choice(4096, visible_in_prefix, replace=False)] = True
        ix.set_deleted(np.packbits(~visible, bitorder="little"))
    exact(ix, X, Q, metric, dtype, k, visible)
    s = ix.stats()
    assert s["seeded"] == seeded and s["seed_rows"] == (4096 if seeded else 0) and s["dist_evals"] == (n + s["seed_rows"]) * nq
    assert 0 < s["hit_rounds"] <= s["rounds"] and (s["seed_hit_rounds"] > 0) == seeded
    ix.close()


TABLES = {"uniform": lambda r, n, d: r.random((n, d), dtype=np.float32), "normal": lambda r, n, d: r.standard_normal((n, d), dtype=np.float32),
          "unit normal": lambda r, n, d: xr.unit(r.standard_normal((n, d), dtype=np.float32))}


def half_ref(X, Q, metric):
    """exact_ref.Ref whose bound("free") is B: gamma'(d + 4) mag, EUCLIDEAN mag = sum x^2 + sum q^2 + 2 sum |x q| (the cancelling form does not earn
    the term-by-term bound), COSINE + u' (|d64| + B) for the subtraction.  Ref.bound multiplies mag by gamma(d + 3) (and adds u (|d64| + e) for
    COSINE), so mag is set to what makes that product B"""
    ref = xr.Ref(X, Q, metric)
    m = ref.d + 4
    mag = xr.mag64(X, Q, 2)
    if metric == 0:
        X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
        mag = (X64 * X64).sum(1)[:, None] + (Q64 * Q64).sum(1)[None, :] + 2 * mag
    B = m * U2 / (1 - m * U2) * mag
    if metric == 1:
        B = B + U2 * (np.abs(ref.d64) + B)
        B = (B - xr.U * np.abs(ref.d64)) / (1 + xr.U)
    ref.mag = B / xr.gamma(xr.free_terms(ref.d))
    return ref


@pytest.mark.parametrize("d", (40, 72, 136))
@pytest.mark.parametrize("n", (3000, 40000))
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_continuous_tables(dtype, table, n, d):
    rng = np.random.default_rng([7, n, d])
    X, Q = to_half(TABLES[table](rng, n, d), dtype), to_half(TABLES[table](rng, 20, d), dtype)
    Xw, Qw = widen(X, dtype), widen(Q, dtype)
    for metric in (0, 1, 2):
        ref = half_ref(Xw, Qw, metric)
        for k in (10, 100):
            xr.assert_cap(ref, k, what="%s %s" % (table, METRIC[metric]))   # from the reference alone, before the device runs
        ix = index(d, metric, dtype)
        ix.attach_rows(X)
        for k in (10, 100):
            ids, dist, cnt = ix.search(Q, k)
            und = xr.check_topk(ids, dist, cnt, Xw, Qw, metric, k, ref=ref, what="%s %s k %d" % (table, METRIC[metric], k))
            assert und <= xr.CAP * k * 20 and ix.stats()["seeded"] == (n >= 32768)
            print("half error ratio %s %s n %d d %d %s k %d: %.4f of B" % (dtype, table, n, d, METRIC[metric], k, xr.error_ratios(ids, dist, cnt, ref)[0]))
        ix.close()


def test_refusals(dtype="float16"):
    from vectordb_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    for dim, metric in ((0, 0), (4097, 0), (64, 3), (64, -1)):
        assert L.eps_half_index_create(dim, metric, 0, 0, C.byref(h)) == _lib.EPS_USER_ERROR and not h.value
    rng = np.random.default_rng(1)
    X, Q = ties(rng, 100, 40, 0, dtype), ties(rng, 2, 40, 0, dtype)
    ix = index(40, 0, dtype)
    ix.attach_rows(X)
    ids, dist, counts, f = np.empty((2, 3), np.int64), np.empty((2, 3), np.float32), np.empty(2, np.int32), np.zeros((2, 40), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, text):
        assert rc == _lib.EPS_USER_ERROR and text in L.eps_half_index_last_error(ix.h).decode()
        exact(ix, X, Q, 0, dtype, 3)   # the handle goes on answering

    refused(L.eps_half_index_search(ix.h, p(Q), 2, 0, p(ids), p(dist), p(counts)), "k must be")
    refused(L.eps_half_index_search(ix.h, p(Q), 2, 1025, p(ids), p(dist), p(counts)), "k must be")
    for bufs in ((None, p(ids), p(dist)), (p(Q), None, p(dist)), (p(Q), p(ids), None)):
        refused(L.eps_half_index_search(ix.h, bufs[0], 2, 3, bufs[1], bufs[2], p(counts)), "null buffer")
    refused(L.eps_half_index_attach_rows(ix.h, None, 5, 40), "null buffer")
    refused(L.eps_half_index_attach_rows(ix.h, p(X), 100, 39), "stride")
    refused(L.eps_half_index_set_deleted(ix.h, p(np.zeros(12, np.uint8)), 12), "shorter")
    refused(L.eps_half_index_set_id_map(ix.h, 0, 0), "stride must be positive")
    import torch
    d_ids = torch.empty((2, 3), dtype=torch.int64, device="cuda")
    refused(L.eps_half_index_search(ix.h, p(Q), 2, 3, C.c_void_p(d_ids.data_ptr()), p(dist), p(counts)), "all be host or all be device")
    refused(L.eps_half_index_convert_floats(ix.h, p(f), 2, C.c_void_p(d_ids.data_ptr())), "both be host or both be device")
    assert L.eps_half_index_search(ix.h, None, 0, 3, None, None, None) == 0   # nq = 0
    assert L.eps_half_index_search(None, p(Q), 2, 3, p(ids), p(dist), p(counts)) == _lib.EPS_USER_ERROR
    ix.close()
