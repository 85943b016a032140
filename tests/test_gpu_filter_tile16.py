"""The 256-query row-id form of the 8-bit filter pass (mfma_filter_kernel_v7<2, FM_IDS, true>: 16 x 16 x 64 MFMAs, 16 row blocks x 4 query
blocks per wavefront, start values handed to the first MFMAs as their C operand) against tests/mirror_ref.py, through ONE launch each
(GpuIndex.filter_pass): counts exactly, lists as sets.  What test_gpu_mirror_pin.py does not pin by construction: every position of the
256 x 256 tile on its own, per-row start values at the threshold, the hit path past the pending list's capacity, and stage ranges whose
tiles do not fill the grid."""
import numpy as np
import pytest

import mirror_ref as mr

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


def grid_table(rng, n, d):
    """rows on the grid's 255 levels per column, independent signs"""
    return (rng.integers(-127, 128, (n, d)).astype(F) / F(127.0)).astype(F)


def open_view(amd, X, Q, metric=0):
    ix = amd.GpuIndex(X.shape[1], metric)
    ix.attach_rows(X)
    v = ix.mirror_view(8, Q)
    assert v["usable"] and v["version"] == 7
    return ix, v, mr.acc8(v)


def one_pass(ix, acc, Q, lo, hi, T, cap, what):
    T = np.asarray(T, np.int64)
    cnt, lists, Tu = ix.filter_pass(Q, 8, lo, hi, cap, T.astype(np.int32))
    assert np.array_equal(Tu, T.astype(np.int32))
    mr.check_pass(acc, lo, hi, T, cap, cnt, lists, what)
    return cnt, lists


@pytest.mark.parametrize("d", [512, 768])
def test_position_map(amd, d):
    """every query passes exactly one row - its own, planted - and over the batch the planted rows take every row % 256 and the queries every
    query % 256: a lane, register or block that reports under a wrong id shows as a wrong list"""
    rng = np.random.default_rng(d)
    n, nq = 3 * 256 + 77, 257
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    j = np.arange(nq)
    rows = (j % 256) + 256 * np.where(j % 256 < 77, j % 4, j % 3)
    rows[256] = 256 * 2            # (query 256 shares row % 256 = 0 with query 0: another tile)
    assert len(set(rows.tolist())) == nq and rows.max() < n
    assert set((rows % 256).tolist()) == set(range(256)) and set((j % 256).tolist()) == set(range(256))
    X[rows] = Q                    # L2: a query's nearest row is its own copy
    ix, v, acc = open_view(amd, X, Q)
    assert v["d_pad"] == d
    T = acc[rows, j]
    assert ((acc >= T[None, :]).sum(0) == 1).all(), "the planted rows are not the unique best ones: the case does not test what it says"
    cnt, lists = one_pass(ix, acc, Q, 0, n, T, 8, "position map d %d" % d)
    assert [l.tolist() for l in lists] == [[int(r)] for r in rows]
    ix.close()


def test_start_values_through_c(amd):
    """folded per-row start values (negative ones, a clamped row, rows at ACC_FORCE - one of them alone in the last tile) decide at the
    threshold: T = the m-th best accumulator reports every tie, T + 1 none of them.  129 queries: the second 128 are padding but one."""
    rng = np.random.default_rng(16)
    n, d, nq = 256 * 5 + 1, 768, 129
    X = rng.random((n, d), dtype=F)
    X[n // 3, 5] = F(30000.0)      # forced rows: the row constant leaves the accumulator's range
    X[n - 1, 9] = F(30000.0)
    X[n // 2, 7] = F(40.0)         # a clamped value: the row carries its own residual
    Q = rng.random((nq, d), dtype=F)
    ix, v, acc = open_view(amd, X, Q)
    start = mr.start8(v)
    assert v["fold"] == 1 and v["forced_rows"] == 2 and start[n // 3] == mr.ACC_FORCE and start[n - 1] == mr.ACC_FORCE
    assert (start < 0).any() and len(np.unique(start)) > n // 2, "the start values do not differ row by row"
    for m in (1, 17, 300):
        T = np.sort(acc, axis=0)[::-1][m - 1]
        one_pass(ix, acc, Q, 0, n, T, 1024, "start values, m %d" % m)
        one_pass(ix, acc, Q, 0, n, T + 1, 1024, "start values, m %d, T + 1" % m)
    ix.close()


def test_hit_path_under_load(amd):
    """one query passes all 256 rows of one tile, its neighbour in the same wavefront all four registers of one lane group in each of the
    16 row blocks of another; cap is below both counts: the wavefront's pending list overflows and entries take the direct path"""
    rng = np.random.default_rng(3)
    n, d, nq = 256 * 4 + 50, 512, 130
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    qa, qb = 5, 6
    rows_a = 256 + np.arange(256)
    rows_b = 256 * 2 + (16 * np.arange(16)[:, None] + 4 * 2 + np.arange(4)[None, :]).ravel()
    for rows, q in ((rows_a, qa), (rows_b, qb)):   # near copies of the query that differ from each other in one column each
        X[rows] = Q[q]
        X[rows, np.arange(len(rows)) % d] = F(0.0)
    ix, v, acc = open_view(amd, X, Q)
    T = np.sort(acc, axis=0)[::-1][0] + 1          # everyone else: nothing passes
    T[qa] = acc[rows_a, qa].min()
    T[qb] = acc[rows_b, qb].min()
    want = acc >= T[None, :]
    assert sorted(np.flatnonzero(want[:, qa]).tolist()) == rows_a.tolist() and sorted(np.flatnonzero(want[:, qb]).tolist()) == sorted(rows_b.tolist())
    cap = 40
    cnt, lists = one_pass(ix, acc, Q, 0, n, T, cap, "hit path under load")
    assert cnt[qa] == 256 and cnt[qb] == 64 and len(lists[qa]) == cap and len(lists[qb]) == cap
    one_pass(ix, acc, Q, 0, n, T, 256, "hit path under load, lists that fit")
    ix.close()


@pytest.mark.parametrize("tiles", [1, 8, 9])
def test_stage_edges(amd, tiles):
    """[lo, hi): lo a tile multiple, hi inside the last of `tiles` tiles (1 and 9: some XCDs get no tile, or one more than the others):
    nothing at or beyond hi is reported, whatever the threshold"""
    rng = np.random.default_rng(40 + tiles)
    n, d, nq = 256 * 12 + 5, 512, 200
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    ix, v, acc = open_view(amd, X, Q)
    lo = 256 * 2
    hi = lo + 256 * (tiles - 1) + 100
    T = np.sort(acc[lo:hi], axis=0)[::-1][16]
    one_pass(ix, acc, Q, lo, hi, T, 1024, "stage edges, %d tiles, m 17" % tiles)
    T = T.copy()
    T[::2] = -(1 << 30)            # every row of the range, no row outside it
    cnt, lists = one_pass(ix, acc, Q, lo, hi, T, hi - lo, "stage edges, %d tiles, open thresholds" % tiles)
    assert (cnt[::2] == hi - lo).all()
    ix.close()
