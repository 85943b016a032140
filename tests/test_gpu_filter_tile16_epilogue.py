"""The epilogue of the 16 x 16 x 64 filter tile (mfma_filter_kernel_v7<2, FM_IDS, true>, csrc/mfma_tile16.hpp): the common path's group maxima
and the hit path that walks only the groups of four row blocks whose maximum passes (the cases also hold for a common path whose maxima are
folded under the last K-step's MFMAs: every row block at the threshold, maxima that must not outlive their tile).  One GpuIndex.filter_pass launch per case against
tests/mirror_ref.py (counts exactly, lists as sets); rows and queries on the 255-level grid, so the integer accumulators are known exactly.
d = 512 (four K-steps, the smallest shape the kernel takes) but for one case.

A wavefront holds queries 64 w .. 64 w + 63 of the tile as four blocks j of 16 and the tile's 256 rows as sixteen blocks i of 16; lane l holds
query l % 16 of each block j and rows 4 (l / 16) .. + 3 of each block i in its four accumulator registers r.  Blocks 14 and 15 live in the
accumulator file; a group g is row blocks 4 g .. 4 g + 3."""
import numpy as np
import pytest

import mirror_ref as mr
from helpers import data

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


def open_view(amd, X, Q):
    ix = amd.GpuIndex(X.shape[1], 0)
    ix.attach_rows(X)
    v = ix.mirror_view(8, Q)
    assert v["usable"] and v["version"] == 7 and v["d_pad"] == X.shape[1]
    return ix, mr.acc8(v)


def one_pass(ix, acc, Q, lo, hi, T, cap, what):
    T = np.asarray(T, np.int64)
    cnt, lists, Tu = ix.filter_pass(Q, 8, lo, hi, cap, T.astype(np.int32))
    assert np.array_equal(Tu, T.astype(np.int32))
    mr.check_pass(acc, lo, hi, T, cap, cnt, lists, what)
    return cnt, lists


def closed(acc):
    """thresholds nothing passes: one above every query's largest accumulator"""
    return acc.max(axis=0) + 1


def plant(X, Q, q, rows):
    """near copies of query q (L2: its closest rows by far) that differ from each other in one column each"""
    rows = np.asarray(rows)
    X[rows] = Q[q]
    X[rows, (7 * np.arange(len(rows)) + 3) % X.shape[1]] = F(0.0)


# ------------------------------------------------------------------------------------------------ 1. the threshold's edge, row block by row block
def edge_query(i, j, r):
    return 64 * ((r + i) % 4) + 16 * j + i


def edge_row(i, j, r):
    return 256 * ((i + j) % 2) + 16 * i + 4 * j + r


@pytest.fixture(scope="module")
def edge_case(amd):
    """256 queries, each with its own copy among 2 x 256 rows: query (i, j, r) - row block i, query block j, register r, in lane group j - so that
    every row block sees all four query blocks and all four registers, and every wavefront every row block"""
    rng = np.random.default_rng(1716)
    n, d, nq = 2 * 256, 512, 256
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    ijr = [(i, j, r) for i in range(16) for j in range(4) for r in range(4)]
    qs = np.array([edge_query(*t) for t in ijr])
    rows = np.array([edge_row(*t) for t in ijr])
    assert sorted(qs.tolist()) == list(range(nq)) and len(set((rows % 256).tolist())) == 256
    X[rows] = Q[qs]
    ix, acc = open_view(amd, X, Q)
    own = np.empty(nq, np.int64)
    own[qs] = rows
    assert ((acc >= acc[own, np.arange(nq)][None, :]).sum(0) == 1).all(), "a query's copy is not its unique best row: the case does not test what it says"
    yield ix, acc, Q, n, own
    ix.close()


@pytest.mark.parametrize("i", range(16))
def test_threshold_edge_in_every_row_block(edge_case, i):
    """row block i (12 and 13: the last group's blocks in arch VGPRs; 14 and 15: the accumulator file): T = the planted row's accumulator lists it,
    T + 1 lists nothing - for the block's sixteen (query block, register) pairs at once, everything else closed"""
    ix, acc, Q, n, own = edge_case
    qs = np.array([edge_query(i, j, r) for j in range(4) for r in range(4)])
    T = closed(acc)
    T[qs] = acc[own[qs], qs]
    cnt, lists = one_pass(ix, acc, Q, 0, n, T, 8, "threshold edge, row block %d" % i)
    assert cnt.sum() == 16 and all(lists[q].tolist() == [int(own[q])] for q in qs)
    assert set(((own[qs] % 256) // 16).tolist()) == {i}
    T[qs] += 1
    cnt, lists = one_pass(ix, acc, Q, 0, n, T, 8, "threshold edge, row block %d, T + 1" % i)
    assert cnt.sum() == 0


# ------------------------------------------------------------------------------------------------ 2. a tile's maxima end with the tile
def test_maxima_do_not_carry_over(amd):
    """1024 queries: four query tiles, so 256 workgroups form 64 row groups and the first 64 row tiles are every workgroup's first tile; with
    3 x 64 + 1 tiles every workgroup walks at least three.  Each first tile holds one planted hit; the thresholds are one above the largest
    accumulator of every later tile, so nothing beyond the first tiles may be counted or listed"""
    rng = np.random.default_rng(1717)
    first = 64
    n, d, nq = 3 * first * 256 + 256, 512, 1024
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    t = np.arange(first)
    qs = (37 * t + 11) % nq
    rows = 256 * t + (29 * t + 7) % 256
    assert len(set(qs.tolist())) == first
    X[rows] = Q[qs]
    ix, acc = open_view(amd, X, Q)
    T = acc[first * 256:].max(axis=0) + 1
    assert (acc[rows, qs] >= T[qs]).all(), "a planted row does not pass"
    cnt, lists = one_pass(ix, acc, Q, 0, n, T, 64, "maxima do not carry over")
    assert (cnt[qs] >= 1).all() and all(int(r) in lists[q].tolist() for q, r in zip(qs, rows))
    assert all((l < first * 256).all() for l in lists)
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. the walk over groups that pass
def local(i, lg, r):
    """row within a tile: row block i, lane group lg, register r"""
    return 16 * i + 4 * lg + r


WALKS = {
    # name: [(query, [rows])] - one wavefront (queries 64 .. 127) but for the last
    "one group": [(64 + 5, [256 + local(i, i % 4, (i + 1) % 4) for i in (4, 5, 7)])],
    "two groups apart": [(64 + 21, [512 + local(1, 2, 3), 512 + local(3, 0, 0), 512 + local(9, 1, 2), 512 + local(10, 3, 1)])],
    "all four groups": [(64 + 38, [local(2, 1, 0), local(6, 3, 3), local(11, 0, 1), local(12, 2, 2), local(15, 1, 3)])],
    "last group": [(64 + 55, [768 + local(i, (i + 2) % 4, i % 4) for i in (12, 13, 14, 15)])],
    "one lane, two registers": [(64 + 9, [512 + local(14, 2, 0), 512 + local(14, 2, 2)])],
    "two query blocks of a wavefront": [(128 + 3, [768 + local(5, 1, 1)]), (128 + 32 + 12, [768 + local(13, 0, 2), 768 + local(0, 3, 3)])],
}


@pytest.fixture(scope="module")
def walk_case(amd):
    rng = np.random.default_rng(1718)
    n, d, nq = 4 * 256 + 50, 512, 256
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    for plan in WALKS.values():
        for q, rows in plan:
            plant(X, Q, q, rows)
    ix, acc = open_view(amd, X, Q)
    yield ix, acc, Q, n
    ix.close()


@pytest.mark.parametrize("name", list(WALKS))
def test_group_narrowed_walk(walk_case, name):
    ix, acc, Q, n = walk_case
    T = closed(acc)
    for q, rows in WALKS[name]:
        T[q] = acc[rows, q].min()
        assert sorted(np.flatnonzero(acc[:, q] >= T[q]).tolist()) == sorted(rows), "other rows pass as well: the case does not test what it says"
    cnt, lists = one_pass(ix, acc, Q, 0, n, T, 16, "walk: " + name)
    assert cnt.sum() == sum(len(rows) for _, rows in WALKS[name])
    for q, rows in WALKS[name]:
        assert sorted(lists[q].tolist()) == sorted(rows)


# ------------------------------------------------------------------------------------------------ 4. a stage that ends inside a tile
def test_stage_edge_inside_a_passing_tile(amd):
    """hi ends inside row block 6 of the third tile; the query's copies sit on both sides of it (the same row block, the next one, the tile's last
    one): those at or beyond hi pass the threshold and are never listed"""
    rng = np.random.default_rng(1719)
    n, d, nq = 4 * 256, 512, 256
    X = grid_table(rng, n, d)
    Q = grid_table(rng, nq, d)
    lo, hi, q = 256, 2 * 256 + 100, 192 + 16 + 7
    inside = [hi - 4, hi - 3, hi - 1, 256 + local(15, 3, 3)]
    beyond = [hi, hi + 1, hi + 3, 512 + local(7, 0, 2), 512 + local(15, 3, 3), 768 + local(6, 1, 0)]
    plant(X, Q, q, inside + beyond)
    ix, acc = open_view(amd, X, Q)
    T = closed(acc)
    T[q] = acc[inside + beyond, q].min()
    assert sorted(np.flatnonzero(acc[:, q] >= T[q]).tolist()) == sorted(inside + beyond)
    cnt, lists = one_pass(ix, acc, Q, lo, hi, T, 16, "stage edge inside a passing tile")
    assert cnt[q] == len(inside) and sorted(lists[q].tolist()) == sorted(inside) and cnt.sum() == len(inside)
    ix.close()


# ------------------------------------------------------------------------------------------------ 5. the whole chain
def test_whole_chain_returns_the_scan(amd):
    """one search through the staged chain (d = 768: six K-steps) against the fp32 stream engine: ids, distances and counts bit for bit"""
    n, d, nq, k = 40_000, 768, 256, 10
    X = data(n, d, 1720)
    Q = data(nq, d, 1721)
    ix = amd.GpuIndex(d, 0)
    ix.attach_rows(X)
    a = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_MFMA_I8)
    st = ix.stats()
    assert st["main_kernel_bits"] == 8 and st["one_pass"] == 0 and st["i8_declined"] == 0, st
    b = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    assert np.array_equal(a[0], b[0]), "%d ids differ" % (a[0] != b[0]).sum()
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    ix.close()
