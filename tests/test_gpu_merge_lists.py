"""Radius search and ordered select across shards on the MI355X: merge_rank_kernel (csrc/merge_lists.hip) behind eps_merge_range,
eps_merge_range_packed, eps_merge_select and eps_exchange_allgather_merge_range, and the helpers search_range_shards / select_shards.

1 synthetic lists with planted ties against tests/merge_ref.py (checked on the CPU in tests/test_merge_ref_cpu.py), over every form of the launch:
  the staged one with several queries per workgroup, with one, the one that searches global memory, and more queries than a grid's y extent;
2, 3 G single-device indices over the rows i mod G of a table against ONE index over the whole table: search_range on every engine, select;
4 the exchange step on a communicator of one rank;  5 refusals.
Every comparison is equality of integers and of float bit patterns: no tolerance appears."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as er
import merge_ref as mr
import range_ref as rr
import select_ref as sr
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
ENGINES = ("stream", "mfma", "mfma_i8")
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
GS = (1, 2, 3, 16)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poisoned(nq, cap, device=False):
    out = (np.full((nq, cap), -7, np.int64), np.full((nq, cap), -7, F), np.full(nq, -7, np.int32), np.full(nq, -7, np.int64))
    return tuple(cuda(a) for a in out) if device else out


def host(out):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def packed(lists, pad=0):
    """the shards' answers in the layout of eps_range_pack_bytes, shard s at s * (pack + pad) of one device buffer; the gaps poisoned"""
    ids, dist, counts, totals = lists
    G, nq, cap = ids.shape
    pack = amd.range_pack_bytes(nq, cap)
    assert pack == (nq * cap * 12 + nq * 12 + 7) // 8 * 8
    stride = pack + pad
    buf = np.full(G * stride, 0xA5, np.uint8)
    for s in range(G):
        o = s * stride
        for a in (ids[s], totals[s], dist[s], counts[s]):   # ids | totals | distances | counts
            b = np.ascontiguousarray(a).view(np.uint8).ravel()
            buf[o:o + len(b)] = b
            o += len(b)
    return cuda(buf), stride


# ---- 1. synthetic lists
def lists_for(G, nq, cap):
    """(lists, reference); beyond 700 queries the first 700 repeat - queries are merged independently, and the point is where they sit in the grid"""
    base = min(nq, 700)
    lists = mr.random_lists(np.random.default_rng([G, nq, cap]), G, base, cap, first_kind=0 if nq >= 7 else 2)
    want = mr.merge_range(*lists)
    if nq > base:
        assert nq % base == 0
        r = nq // base
        lists = tuple(np.ascontiguousarray(np.tile(a, (1, r) + (1,) * (a.ndim - 2))) for a in lists)
        want = tuple(np.ascontiguousarray(np.tile(a, (r,) + (1,) * (a.ndim - 1))) for a in want)
    return lists, want


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nq,cap", [(1, 1), (70, 8), (70, 100), (2, 8192), (70000, 2)])
def test_synthetic_lists_equal_the_reference_on_every_path(G, nq, cap):
    lists, want = lists_for(G, nq, cap)
    ids, dist, counts, totals = lists
    assert ids.shape == (G, nq, cap)
    if nq >= 70:   # what the lists plant (tests/test_merge_ref_cpu.py holds the generator to its promises)
        assert (counts.sum(axis=0) == 0).any() and (G == 1 or ((counts == cap).sum(axis=0) == 1).any()) and (totals > cap).any()
    else:
        assert (counts == cap).all(axis=0).any()   # every list full: G * cap keys of one query
    what = "G %d nq %d cap %d" % (G, nq, cap)
    # host buffers
    got = amd.merge_range(*lists, out=poisoned(nq, cap))
    mr.same_range(got, want, what + " host")
    # device buffers
    dl = tuple(cuda(a) for a in lists)
    out = poisoned(nq, cap, device=True)
    assert amd.merge_range(*dl, out=out)[0] is out[0]
    mr.same_range(host(out), want, what + " device")
    dev = amd.merge_range(*dl)   # buffers of the library's choosing: device in, device out
    assert all(hasattr(t, "data_ptr") for t in dev)
    mr.same_range(host(dev), want, what + " device, no out=")
    # one gathered buffer, the shards' packs next to each other and 16 bytes apart
    for pad in (0, 16):
        buf, stride = packed(lists, pad)
        out = poisoned(nq, cap, device=True)
        amd.merge_range_packed(buf, stride, G, nq, cap, out=out)
        mr.same_range(host(out), want, what + " packed, pad %d" % pad)
    # counts and totals are optional
    L = amd._lib.load()
    out = poisoned(nq, cap, device=True)
    rc = L.eps_merge_range(*(C.c_void_p(t.data_ptr()) for t in dl), G, nq, cap, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), None, None, 0, None)
    assert rc == 0
    got = host(out)
    mr.same_range(got[:2], want[:2], what + " without counts and totals")
    assert (got[2] == -7).all() and (got[3] == -7).all()


def test_nan_distances_sort_after_infinity_and_no_queries_is_ok():
    G, nq, cap = 3, 2, 8
    ids = np.arange(G * nq * cap, dtype=np.int64).reshape(G, nq, cap)
    dist = np.zeros((G, nq, cap), F)
    dist[:, :, :] = np.array([0.5, np.inf, np.nan, -np.nan, np.nan, -np.nan, np.nan, np.nan], F)   # (both NaN signs: one ordinal, ordered by id)
    dist[1, :, 0] = -0.0
    counts = np.full((G, nq), cap, np.int32)
    totals = np.full((G, nq), cap, np.int64)
    want = mr.merge_range(ids, dist, counts, totals)
    assert mr.bits(want[1][0]).tolist() == mr.bits(np.array([0, 0.5, 0.5, np.inf, np.inf, np.inf, np.nan, np.nan], F)).tolist()
    assert want[0][0].tolist() == [16, 0, 32, 1, 17, 33, 2, 3]   # (the NaNs by id, whatever their sign)
    mr.same_range(amd.merge_range(ids, dist, counts, totals), want, "host")
    mr.same_range(host(amd.merge_range(*(cuda(a) for a in (ids, dist, counts, totals)))), want, "device")
    L = amd._lib.load()
    assert L.eps_merge_range(ids.ctypes.data, dist.ctypes.data, counts.ctypes.data, totals.ctypes.data, G, 0, cap, ids.ctypes.data, dist.ctypes.data, None, None, 0, None) == 0


def test_every_kind_of_query_on_the_form_that_searches_global_memory():
    """3 x 2048 keys of 12 bytes are more than a workgroup stages: empty queries, one full list among empty ones, ties - spread over workgroups"""
    G, nq, cap = 3, 14, 2048
    lists = mr.random_lists(np.random.default_rng(2048), G, nq, cap)
    assert (lists[2].sum(axis=0) == 0).any() and ((lists[2] == cap).sum(axis=0) == 1).any()
    want = mr.merge_range(*lists)
    out = poisoned(nq, cap, device=True)
    amd.merge_range(*(cuda(a) for a in lists), out=out)
    mr.same_range(host(out), want, "device")
    mr.same_range(amd.merge_range(*lists, out=poisoned(nq, cap)), want, "host")


@pytest.mark.parametrize("G", GS)
def test_synthetic_select_lists(G):
    import torch
    rng = np.random.default_rng(G)
    for length in (0, 1, 40, 5000):   # (5000: G * 5000 ids no longer fit a workgroup's LDS for G >= 2: the form that searches global memory)
        counts = rng.integers(0, length + 1, G).astype(np.int64)
        counts[rng.integers(0, G)] = length
        ids = rng.integers(-9, 9, (G, length)).astype(np.int64)   # (tails hold garbage)
        for s in range(G):
            ids[s, :counts[s]] = np.sort(rng.integers(0, max(2 * length, 1), counts[s])) * (1 << 31)   # (duplicates inside and across shards)
        totals = counts + rng.integers(0, 5, G)
        d = (cuda(ids), cuda(counts), cuda(totals))
        for skip, limit in ((0, length), (0, min(10, length)), (length // 2, length - length // 2), (length // 3, length // 3), (length, 0)):
            want = mr.merge_select(ids, counts, totals, skip, limit)
            got = amd.merge_select(ids, counts, totals, skip, limit, out=(np.full(limit, -7, np.int64), np.full(2, -7, np.int64)))
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (G, length, skip, limit)
            o_ids, o_counts = amd.merge_select(*d, skip, limit, out=(torch.full((limit,), -7, dtype=torch.int64, device="cuda"), torch.full((2,), -7, dtype=torch.int64, device="cuda")))
            torch.cuda.synchronize()
            o_ids, o_counts = o_ids.cpu().numpy(), o_counts.cpu().numpy()
            m = len(want[0])
            assert o_counts.tolist() == [m, want[1]] and np.array_equal(o_ids[:m], want[0]) and (o_ids[m:] == -1).all(), (G, length, skip, limit)
        if length:
            assert amd.merge_select(ids, counts, totals, 1)[0].shape == mr.merge_select(ids, counts, totals, 1, length - 1)[0].shape   # limit=None: the rest


# ---- 2., 3. G indices over the rows i mod G against one index over the table
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


def index(X, metric):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    ix.attach_rows(X)
    return ix


def split(X, metric, G, deleted=None, program=None, rows=None):
    """the whole table's index and G indices over its rows s, s + G, ..: ids through set_id_map(s, G), every shard its slice of the deleted bitset and
    of the attribute rows"""
    n = len(X)
    whole = index(X, metric)
    parts = []
    for s in range(G):
        ix = index(np.ascontiguousarray(X[s::G]), metric)
        ix.set_id_map(s, G)
        parts.append(ix)
    for ix, sel in [(whole, slice(None))] + [(p, slice(s, None, G)) for s, p in enumerate(parts)]:
        if deleted is not None:
            gone = np.unpackbits(deleted, bitorder="little")[:n][sel]
            ix.set_deleted(np.packbits(np.concatenate([gone, np.zeros(-len(gone) % 8, np.uint8)]), bitorder="little"))
        if program is not None:
            ix.set_filter_program(program, np.ascontiguousarray(rows[sel]))
    return whole, parts


def close(whole, parts):
    whole.close()
    for p in parts:
        p.close()


@pytest.mark.parametrize("d", [19, 64])
@pytest.mark.parametrize("metric", [0, 2])
def test_sharded_radius_search_equals_the_unsharded_one(metric, d):
    n, nq = 2600, 10
    X, Q = er.make("integers -8..8", n, d, nq, seed=40 + metric)
    d32 = rr.dist32(X, Q, metric)
    s_ = np.sort(d32, axis=0)
    # none, the closest row alone (no row in the other shards), dozens, hundreds, the whole table
    radius = np.array([s_[(0, 0, 40, 700, n - 1)[q % 5], q] + F(0.5) * (q % 5 > 0) - F(0.5) * (q % 5 == 0) for q in range(nq)], F)
    rng = np.random.default_rng(d)
    deleted = np.packbits(rng.random((n + 7) // 8 * 8) < 0.2, bitorder="little")
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    r2 = float(np.median(s_[1500])) + 0.5   # the program cuts the widest radii at r2, and reads the exact distance to do it
    prog = [("f32", 4), ("const", 0.2), (">",), ("dist",), ("const", r2), ("<",), ("and",)]
    vis = np.stack([sr.visible_rows(n, deleted=deleted, program=prog, rows=rows, dist=d32[:, q].astype(np.float64)) for q in range(nq)], axis=1)
    for G in (2, 3):
        whole, parts = split(X, metric, G, deleted, prog, rows)
        for cap in (8, 256):
            want = rr.numpy_range(d32, radius, cap, visible=vis)
            assert (want[3] == 0).any() and (want[3] > cap).any() and ((want[3] > 0) & (want[3] <= cap)).any() and (want[3] == 1).any()
            for eng in ENGINES:
                one = whole.search_range(Q, radius, cap, flat_engine=eng)
                mr.same_range(one, want, "unsharded %s" % eng)
                got = amd.search_range_shards(parts, Q, radius, cap, flat_engine=eng)
                mr.same_range(got, one, "G %d cap %d %s" % (G, cap, eng))
        # a shard's own total beyond cap, and a query with no row in some shard
        per = [rr.numpy_range(d32[s::G], radius, 8, visible=vis[s::G])[3] for s in range(G)]
        assert any((t > 8).any() for t in per) and any(((t == 0) & (want[3] > 0)).any() for t in per)
        # device queries give device tensors
        got = amd.search_range_shards(parts, cuda(Q), radius, 256)
        assert all(hasattr(t, "data_ptr") for t in got)
        mr.same_range(host(got), whole.search_range(Q, radius, 256), "G %d device" % G)
        close(whole, parts)


def test_sharded_radius_search_on_a_continuous_table():
    """uniform floats, COSINE, normalised: a row's exact distance does not depend on which index holds the row, so the bits agree here too"""
    n, d, nq, cap = 3000, 64, 16, 64
    X, Q = er.make("uniform", n, d, nq)
    X = np.ascontiguousarray(X / np.linalg.norm(X, axis=1, keepdims=True), F)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), F)
    radius = rr.midway_radii(er.Ref(X, Q, 1), 20)
    radius[::4] = rr.midway_radii(er.Ref(X, Q, 1), 200)[::4]   # (total > cap)
    for G in (2, 3):
        whole, parts = split(X, 1, G)
        for eng in ENGINES:
            one = whole.search_range(Q, radius, cap, flat_engine=eng)
            assert (one[3] == 20).any() and (one[3] == 200).any()
            mr.same_range(amd.search_range_shards(parts, Q, radius, cap, flat_engine=eng), one, "G %d %s" % (G, eng))
        close(whole, parts)


def test_sharded_select_equals_the_unsharded_one():
    n = 2600
    X = np.zeros((n, 4), F)
    rng = np.random.default_rng(6)
    deleted = np.packbits(rng.random((n + 7) // 8 * 8) < 0.25, bitorder="little")
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    prog = [("i32", 0), ("const", 3), ("%",), ("const", 0), ("=",), ("f32", 4), ("const", 0.4), (">",), ("or",)]
    vis = sr.visible_rows(n, deleted=deleted, program=prog, rows=rows)
    total = int(vis.sum())
    assert 1000 < total < 2000
    for G in (2, 3):
        whole, parts = split(X, 0, G, deleted, prog, rows)
        for skip, limit in ((0, 10), (700, 300), (total - 5, 20), (total + 3, 10), (5, 0), (0, None), (n + 50, 4)):
            want = sr.expected(vis, skip, n if limit is None else limit)
            one = whole.select(skip, limit)
            assert np.array_equal(one[0], want[0]) and one[1] == want[1] == total
            got = amd.select_shards(parts, skip, limit)
            assert np.array_equal(got[0], one[0]) and got[1] == one[1], (G, skip, limit)
        close(whole, parts)


def test_sharded_select_with_lists_that_span_workgroups():
    n, G = 15001, 3
    X = np.zeros((n, 4), F)
    deleted = np.packbits(np.random.default_rng(7).random((n + 7) // 8 * 8) < 0.1, bitorder="little")
    vis = sr.visible_rows(n, deleted=deleted)
    whole, parts = split(X, 0, G, deleted)
    for skip, limit in ((0, 5000), (4000, 1000), (13000, 2001)):   # (len = 5000 per shard; the last runs across the last visible row)
        one = whole.select(skip, limit)
        want = sr.expected(vis, skip, limit)
        assert np.array_equal(one[0], want[0]) and one[1] == want[1]
        got = amd.select_shards(parts, skip, limit)
        assert np.array_equal(got[0], one[0]) and got[1] == one[1], (skip, limit)
    close(whole, parts)


# ---- 4. the exchange step (a communicator of one rank: RCCL refuses two ranks on one device)
def test_exchange_of_radius_answers_on_rccl_world_of_one():
    import torch
    x = amd.Exchange(0, 1, amd.Exchange.unique_id(), device=0)
    stream = torch.cuda.current_stream().cuda_stream
    for nq, cap in ((1, 1), (7, 3), (70, 100), (1024, 10)):
        ids, dist, counts, totals = (a[0] for a in mr.random_lists(np.random.default_rng([nq, cap]), 1, nq, cap))
        d = tuple(cuda(a) for a in (ids, dist, counts, totals))
        out = poisoned(nq, cap, device=True)
        x.allgather_merge_range(*d, out=out, stream=stream)
        got = host(out)
        # the rank's own answer, the tails normalised
        live = np.arange(cap)[None, :] < counts[:, None]
        want = (np.where(live, ids, -1), np.where(live, dist + F(0), np.inf).astype(F), counts, totals)
        mr.same_range(got, want, "world of one, nq %d cap %d" % (nq, cap))
        buf, stride = packed(tuple(a[None] for a in (ids, dist, counts, totals)))
        mr.same_range(host(amd.merge_range_packed(buf, stride, 1, nq, cap)), got, "the packed merge over the same bytes")
        mr.same_range(host(x.allgather_merge_range(*d, stream=stream)), got, "no out=")
    t = x.times_us(8)
    assert len(t) == 8 and all(a >= 0 and b >= 0 for a, b in t)
    with pytest.raises(EpsillaError) as e:
        x.allgather_merge_range(*(cuda(a) for a in (np.zeros((1, 8193), np.int64), np.zeros((1, 8193), F), np.zeros(1, np.int32), np.zeros(1, np.int64))))
    assert e.value.code == 30000 and "cap" in str(e.value)
    L = amd._lib.load()
    h = (np.zeros((1, 4), np.int64), np.zeros((1, 4), F), np.zeros(1, np.int32), np.zeros(1, np.int64))
    p = [a.ctypes.data for a in h]
    assert L.eps_exchange_allgather_merge_range(x.h, *p, 1, 4, *p, None) == 30000 and "device" in L.eps_exchange_last_error(x.h).decode()
    x.close()


# ---- 5. refusals
def test_refusals(capfd):
    G, nq, cap = 2, 3, 4
    ids, dist, counts, totals = mr.random_lists(np.random.default_rng(0), G, nq, cap)
    L = amd._lib.load()
    for shape, word in (((17, 1, 4), "shards"), ((2, 1, 8193), "cap")):
        with pytest.raises(EpsillaError) as e:
            amd.merge_range(np.zeros(shape, np.int64), np.zeros(shape, F), np.zeros(shape[:2], np.int32), np.zeros(shape[:2], np.int64))
        assert e.value.code == 30000 and word in str(e.value)
        with pytest.raises(EpsillaError) as e:
            amd.merge_range_packed(cuda(np.zeros(1 << 20, np.uint8)), 1 << 16, shape[0], 1, shape[2])
        assert e.value.code == 30000 and word in str(e.value)
    # a mixed host / device set: the wrapper refuses it, and so does the library
    out = poisoned(nq, cap)
    with pytest.raises(ValueError) as e:
        amd.merge_range(cuda(ids), dist, counts, totals)
    assert "device" in str(e.value)
    with pytest.raises(ValueError) as e:
        amd.merge_range(ids, dist, counts, totals, out=poisoned(nq, cap, device=True))
    assert "device" in str(e.value)
    d_ids = cuda(ids)
    capfd.readouterr()
    rc = L.eps_merge_range(C.c_void_p(d_ids.data_ptr()), dist.ctypes.data, counts.ctypes.data, totals.ctypes.data, G, nq, cap, out[0].ctypes.data, out[1].ctypes.data,
                           out[2].ctypes.data, out[3].ctypes.data, 0, None)
    assert rc == 30000 and "all be host or all be device" in capfd.readouterr().err
    assert (out[0] == -7).all()
    c = np.zeros(2, np.int64)
    sel = np.zeros((2, 4), np.int64)
    o2 = np.zeros(4, np.int64)
    d_sel = cuda(sel)
    rc = L.eps_merge_select(C.c_void_p(d_sel.data_ptr()), c.ctypes.data, c.ctypes.data, 2, 4, 0, 4, o2.ctypes.data, c.ctypes.data, None, 0, None)
    assert rc == 30000 and "all be host or all be device" in capfd.readouterr().err
    with pytest.raises(ValueError):
        amd.merge_select(d_sel, c, c, 0, 2)
    # a list shorter than the window reaches; negative arguments
    with pytest.raises(EpsillaError) as e:
        amd.merge_select(sel, c, c, skip=3, limit=2)
    assert e.value.code == 30000 and "skip + limit" in str(e.value)
    for kw in (dict(skip=-1, limit=1), dict(skip=0, limit=-1)):
        with pytest.raises(EpsillaError) as e:
            amd.merge_select(sel, c, c, out=(o2[:max(kw["limit"], 0)], np.zeros(2, np.int64)), **kw)
        assert e.value.code == 30000 and "negative" in str(e.value)
    assert L.eps_merge_select(sel.ctypes.data, c.ctypes.data, c.ctypes.data, 2, -1, 0, 0, o2.ctypes.data, c.ctypes.data, None, 0, None) == 30000
    assert L.eps_merge_range(ids.ctypes.data, dist.ctypes.data, counts.ctypes.data, totals.ctypes.data, G, -1, cap, out[0].ctypes.data, out[1].ctypes.data, None, None, 0, None) == 30000
    for shards in ([], [None] * 17):
        with pytest.raises(EpsillaError) as e:
            amd.select_shards(shards)
        assert e.value.code == 30000 and "shards" in str(e.value)
