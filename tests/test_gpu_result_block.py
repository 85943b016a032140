"""What the serving calls of one index share (csrc/index_calls.cpp): the device block behind host results (ResultBlock, csrc/result_block.hpp - one
buffer for search, select, search_range, search_among, search_groups and search_group_rows) and the flat-engine rule with its count of
single-query searches.

  1. one handle serves every call in turn, with odd sizes, forwards and backwards - the shared block grows, then is reused at smaller sizes: every
     array equals, bit for bit, the same call's on a fresh index that has served nothing else.  Host results on both paths of fetch_to_host
     (EPS_HOST_STAGING unset / 0), then device results with the optional outputs null.
  2. only a search counts towards the 8-bit mirror that FLAT_AUTO builds for single-query traffic: search_range and search_groups calls between
     the searches leave their sequence of engines as it is."""
import ctypes as C

import numpy as np
import pytest

from helpers import bitset, data

pytestmark = pytest.mark.gpu

N, DIM, NQ, K, M, CAP = 3000, 32, 5, 7, 3, 9          # nq * k, nq * k * m, nq * cap: all odd, so a 4-byte array ends off an 8-byte boundary
SKIP, LIMIT = 2, 11
ORDER = ("search", "search_range", "search_groups", "select", "search_group_rows", "search_among", "search")


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


def fresh(amd, t):
    ix = amd.GpuIndex(DIM, "L2")
    ix.attach_rows(t["X"])
    ix.set_id_map(5, 3)
    ix.set_deleted(t["deleted"])
    ix.set_groups(t["keys"])
    return ix


def call(amd, ix, t, name):
    """the call `name` with NumPy results, as a tuple of arrays"""
    if name == "search":
        return ix.search(t["Q"], K, mode=amd.MODE_FLAT)
    if name == "search_range":
        return ix.search_range(t["Q"], t["radius"], CAP)
    if name == "search_groups":
        return ix.search_groups(t["Q"], K)
    if name == "select":
        ids, total = ix.select(SKIP, LIMIT)
        return ids, np.array([len(ids), total], np.int64)
    if name == "search_group_rows":
        return ix.search_group_rows(t["Q"], K, M)
    return ix.search_among(t["Q"], t["cand"], K)


def same_bits(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: array %d differs" % (what, i)


@pytest.fixture(scope="module")
def table(amd):
    rng = np.random.default_rng(64)
    X, Q = data(N, DIM, 640), data(NQ, DIM, 641)
    hidden = np.nonzero(rng.random(N) < 1.0 / 3.0)[0]
    keys = rng.integers(0, 200, N).astype(np.int64) * 1000 - 7          # about 200 groups of about 15 rows
    d = ((X[None, :, :] - Q[:, None, :]) ** 2).sum(2)
    d[:, hidden] = np.inf
    rank = np.array([3, 20, 9, 0, 40])                                  # fewer rows than cap, more, exactly cap - 1 .. : totals on both sides of cap
    radius = np.sort(d, 1)[np.arange(NQ), rank].astype(np.float32)
    cand = (rng.choice(N, 301, replace=False).astype(np.int64)) * 3 + 5   # global ids (set_id_map(5, 3)), hidden rows among them
    t = dict(X=X, Q=Q, deleted=bitset(N, hidden), keys=keys, radius=radius, cand=cand)
    t["want"] = {}
    for name in set(ORDER):   # each on an index of its own that serves nothing else
        ix = fresh(amd, t)
        t["want"][name] = tuple(np.array(a, copy=True) for a in call(amd, ix, t, name))
        ix.close()
    w = t["want"]
    assert (w["search"][2] == K).all() and (w["search_among"][2] == K).all() and (w["search_groups"][3] == K).all()   # (the table answers in full)
    assert (w["search_range"][3] > CAP).any() and (w["search_range"][3] < CAP).any() and w["select"][1][0] == LIMIT
    assert (w["search_group_rows"][3] < M).any() or (w["search_group_rows"][4] > M).any()
    return t


@pytest.mark.parametrize("staging", [None, "0"])
def test_one_handle_serves_every_call_from_one_block(amd, table, monkeypatch, staging):
    if staging is None:
        monkeypatch.delenv("EPS_HOST_STAGING", raising=False)
    else:
        monkeypatch.setenv("EPS_HOST_STAGING", staging)
    ix = fresh(amd, table)
    for step, name in enumerate(ORDER + ORDER[::-1]):
        same_bits(call(amd, ix, table, name), table["want"][name], "step %d, %s" % (step, name))
    ix.close()


def test_one_handle_serves_every_call_with_device_results(amd, table):
    """device results are written in place, the optional outputs null: counts everywhere, totals, select's total, group_rows' group_sizes"""
    import torch
    t, want = table, table["want"]
    ix = fresh(amd, t)
    L, h = ix.L, ix.h
    Qd = torch.from_numpy(t["Q"]).cuda()
    p = ix.params(mode=amd.MODE_FLAT)

    def out(like):   # a device tensor of like's shape and dtype, filled with a value no call writes
        return torch.full(like.shape, -77, dtype=getattr(torch, str(like.dtype)), device="cuda")

    def ptr(a):
        return C.c_void_p(a.data_ptr())

    def run(name):
        w = want[name]
        if name == "search":
            o = [out(w[0]), out(w[1])]
            rc = L.eps_index_search(h, ptr(Qd), NQ, K, C.byref(p), ptr(o[0]), ptr(o[1]), None)
            keep = (0, 1)
        elif name == "search_range":
            o = [out(w[0]), out(w[1])]
            rc = L.eps_index_search_range(h, ptr(Qd), NQ, C.c_void_p(t["radius"].ctypes.data), CAP, C.byref(p), ptr(o[0]), ptr(o[1]), None, None)
            keep = (0, 1)
        elif name == "search_groups":
            o = [out(w[0]), out(w[1]), out(w[2])]
            rc = L.eps_index_search_groups(h, ptr(Qd), NQ, K, C.byref(p), 0, 0, 0, ptr(o[0]), ptr(o[1]), ptr(o[2]), None)
            keep = (0, 1, 2)
        elif name == "select":
            o = [torch.full((LIMIT,), -77, dtype=torch.int64, device="cuda"), torch.full((1,), -77, dtype=torch.int64, device="cuda")]
            rc = L.eps_index_select(h, SKIP, LIMIT, ptr(o[0]), ptr(o[1]), None)
            torch.cuda.synchronize()
            ix.synchronize()
            assert rc == 0 and int(o[1][0]) == LIMIT and np.array_equal(o[0].cpu().numpy(), w[0]), name
            return
        elif name == "search_group_rows":
            o = [out(w[0]), out(w[1]), out(w[2]), out(w[3])]
            rc = L.eps_index_search_group_rows(h, ptr(Qd), NQ, K, M, C.byref(p), 0, 0, 0, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None, None)
            keep = (0, 1, 2, 3)
        else:
            o = [out(w[0]), out(w[1])]
            rc = L.eps_index_search_among(h, ptr(Qd), NQ, C.c_void_p(t["cand"].ctypes.data), None, len(t["cand"]), K, ptr(o[0]), ptr(o[1]), None)
            keep = (0, 1)
        assert rc == 0, (name, L.eps_index_last_error(h))
        ix.synchronize()
        same_bits([a.cpu().numpy() for a in o], [w[i] for i in keep], name + " (device results)")

    torch.cuda.synchronize()
    for name in ORDER + ORDER[::-1]:
        run(name)
    ix.close()


def test_only_a_search_counts_towards_the_mirror(amd):
    """FLAT_AUTO, single queries, the smallest table the rule considers: 16 searches on the stream engine, the 8-bit mirror and the one-pass search
    from the 18th on (tests/test_gpu_mfma_i8.py pins that sequence on searches alone) - with a single-query search_range and a single-query
    search_groups on the pages engine, both FLAT_AUTO, between every two searches.  Neither counts: they take the stream engine (32 bits) while a
    search still would, and what they return is the stream engine's, bit for bit, throughout."""
    n, d, k = 65_536, 256, 10
    X, Q = data(n, d, 650), data(24, d, 651)
    keys = (np.arange(n, dtype=np.int64) * 7919) % 3000
    ix = amd.GpuIndex(d, 0)
    ix.attach_rows(X)
    ix.set_groups(keys)
    ref = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    radius = ref[1][:, 3].copy()   # (squared L2: the radius admits 4 rows)
    ref_range = ix.search_range(Q, radius, 8, flat_engine="stream")
    ref_groups = ix.search_groups(Q, k, engine="pages", flat_engine="stream")
    seen = []
    for i in range(24):
        r = ix.search(Q[i:i + 1], k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_AUTO)
        st = ix.stats()
        seen.append((st["main_kernel_bits"], st["one_pass"]))
        assert np.array_equal(r[0][0], ref[0][i]) and np.array_equal(r[1][0], ref[1][i]), i
        got = ix.search_range(Q[i:i + 1], radius[i:i + 1], 8, flat_engine="auto")
        range_bits = ix.stats()["main_kernel_bits"]
        same_bits(got, [a[i:i + 1] for a in ref_range], "search_range after search %d" % i)
        got = ix.search_groups(Q[i:i + 1], k, engine="pages", flat_engine="auto")
        groups_bits = ix.stats()["main_kernel_bits"]
        same_bits(got, [a[i:i + 1] for a in ref_groups], "search_groups after search %d" % i)
        if i < 15:   # (behind the 16th search the next call of any kind would be the 17th: the rule lets it take the matrix engine)
            assert (range_bits, groups_bits) == (32, 32), (i, range_bits, groups_bits)
    assert seen[:16] == [(32, 0)] * 16 and seen[17:] == [(8, 1)] * 7, seen
    ix.close()
