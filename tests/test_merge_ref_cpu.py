"""CPU checks of the merge of radius answers and ordered selects across shards (eps_merge_range, eps_merge_select; csrc/merge_lists.hip):

(a) tests/merge_ref.py's two statements - sort and cut; rank by counting - agree on lists with planted ties, and the rank rule writes no slot twice;
(b) the claim the merge exists for: split a table's rows by i mod G, answer every shard with range_ref / select_ref, merge - the answer of the
    whole table, totals included;
(c) header, library and ctypes binding agree on the five new entry points;
(d) the host side of the calls (csrc/merge_host.hpp: argument checks, packed layout, staging) as a stand-alone program under
    AddressSanitizer and UBSan, with the launch replaced by a serial merge.
No GPU is touched.  Every comparison is equality of integers and of float bit patterns."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exact_ref as er
import merge_ref as mr
import range_ref as rr
import select_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GS = (1, 2, 3, 16)


# ---- (a)
def test_ordinals_order_floats_as_make_key_does():
    d = np.array([-np.inf, -3.0, -0.0, 0.0, 1e-45, 0.5, np.inf, np.nan, -np.nan], F)
    o = mr.ordinal(d)
    assert o[2] == o[3] and o[7] == o[8] == mr.ORD_NAN and (np.diff(o[[0, 1, 2, 4, 5, 6, 7]].astype(np.int64)) > 0).all()
    back = mr.ord2f(o)
    assert np.array_equal(mr.bits(back[:7]), mr.bits(d[:7] + F(0))) and np.isnan(back[7:]).all()
    assert mr.bits(back[2:4]).tolist() == [0, 0]   # (-0 comes back as +0)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nq,cap", [(1, 1), (21, 2), (21, 8), (14, 37)])
def test_rank_rule_equals_sort_and_cut_on_planted_ties(G, nq, cap):
    rng = np.random.default_rng([G, nq, cap])
    for plant in (True, False):
        lists = mr.random_lists(rng, G, nq, cap, plant)
        for skip in (0, 3):
            want = mr.merge_range(*lists, skip=skip)
            got = mr.rank_range(*lists, skip=skip)
            assert not got[4], "the ranks are not a permutation"
            mr.same_range(got[:4], want, "G %d nq %d cap %d skip %d plant %s" % (G, nq, cap, skip, plant))
        assert (want[2] == np.clip(np.clip(lists[2], 0, cap).sum(axis=0) - 3, 0, cap)).all()
    ids, dist, counts, totals = lists
    assert G == 1 or nq < 7 or (counts.sum(axis=0) == 0).any()   # (the all-empty query is there)


def test_random_lists_plant_what_they_promise():
    ids, dist, counts, totals = mr.random_lists(np.random.default_rng(1), 3, 70, 8)
    assert (counts.sum(axis=0) == 0).any() and ((counts == 8).sum(axis=0) == 1).any() and (totals > 8).any() and (counts == 0).any()
    dup = tie = False
    for j in range(70):
        a = [(mr.ordinal(dist[s, j, :counts[s, j]]), ids[s, j, :counts[s, j]]) for s in range(3)]
        tie |= len(np.intersect1d(a[0][0], a[1][0])) > 0
        dup |= len(np.intersect1d(a[0][1], a[2][1])) > 0
        for o, i in a:   # sorted by (ordinal, id)
            k = o.astype(object) * (1 << 64) + (i.astype(object) + (1 << 63))
            assert all(k[p] <= k[p + 1] for p in range(len(k) - 1))
    assert dup and tie
    assert (np.signbit(dist) & (dist == 0)).any() and np.isposinf(dist).any() and (ids > 1 << 32).any()


@pytest.mark.parametrize("G", GS)
def test_select_rank_rule_equals_sort_and_cut(G):
    rng = np.random.default_rng(G)
    for length in (0, 1, 9, 300):
        counts = rng.integers(0, length + 1, G)
        counts[rng.integers(0, G)] = length
        ids = np.full((G, length), -1, np.int64)
        for s in range(G):
            ids[s, :counts[s]] = np.sort(rng.integers(0, 40, counts[s]))   # (duplicates inside and across shards)
        totals = counts + rng.integers(0, 5, G)
        for skip, limit in ((0, length), (0, min(10, length)), (length // 2, length - length // 2), (length, 0)):
            want = mr.merge_select(ids, counts, totals, skip, limit)
            got = mr.rank_select(ids, counts, totals, skip, limit)
            assert not got[2] and np.array_equal(got[0], want[0]) and got[1] == want[1] == totals.sum(), (G, length, skip, limit)


# ---- (b)
def shard_rows(n, G, s):
    return np.arange(s, n, G)


@pytest.fixture(scope="module")
def table():
    n, d, nq = 2600, 19, 12
    X, Q = er.make("integers -8..8", n, d, nq, seed=8)
    deleted = np.packbits(np.random.default_rng(8).random((n + 7) // 8 * 8) < 0.3, bitorder="little")
    return X, Q, sr.visible_rows(n, deleted=deleted)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("cap", [8, 256])
def test_sharded_radius_answers_merge_into_the_unsharded_answer(table, G, metric, cap):
    X, Q, vis = table
    n, nq = len(X), len(Q)
    d32 = rr.dist32(X, Q, metric)
    s_ = np.sort(d32, axis=0)
    radius = np.array([s_[(0, 0, 40, 700, n - 1)[q % 5], q] + F(0.5) * (q % 5 > 0) - F(0.5) * (q % 5 == 0) for q in range(nq)], F)   # none, the closest, dozens, hundreds, all
    want = rr.numpy_range(d32, radius, cap, visible=vis)
    assert (want[3] == 0).any() and (want[3] > cap).any() and ((want[3] > 0) & (want[3] <= cap)).any()
    parts = []
    for s in range(G):
        rows = shard_rows(n, G, s)
        ids, dist, counts, totals = rr.numpy_range(d32[rows], radius, cap, visible=vis[rows])
        parts.append((np.where(ids >= 0, ids * G + s, -1), dist, counts, totals))
    lists = [np.stack([p[i] for p in parts]) for i in range(4)]
    assert G == 1 or 2 * G * cap > n or (lists[3] > cap).any()   # (a shard's own total beyond cap, where a shard has that many rows)
    assert G < 3 or ((lists[2] == 0) & (want[3][None, :] > 0)).any()   # (a query with no row in some shard)
    mr.same_range(mr.merge_range(*lists), want, "sort and cut, G %d" % G)
    got = mr.rank_range(*lists)
    assert not got[4]
    mr.same_range(got[:4], want, "rank rule, G %d" % G)


@pytest.mark.parametrize("G", GS)
def test_sharded_selects_merge_into_the_unsharded_select(table, G):
    X, Q, vis = table
    n = len(X)
    total = int(vis.sum())
    for skip, limit in ((0, 10), (700, 300), (total - 5, 20), (total + 3, 10), (5, 0), (0, n)):
        want_ids, want_total = sr.expected(vis, skip, limit)
        length = min(skip + limit, n)
        ids = np.full((G, length), -1, np.int64)
        counts, totals = np.zeros(G, np.int64), np.zeros(G, np.int64)
        for s in range(G):
            rows = shard_rows(n, G, s)
            got, totals[s] = sr.expected(vis[rows], 0, length, base=s, stride=G)
            counts[s] = len(got)
            ids[s, :len(got)] = got
        window = min(limit, max(length - skip, 0))
        for f in (mr.merge_select, mr.rank_select):
            got = f(ids, counts, totals, min(skip, length), window)
            assert np.array_equal(got[0], want_ids) and got[1] == want_total == total, (G, skip, limit, f.__name__)


# ---- (c)
NEW = {"eps_merge_range": "int32_t", "eps_range_pack_bytes": "int64_t", "eps_merge_range_packed": "int32_t", "eps_merge_select": "int32_t",
       "eps_exchange_allgather_merge_range": "int32_t"}
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64}


def test_header_library_and_binding_agree_on_the_five_entry_points():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    lib = C.CDLL(build())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read(), flags=re.S)
    L = _lib.load()
    for name, ret in NEW.items():
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m and m.group(1) == ret, name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        want = []
        for arg in m.group(2).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else CTYPE[arg.split()[-2]])
        f = getattr(L, name)
        assert list(f.argtypes) == want, (name, f.argtypes, want)
        assert f.restype is CTYPE[ret], (name, f.restype)
    assert L.eps_range_pack_bytes(3, 5) == 3 * 5 * 8 + 3 * 8 + 3 * 5 * 4 + 3 * 4 == 216
    assert L.eps_range_pack_bytes(3, 1) == 24 + 24 + 12 + 12 + 0 and L.eps_range_pack_bytes(1, 1) == 24   # (21 bytes rounded up to 8)
    assert L.eps_range_pack_bytes(0, 8) == 0 and L.eps_range_pack_bytes(-1, 8) == -1 and L.eps_range_pack_bytes(1, 8193) == -1
    import vectordb_amd as amd
    assert amd.range_pack_bytes(70, 100) == 70 * 100 * 12 + 70 * 12


def test_refusals_that_need_no_device():
    """the argument checks come before the first device call: status codes from the library, reasons from the wrapper"""
    import vectordb_amd as amd
    from vectordb_amd import _lib
    L = _lib.load()
    i64, f32, i32 = np.zeros((2, 3, 4), np.int64), np.zeros((2, 3, 4), F), np.zeros((2, 3), np.int32)
    o = (np.zeros((3, 4), np.int64), np.zeros((3, 4), F), np.zeros(3, np.int32), np.zeros(3, np.int64))
    p = lambda a: a.ctypes.data   # noqa: E731
    t = np.zeros((2, 3), np.int64)
    for shards, cap, nq in ((17, 4, 3), (0, 4, 3), (2, 8193, 3), (2, 0, 3), (2, 4, -1)):
        assert L.eps_merge_range(p(i64), p(f32), p(i32), p(t), shards, nq, cap, p(o[0]), p(o[1]), p(o[2]), p(o[3]), 0, None) == 30000, (shards, cap, nq)
        assert L.eps_merge_range_packed(p(i64), 1 << 20, shards, nq, cap, p(o[0]), p(o[1]), p(o[2]), p(o[3]), 0, None) == 30000, (shards, cap, nq)
    assert L.eps_merge_range(None, p(f32), p(i32), p(t), 2, 3, 4, p(o[0]), p(o[1]), p(o[2]), p(o[3]), 0, None) == 30000
    assert L.eps_merge_range(None, None, None, None, 2, 0, 4, None, None, None, None, 0, None) == 0       # (nq = 0: nothing is read)
    assert L.eps_merge_range(None, None, None, None, 17, 0, 4, None, None, None, None, 0, None) == 30000   # (but the ranges hold)
    assert L.eps_merge_range_packed(p(i64), 8, 2, 3, 4, p(o[0]), p(o[1]), p(o[2]), p(o[3]), 0, None) == 30000        # a stride below the pack
    c = np.zeros(2, np.int64)
    for length, skip, limit in ((4, 3, 2), (4, 5, 0), (-1, 0, 0), (4, -1, 1), (4, 0, -1)):
        assert L.eps_merge_select(p(i64), p(c), p(c), 2, length, skip, limit, p(o[0]), p(c), None, 0, None) == 30000, (length, skip, limit)
    assert L.eps_merge_select(p(i64), p(c), p(c), 17, 4, 0, 1, p(o[0]), p(c), None, 0, None) == 30000
    # the wrapper names the reason, and checks buffers before the library sees them
    with pytest.raises(amd.EpsillaError) as e:
        amd.merge_range(np.zeros((17, 3, 4), np.int64), np.zeros((17, 3, 4), F), np.zeros((17, 3), np.int32), np.zeros((17, 3), np.int64))
    assert e.value.code == 30000 and "shards" in str(e.value)
    with pytest.raises(amd.EpsillaError) as e:
        amd.merge_range(np.zeros((2, 1, 8193), np.int64), np.zeros((2, 1, 8193), F), np.zeros((2, 1), np.int32), np.zeros((2, 1), np.int64))
    assert e.value.code == 30000 and "cap" in str(e.value)
    with pytest.raises(amd.EpsillaError) as e:
        amd.merge_select(np.zeros((2, 4), np.int64), c, c, skip=3, limit=2)
    assert e.value.code == 30000 and "skip + limit" in str(e.value)
    with pytest.raises(amd.EpsillaError) as e:
        amd.merge_select(np.zeros((2, 4), np.int64), c, c, skip=-1, limit=2)
    assert e.value.code == 30000 and "negative" in str(e.value)
    for bad in (dict(ids=np.zeros((2, 3, 4), np.int32)), dict(dist=np.zeros((2, 3, 5), F)), dict(counts=np.zeros((2, 3), np.int64)),
                dict(totals=np.zeros((3, 2), np.int64).T), dict(out=(o[0], o[1], o[2], np.zeros(4, np.int64)))):
        kw = dict(ids=i64, dist=f32, counts=i32, totals=t)
        kw.update(bad)
        with pytest.raises(ValueError):
            amd.merge_range(**kw)
    with pytest.raises(ValueError):
        amd.merge_select(np.zeros((2, 4), np.int64), c, c, 0, 2, out=(np.zeros(3, np.int64), np.zeros(2, np.int64)))
    with pytest.raises(ValueError):
        amd.merge_range_packed(np.zeros(64, np.uint8), 32, 2, 1, 1)   # a host buffer


# ---- (d)
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_merge_kernel_uses_no_scratch_and_fits_the_default_lds(tmp_path):
    """four forms (radius / select keys x LDS / global search), none with scratch memory; the static LDS (list lengths) and the 60 KB of staged
    keys the launcher allows stay inside the 64 KB a workgroup gets by default"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "merge_lists.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "ml.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    forms = {k: v for k, v in usage.items() if "merge_rank_kernel" in k}
    assert len(forms) == 4, list(usage)
    staged = int(re.search(r"ML_LDS_BYTES = (\d+) \* 1024", open(src).read()).group(1)) * 1024
    for k, u in forms.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 64, (k, u)
        assert u["LDS Size [bytes/block]"] + staged <= 65536, (k, u)


def test_host_staging_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "merge_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "merge_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "merge_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
