"""CPU side of GpuIndex.search_among (eps_index_search_among): the reference the GPU tests trust (tests/among_ref.py) agrees with the oracle's
brute-force search under the complementary deleted bitset - the route a caller has without the entry point - and catches planted faults; the
symbol is declared, listed and exported; csrc/among.hip compiles for gfx950 without scratch memory; the host planning (csrc/among_host.hpp)
passes its stand-alone check under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import among_ref as ar
import exact_ref as er
import range_ref as rr
from helpers import bitset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N, D, NQ = 400, 19, 6


def table(name, metric, seed=0):
    X, Q = er.make(name, N, D, NQ, seed=seed)
    ref = er.Ref(X, Q, metric)
    d32 = rr.dist32(X, Q, metric)
    assert np.array_equal(d32.astype(np.float64), ref.d64)   # (an exact table: fp32 in any order is the fp64 distance)
    return X, Q, ref, d32


def lists_of(seed, lengths):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(N, size=m, replace=False)).astype(np.int64) for m in lengths]


# ---- the id rule
def test_rows_of_restates_the_id_rule():
    assert ar.rows_of([5, 3, 5, -1, 10, 11, 2 ** 40, 0], 0, 1, 10).tolist() == [0, 3, 5]
    assert ar.rows_of([3, 11, 19, 4, 2, -5, 3 + 8 * 9, 3 + 8 * 10, 11], 3, 8, 10).tolist() == [0, 1, 2, 9]
    assert ar.rows_of([-7, -4, -1, 2, -10], -7, 3, 3).tolist() == [0, 1, 2]   # a negative base: ids below zero name rows
    assert ar.rows_of([], 0, 1, 10).tolist() == [] and ar.rows_of([2 ** 63 - 1, -2 ** 63], 5, 7, 10).tolist() == []


# ---- numpy_among is the oracle's brute force under the complementary bitset
@pytest.mark.parametrize("name,metric", [("integers -8..8", 0), ("integers -8..8", 2), ("integers / 16", 1)])
def test_numpy_among_equals_the_oracle_under_the_complementary_bitset(oracle, name, metric):
    from oracle.pyoracle import make_filter
    X, Q, ref, d32 = table(name, metric, seed=metric)
    lists = lists_of(3 + metric, (0, 1, 7, 40, 399, 400))
    for k in (1, 10, 64):
        ids, dist, counts = ar.numpy_among(d32, lists, k)
        for q in range(NQ):
            gone = np.setdiff1d(np.arange(N), lists[q])
            flt, keep = make_filter(deleted=bitset(N, gone.tolist()))
            rid, rd = oracle.topk_flat(metric, X, Q[q], k, flt=flt)
            m = min(k, len(lists[q]))
            assert counts[q] == m == len(rid), (q, k)
            assert np.array_equal(ids[q, :m], np.asarray(rid, np.int64)), (q, k)
            assert np.array_equal((dist[q, :m] + F(0)).view(np.uint32), (np.asarray(rd, F) + F(0)).view(np.uint32)), (q, k)
            assert (ids[q, m:] == -1).all() and np.isposinf(dist[q, m:]).all()
        ar.check_among(ids, dist, counts, ref, lists, k, exact=True)
    # one list for every query, and a visible set on top of it
    shared = lists[3]
    vis = np.ones(N, bool)
    vis[::3] = False
    ids, dist, counts = ar.numpy_among(d32, shared, 10, visible=vis)
    assert (counts == 10).all() and vis[ids].all() and np.isin(ids, shared).all()
    ar.check_among(ids, dist, counts, ref, shared, 10, visible=vis, exact=True)


# ---- planted faults
@pytest.fixture(scope="module")
def ints():
    X, Q, ref, d32 = table("integers -8..8", 0, seed=5)
    lists = lists_of(9, (30, 31, 32, 33, 34, 35))
    for q in range(NQ - 1):   # pairwise disjoint neighbours, so that an answer from the wrong list cannot pass by luck
        lists[q + 1] = np.setdiff1d(lists[q + 1], lists[q])
    return ref, d32, lists


def answer(ints, k, visible=None):
    ref, d32, lists = ints
    return [a.copy() for a in ar.numpy_among(d32, lists, k, visible)]


def test_the_numpy_answer_passes(ints):
    ref, d32, lists = ints
    for k in (1, 10, 64):
        ar.check_among(*answer(ints, k), ref, lists, k, exact=True)
        assert ar.check_among(*answer(ints, k), ref, lists, k, exact=False) == 0   # (no band on an exact table)


def test_a_duplicate_returned_twice_is_caught(ints):
    ref, d32, lists = ints
    ids, dist, counts = answer(ints, 64)
    m = counts[2]
    ids[2, m], dist[2, m] = ids[2, m - 1], dist[2, m - 1]   # the last row once more, where a list that names it twice would put it
    counts[2] += 1
    with pytest.raises(AssertionError, match="results|returned 2 times"):
        ar.check_among(ids, dist, counts, ref, lists, 64, exact=True)
    ids, dist, counts = answer(ints, 10)
    ids[2, 4], dist[2, 4] = ids[2, 3], dist[2, 3]   # ... and inside a full answer
    with pytest.raises(AssertionError, match="returned 2 times"):
        ar.check_among(ids, dist, counts, ref, lists, 10, exact=True)


def test_an_invalid_id_accepted_is_caught(ints):
    """id 2 * row + 1 names no row under (base 0, stride 2); an engine that rounds it down returns a row the list does not name"""
    ref, d32, lists = ints
    named = ar.rows_of(2 * lists[1] + 1, 0, 2, N)
    assert len(named) == 0
    got = ar.numpy_among(d32, lists, 10)   # what the rounding engine returns for query 1 ...
    want_lists = list(lists)
    want_lists[1] = named                  # ... where nothing is to be returned
    with pytest.raises(AssertionError, match="results|not visible"):
        ar.check_among(*got, ref, want_lists, 10, exact=True)
    ids, dist, counts = answer(ints, 64)
    ids[0, counts[0]], dist[0, counts[0]] = N, F(0)   # row n: one past the table
    counts[0] += 1
    with pytest.raises(AssertionError, match="results|outside the table"):
        ar.check_among(ids, dist, counts, ref, lists, 64, exact=True)


def test_a_query_answered_from_its_neighbours_list_is_caught(ints):
    ref, d32, lists = ints
    shifted = lists[1:] + lists[:1]
    got = ar.numpy_among(d32, shifted, 10)
    with pytest.raises(AssertionError, match="not visible"):
        ar.check_among(*got, ref, lists, 10, exact=True)
    with pytest.raises(AssertionError, match="not visible"):
        ar.check_among(*got, ref, lists, 10, exact=False)


def test_a_hidden_row_returned_is_caught(ints):
    ref, d32, lists = ints
    vis = np.ones(N, bool)
    got = answer(ints, 10)
    vis[got[0][4, 2]] = False   # the third row of query 4's answer is deleted
    with pytest.raises(AssertionError, match="not visible"):
        ar.check_among(*got, ref, lists, 10, visible=vis, exact=True)
    ar.check_among(*answer(ints, 10, visible=vis), ref, lists, 10, visible=vis, exact=True)


def test_a_tie_in_the_wrong_id_order_is_caught(ints):
    ref, d32, lists = ints
    ids, dist, counts = answer(ints, 64)
    hit = [(q, e) for q in range(NQ) for e in range(counts[q] - 1) if dist[q, e] == dist[q, e + 1]]
    assert hit, "the lists hold no tie: pick another seed"
    q, e = hit[0]
    ids[q, e], ids[q, e + 1] = ids[q, e + 1], ids[q, e]
    with pytest.raises(AssertionError, match="expected"):
        ar.check_among(ids, dist, counts, ref, lists, 64, exact=True)
    with pytest.raises(AssertionError, match="out of order"):
        ar.check_among(ids, dist, counts, ref, lists, 64, exact=False)


def test_a_count_one_short_is_caught(ints):
    ref, d32, lists = ints
    for k in (64, 10):
        ids, dist, counts = answer(ints, k)
        counts[3] -= 1
        ids[3, counts[3]], dist[3, counts[3]] = -1, np.inf
        with pytest.raises(AssertionError, match="results"):
            ar.check_among(ids, dist, counts, ref, lists, k, exact=True)


# ---- the continuous tables of the GPU tests: the band hides nothing, and numpy's own fp32 answer passes
@pytest.mark.parametrize("name,metric", ar.CONT)
def test_continuous_tables_leave_no_row_undecided(name, metric):
    n, d, nq = ar.CONT_SHAPE
    X, Q = er.make(name, n, d, nq, seed=7)
    ref = er.Ref(X, Q, metric)
    d32 = rr.dist32(X, Q, metric)
    for rows in ar.cont_lists():
        for k in ar.CONT_K:
            mask = er._visible(n, rows)
            er.assert_cap(ref, k, visible=mask, what=name)
            assert er.undecided(ref, k, visible=mask, bound="tree") == 0, (name, len(rows), k)
            und = ar.check_among(*ar.numpy_among(d32, rows, k), ref, rows, k, what="numpy %s" % name)
            assert und == 0


# ---- the entry point: declared, listed, exported
def test_symbol_is_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert re.search(r"int32_t eps_index_search_among\(eps_index\* h, const float\* queries, int64_t nq, const int64_t\* cand_ids, "
                     r"const int64_t\* cand_offsets, int64_t n_cand,\s*int32_t k, int64_t\* ids_out, float\* dist_out, int32_t\* counts_out\);", hdr)
    assert "vec_search_executor.cpp:966-1013" in hdr
    assert "eps_index_search_among" in _lib.EXPORTS
    lib = C.CDLL(build())
    assert hasattr(lib, "eps_index_search_among")
    L = _lib.load()
    vp = C.c_void_p
    f = _lib._lib.eps_index_search_among   # (the loaded library itself: under EPS_TUNING_FROM_ENV the proxy wraps the call)
    assert list(f.argtypes) == [vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_int32, vp, vp, vp]
    assert f.restype is C.c_int32
    assert L.eps_index_search_among(None, None, 0, None, None, 0, 1, None, None, None) == 30000   # no handle
    assert "among.hip" in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "among_host.hpp")).read()
    assert int(re.search(r"constexpr int32_t AMONG_MAX_K = (\d+);", src).group(1)) == 1024
    assert "hip" not in re.sub(r"//.*", "", src).replace("__HIPCC__", "").lower()   # no HIP type in the planning header


def test_wrapper_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer or a wrong number of offsets is refused before either is touched"""
    from vectordb_amd.index import GpuIndex
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim = 4
    ix._keep = {}
    Q = np.zeros((3, 4), F)
    good = (np.empty((3, 5), np.int64), np.empty((3, 5), F), np.empty(3, np.int32))
    for which, bad in ((0, np.empty((3, 5), np.int32)), (1, np.empty((3, 4), F)), (2, np.empty(3, np.int64)), (0, np.empty((3, 10), np.int64)[:, ::2])):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError):
            ix.search_among(Q, [1, 2, 3], 5, out=tuple(out))
    with pytest.raises(ValueError, match="nq \\+ 1"):
        ix.search_among(Q, [1, 2, 3], 5, offsets=[0, 1, 3])
    ix.h = None


# ---- the kernels
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_among_kernels_use_no_scratch(tmp_path):
    """{1, 2, 4 queries x KPL 1, 2; 1 query x KPL 4, 8, 16} x {16-byte, scalar} row loads of the gather, five widths of the merge: none with
    scratch memory (the 1024-entry list of KPL = 16 is 32 registers of keys per lane); the merge's static LDS (four lists) inside 64 KB"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "among.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "among.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    gather = {k: v for k, v in usage.items() if "among_gather_kernel" in k}
    merge = {k: v for k, v in usage.items() if "among_merge_kernel" in k}
    assert len(gather) == 18 and len(merge) == 5 and len(usage) == 23, list(usage)   # (and nothing else: no kernel of another unit is compiled again here)
    for k, u in list(gather.items()) + list(merge.items()):
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256, (k, u)
    for k, u in merge.items():
        assert u["LDS Size [bytes/block]"] <= 65536, (k, u)
    # the units that share device_common.hpp's `offer` still define their own kernels only
    flat = open(os.path.join(ROOT, "vectordb_amd", "csrc", "flat_kernels.hip")).read()
    assert "among_gather_kernel" not in flat and "void flat_scan_kernel" not in open(src).read()


def test_host_planning_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "among_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "among_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "among_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
