"""eps_index_search_diverse without a GPU: the numpy model of tests/diverse_ref.py on hand-written cases; planted faults, each caught by the
comparator the GPU tests use; the conditions on the ties fixtures that keep a trivial implementation from passing; the argument checks and the LDS
layout (csrc/diverse_host.hpp) through their stand-alone check under the address and undefined-behaviour sanitizers; csrc/diverse.hip compiled for
gfx950 with its registers, LDS and scratch (none) recorded; the entry point declared, listed, exported and wrapped."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import diverse_ref as dr
import groups_ref as gr
import range_ref as rr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = F(np.nan), F(np.inf)


def l2_pairs(P):
    P = np.asarray(P, F)
    return rr.dist32(P, P, 0)


# ---- hand-written cases
def test_lambda_one_is_the_pools_head():
    d = np.array([1, 2, 2, 5, 9], F)
    D = l2_pairs(np.arange(5)[:, None] * 3)
    pos, dist, score, cnt = dr.numpy_diverse(d, D, 3, 1.0)
    assert pos.tolist() == [0, 1, 2] and dist.tolist() == [1, 2, 2] and score.tolist() == [1, 2, 2] and cnt == 3


def test_lambda_zero_still_starts_at_position_zero_then_goes_far():
    d = np.array([1, 2, 3, 4], F)
    D = l2_pairs([[0], [1], [10], [4]])
    pos, dist, score, cnt = dr.numpy_diverse(d, D, 3, 0.0)
    assert pos.tolist() == [0, 2, 3]   # farthest from row 0, then the largest min(D to 0, D to 2): 16 at position 3 against 1 at position 1
    assert score.tolist() == [0, -100, -16] and dist.tolist() == [1, 3, 4] and cnt == 3


def test_two_identical_rows_the_second_is_pushed_back():
    P = [[0, 0], [0, 0], [3, 0], [0, 4]]   # positions 0 and 1 are copies
    d = np.array([1, 1, 2, 3], F)
    pos, _, score, _ = dr.numpy_diverse(d, l2_pairs(P), 4, 0.5)
    assert pos.tolist() == [0, 3, 2, 1]   # the copy comes last: its m is 0
    assert score.tolist() == [0.5, 1.5 - 8, 1 - 4.5, 0.5]


def test_a_pool_shorter_than_k_pads():
    pos, dist, score, cnt = dr.numpy_diverse(np.array([1, 2], F), l2_pairs([[0], [1]]), 5, 0.5)
    assert cnt == 2 and pos.tolist() == [0, 1, -1, -1, -1] and np.isinf(dist[2:]).all() and np.isinf(score[2:]).all()
    pos, dist, score, cnt = dr.numpy_diverse(np.zeros(0, F), np.zeros((0, 0), F), 2, 0.5)
    assert cnt == 0 and pos.tolist() == [-1, -1] and np.isinf(score).all()


def test_nan_and_infinite_distances():
    d = np.array([-INF, 1, INF, NAN], F)   # a pool in key order: -inf first, NaN after +inf
    D = np.array([[0, 1, 4, 9], [1, 0, 1, 4], [4, 1, 0, 1], [9, 4, 1, 0]], F)
    pos, dist, score, cnt = dr.numpy_diverse(d, D, 4, 0.5)
    assert pos.tolist() == [0, 1, 2, 3] and np.isneginf(score[0]) and score[1] == 0 and np.isposinf(score[2]) and np.isnan(score[3]) and cnt == 4
    # a NaN pair distance: it seeds m after the first selection and is never replaced; it never replaces a value later
    D2 = D.copy()
    D2[1, 0] = NAN   # position 1 against the first selected row
    D2[2, 1] = NAN   # position 2 against a later one
    d2 = np.array([1, 2, 3, 4], F)
    pos, _, score, _ = dr.numpy_diverse(d2, D2, 4, 0.5)
    assert pos.tolist() == [0, 3, 2, 1] and np.isnan(score[3])   # position 1 keeps its NaN m: last; position 2 keeps m = 4, then 1
    assert score[:3].tolist() == [0.5, 2 - 4.5, 1.5 - 0.5]
    assert dr.ordinal(np.array([-0.0, 0.0], F)).tolist() == [0x80000000, 0x80000000] and dr.ordinal(-NAN) == dr.ordinal(NAN) > dr.ordinal(INF)
    assert dr.bits(dr.key_float(F(-0.0))) == 0 and dr.bits(dr.key_float(-NAN)) == 0x7FC00000


def test_a_tie_goes_to_the_smaller_position():
    d = np.array([1, 2, 2, 2], F)
    D = np.array([[0, 4, 4, 4], [4, 0, 1, 1], [4, 1, 0, 1], [4, 1, 1, 0]], F)
    info = {}
    pos, _, score, _ = dr.numpy_diverse(d, D, 3, 0.5, info=info)
    assert pos.tolist() == [0, 1, 2] and score.tolist() == [0.5, -1, 0.5] and info["tied_steps"] == 2


# ---- the fixtures, and the conditions on them
@pytest.fixture(scope="module")
def ties():
    out = []
    for n, d, nq, fetch_k, k, lams in dr.FIXTURES:
        for metric in (0, 1, 2):
            X, Q, d32 = gr.ties_table(metric, n, d, nq, seed=3)
            out.append((metric, X, d32, fetch_k, k, lams))
    return out


@pytest.fixture(scope="module")
def continuous():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((400, 24)).astype(F)
    Q = rng.standard_normal((6, 24)).astype(F)
    return X, rr.dist32(X, Q, 0), (lambda rows: rr.dist32(X[rows], X[rows], 0))


def test_on_every_ties_fixture_the_selection_differs_from_the_pools_head_and_best_scores_tie(ties):
    tied_anywhere = 0
    for metric, X, d32, fetch_k, k, lams in ties:
        pairs = dr.ties_pairs(X, metric)
        head = dr.numpy_answer(d32, pairs, k, fetch_k, 1.0)
        for q in range(d32.shape[1]):   # lambda = 1: the pool's first k
            pool = dr.pool_rows(d32[:, q], np.ones(len(X), bool), fetch_k)
            assert np.array_equal(head[0][q], pool[:k]) and np.array_equal(head[1][q], d32[pool[:k], q])
        for lam in dr.LAMBDAS[:-1]:   # every lambda <= 0.75 the GPU tests use
            info = {}
            ids = dr.numpy_answer(d32, pairs, k, fetch_k, lam, info=info)[0]
            assert all((ids[q] != head[0][q]).any() for q in range(len(ids))), (metric, len(X), lam)
            if lam in lams:
                tied_anywhere += sum(info["tied_steps"])
                assert sum(info["tied_steps"]) > 0 or len(X) == 500, (metric, len(X), lam)
    assert tied_anywhere > 50


def test_the_true_model_passes(ties, continuous):
    for metric, X, d32, fetch_k, k, lams in ties[:3]:
        a = dr.numpy_answer(d32, dr.ties_pairs(X, metric), k, fetch_k, lams[0])
        dr.same(a, tuple(x.copy() for x in a))
    X, d32, pairs = continuous
    a = dr.numpy_answer(d32, pairs, 10, 100, 0.7)
    dr.same(a, tuple(x.copy() for x in a))


# ---- planted faults
def caught(got, want):
    with pytest.raises(AssertionError):
        dr.same(got, want)


def test_a_fused_multiply_subtract_is_caught_on_a_continuous_table(continuous):
    X, d32, pairs = continuous
    caught(dr.numpy_answer(d32, pairs, 10, 100, 0.7, fault="fma"), dr.numpy_answer(d32, pairs, 10, 100, 0.7))


@pytest.mark.parametrize("fault", ["overwrite", "seed0", "reselect", "ties_larger"])
def test_a_wrong_update_of_m_a_row_selected_twice_and_ties_to_the_larger_position_are_caught(ties, fault):
    metric, X, d32, fetch_k, k, lams = ties[6]   # 200 x 4, fetch_k 200, k 32: many tied steps
    pairs = dr.ties_pairs(X, metric)
    caught(dr.numpy_answer(d32, pairs, k, fetch_k, 0.5, fault=fault), dr.numpy_answer(d32, pairs, k, fetch_k, 0.5))


def test_nan_scores_ordered_first_are_caught():
    d = np.array([1, 2, NAN], F)
    D = l2_pairs([[0], [1], [2]])
    good, bad = dr.numpy_diverse(d, D, 3, 0.5), dr.numpy_diverse(d, D, 3, 0.5, fault="nan_first")
    assert good[0].tolist() == [0, 1, 2] and bad[0].tolist() == [0, 2, 1]
    caught(bad[:3] + (np.int32(bad[3]),), good[:3] + (np.int32(good[3]),))


def test_a_first_pick_by_score_at_lambda_zero_is_caught():
    """with finite distances every first score is 0 at lambda = 0 and the tie rule hides the fault: position 0 either way.  An infinite d_0 shows
    it: 0 * -inf is a NaN score, last in the order, and a first pick by score takes position 1 - the rule takes position 0, score NaN"""
    d = np.array([-INF, 2, 3], F)
    D = np.array([[0, 9, 1], [9, 0, 9], [1, 9, 0]], F)
    good, bad = dr.numpy_diverse(d, D, 2, 0.0), dr.numpy_diverse(d, D, 2, 0.0, fault="first_by_score")
    assert good[0].tolist() == [0, 1] and np.isnan(good[2][0]) and good[2][1] == -9 and bad[0].tolist() == [1, 2]
    caught(bad[:3] + (np.int32(2),), good[:3] + (np.int32(2),))
    assert dr.numpy_diverse(np.array([1, 2, 3], F), D, 2, 0.0)[0].tolist() == [0, 1]


def test_pair_distances_with_the_roles_swapped_under_a_filter_are_caught():
    """D(c, s) is what search_among returns for row c with row s as the QUERY.  Under a program on @distance a caller who builds D from
    search_among with the roles swapped - row c as the query - and the filter still installed sees the filter judge the wrong side: a pair is
    missing (read as +inf) in one orientation only.  The matrix stops being symmetric and the selection changes."""
    P = np.array([[0], [1], [5], [6]], F)
    d = np.array([1, 2, 3, 4], F)
    D = l2_pairs(P)
    hidden = D.copy()
    hidden[2, 0] = INF   # the program hides row 2 from query-row 0 only
    good = dr.numpy_diverse(d, hidden, 3, 0.25)
    swapped = dr.numpy_diverse(d, hidden.T, 3, 0.25)
    assert good[0].tolist() != swapped[0].tolist()
    caught(swapped[:3] + (np.int32(3),), good[:3] + (np.int32(3),))


@pytest.mark.parametrize("which,pad", [(0, 0), (1, F(0)), (2, F(0))])
def test_unpadded_unused_slots_and_a_wrong_count_are_caught(which, pad):
    good = dr.numpy_answer(np.array([[1], [2]], F), lambda rows: l2_pairs(rows[:, None]), 4, 4, 0.5)
    bad = [x.copy() for x in good]
    bad[which][0, 2:] = pad
    caught(tuple(bad), good)
    bad = [x.copy() for x in good]
    bad[3][0] = 4
    caught(tuple(bad), good)


def test_lists_an_id_map_and_visibility_shape_the_pool():
    X, Q, d32 = gr.ties_table(0, 60, 4, 3, seed=3)
    pairs = dr.ties_pairs(X, 0)
    vis = np.ones(60, bool)
    vis[::3] = False
    rows = np.arange(10, 50)
    ids, dist, score, counts = dr.numpy_answer(d32, pairs, 5, 20, 0.5, visible=vis, lists=rows, base=7, stride=3)
    got_rows = (ids - 7) // 3
    assert ((ids - 7) % 3 == 0).all() and vis[got_rows].all() and ((got_rows >= 10) & (got_rows < 50)).all() and counts.tolist() == [5, 5, 5]
    for q in range(3):
        pool = dr.pool_rows(d32[:, q], vis, 20, rows=rows)
        assert got_rows[q, 0] == pool[0] and set(got_rows[q]) <= set(pool.tolist())


# ---- the host side
def test_host_checks_and_lds_layout_are_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "diverse_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "diverse_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "diverse_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "diverse_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower().replace("__hipcc__", "")   # no HIP type in the host header
    assert int(re.search(r"constexpr int32_t DIVERSE_MAX_FETCH = (\d+);", src).group(1)) == 1024
    assert int(re.search(r"constexpr int DIVERSE_THREADS = (\d+);", src).group(1)) == 256


# ---- the kernel
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_diverse_kernel_uses_no_scratch_and_the_figures_design_md_states(tmp_path):
    """diverse_select_kernel in its 16-byte and scalar forms: no scratch memory, no static LDS (the layout of diverse_host.hpp is all dynamic), at
    most 96 VGPRs so that 5 wavefronts per SIMD hide the gather's latency"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "diverse.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "diverse.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    print("\n".join("%s %s" % kv for kv in sorted(usage.items())))
    assert len(usage) == 2 and all("diverse_select_kernel" in k for k in usage), list(usage)   # (no kernel of another unit is compiled again here)
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0, (k, u)
        assert u["VGPRs"] <= 96 and u["Occupancy [waves/SIMD]"] >= 5, (k, u)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.15" in design and "at most 96 VGPRs" in design and "46 112 bytes" in design
    unit = open(src).read()
    assert "asm" not in re.sub(r"//.*", "", unit) and "__fmul_rn" in unit and "__fsub_rn" in unit   # ordinary C++; the score's three rounded operations


# ---- the entry point: declared, listed, exported, wrapped
def test_symbol_is_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert re.search(r"int32_t eps_index_search_diverse\(eps_index\* h, const float\* queries, int64_t nq, int32_t k, int32_t fetch_k, float lambda, "
                     r"const int64_t\* cand_ids,\s*const int64_t\* cand_offsets, int64_t n_cand, const eps_search_params\* p, int64_t\* ids_out, "
                     r"float\* dist_out,\s*float\* score_out, int32_t\* counts_out\);", hdr)
    assert re.search(r"eps_index_search_diverse\s+\(new\)", hdr)
    lib = C.CDLL(build())
    L = _lib.load()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert "eps_index_search_diverse" in _lib.EXPORTS and hasattr(lib, "eps_index_search_diverse")
    assert _lib._lib.eps_index_search_diverse.restype is i32
    assert list(_lib._lib.eps_index_search_diverse.argtypes) == [vp, vp, i64, i32, i32, C.c_float, vp, vp, i64, C.POINTER(_lib.SearchParams), vp, vp, vp, vp]
    assert L.eps_index_search_diverse(None, None, 0, 1, 1, 0.5, None, None, 0, None, None, None, None, None) == 30000   # no handle
    assert '"diverse.hip"' in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()


def test_wrapper_rejects_bad_out_buffers_before_any_pointer_reaches_the_library():
    from vectordb_amd.index import GpuIndex
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim = 4
    ix._keep = {}
    q, k = np.zeros((3, 4), F), 2
    good = (np.empty((3, k), np.int64), np.empty((3, k), F), np.empty((3, k), F), np.empty(3, np.int32))
    for which, bad in ((0, np.empty((3, k), np.int32)), (0, np.empty((k, 3), np.int64)), (1, np.empty((3, k), np.float64)), (2, np.empty((3, k + 1), F)),
                       (3, np.empty(3, np.int64)), (2, np.empty((3, 2 * k), F)[:, ::2])):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError):
            ix.search_diverse(q, k, 8, out=tuple(out))
    with pytest.raises(ValueError):
        ix.search_diverse(q, k, 8, out=good[:3])   # one buffer short
    with pytest.raises(ValueError):
        ix.search_diverse(q, k, 8, offsets=[0, 0, 0, 0])   # offsets without ids
    with pytest.raises(ValueError):
        ix.search_diverse(q, k, 8, ids=[1, 2], offsets=[0, 1, 2])   # nq + 1 entries are needed
    with pytest.raises(KeyError):
        ix.search_diverse(q, k, 8, flat_engine="no such engine")
    ix.h = None
