"""eps_index_search_multi without a GPU: the numpy model of tests/multi_ref.py on hand-written cases; planted faults, each caught by the comparator
the GPU tests use; the host plan (csrc/multi_host.hpp) through its stand-alone check under the address and undefined-behaviour sanitizers; the
kernels of csrc/multi.hip compiled for gfx950 with their registers, scratch (none) and LDS recorded; the entry point declared, listed, exported and
wrapped."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import groups_ref as gr
import multi_ref as mr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = F(np.nan), F(np.inf)


def answer(d, keys, sizes, k, vis=None, **kw):
    return mr.numpy_multi(np.asarray(d, F), vis, np.asarray(keys, np.int64), mr.bag_offsets(sizes), k, **kw)


# ---- hand-written cases
def test_a_bag_of_one_vector_is_search_groups_with_score_the_representative_distance():
    X, Q, d32 = gr.ties_table(0, 300, 8, 5, seed=3)
    keys = gr.layouts(300, seed=3)["n / 8 groups"]
    gk, score, counts, mrow, mdist = mr.numpy_multi(d32.T, None, keys, mr.bag_offsets([1] * 5), 7)
    ids, dist, gkeys, cnt = gr.numpy_groups(d32, keys, 300)   # every group's representative
    for q in range(5):
        m = cnt[q]
        order = mr.score_order(dist[q, :m], gkeys[q, :m])[:7]   # (equal distances: the smaller key, not the smaller row)
        assert np.array_equal(gk[q], gkeys[q, :m][order]) and np.array_equal(score[q], dist[q, :m][order]) and counts[q] == 7
        assert np.array_equal(mr.matches(mrow, mr.bag_offsets([1] * 5), 7, q)[:, 0], ids[q, :m][order])
        assert np.array_equal(mr.matches(mdist, mr.bag_offsets([1] * 5), 7, q)[:, 0], score[q])


def test_the_empty_bag_has_no_group_and_k_above_the_qualifying_groups_pads():
    d = [[1, 2, 3, 4], [4, 3, 2, 1]]
    gk, score, counts, mrow, mdist = answer(d, [10, 10, 20, 20], [0, 2, 0], 3)
    assert counts.tolist() == [0, 2, 0]
    assert gk.tolist() == [[0, 0, 0], [10, 20, 0], [0, 0, 0]]
    assert score[1].tolist()[:2] == [4.0, 4.0] and np.isinf(score[0]).all() and np.isinf(score[1, 2]) and np.isinf(score[2]).all()
    assert mrow.tolist() == [0, 1, 2, 3, -1, -1] and mdist.tolist()[:4] == [1, 3, 3, 1] and np.isinf(mdist[4:]).all()


def test_a_group_invisible_to_one_vector_only_does_not_qualify():
    d = np.array([[1, 5, 2], [9, 5, 2], [1, 5, 2]], F)   # (the second bag: vector 0 again, alone)
    vis = d < 6   # a program `@distance < 6`: row 0 is invisible to vector 1 only
    gk, score, counts, mrow, _ = answer(d, [7, 8, 9], [2, 1], 3, vis=vis)
    assert counts.tolist() == [2, 3] and gk[0].tolist() == [9, 8, 0] and score[0].tolist()[:2] == [4.0, 10.0]
    assert gk[1].tolist() == [7, 9, 8]   # the bag of vector 0 alone sees group 7


def test_a_nan_term_gives_a_nan_score_that_sorts_last_and_still_counts():
    d = np.array([[1, NAN, 3], [1, 1, INF]], F)
    gk, score, counts, mrow, mdist = answer(d, [5, 4, 3], [2], 3)
    assert counts.tolist() == [3] and gk[0].tolist() == [5, 3, 4]
    assert score[0, 0] == 2 and np.isposinf(score[0, 1]) and np.isnan(score[0, 2])
    assert np.isnan(mr.matches(mdist, [0, 2], 3, 0)[2, 0])


def test_plus_and_minus_infinity_terms_propagate():
    d = np.array([[INF, -INF, -INF], [-INF, -INF, 5]], F)
    gk, score, counts, _, _ = answer(d, [1, 2, 3], [2], 3)
    assert gk[0].tolist() == [2, 3, 1] and np.isneginf(score[0, :2]).all() and np.isnan(score[0, 2]) and counts[0] == 3   # inf - inf = NaN: last


def test_equal_scores_go_to_the_smaller_key_and_extreme_keys_order_as_int64():
    d = np.array([[1, 2, 2, 1], [2, 1, 1, 2]], F)
    gk, score, counts, _, _ = answer(d, [gr.I64_MAX, -1, gr.I64_MIN, 0], [2], 4)
    assert (score == 3).all() and gk[0].tolist() == [gr.I64_MIN, -1, 0, gr.I64_MAX]


def test_ties_inside_a_group_go_to_the_smaller_row():
    d = np.array([[2, 2, 2], [1, 1, 1]], F)
    _, _, _, mrow, _ = answer(d, [4, 4, 4], [2], 1)
    assert mrow.tolist() == [0, 0]


def test_repeated_and_unknown_candidate_keys():
    d = np.array([[1, 2, 3], [1, 2, 3]], F)
    keys = [10, 20, 30]
    gk, score, counts, _, _ = answer(d, keys, [2], 4, cand_keys=[30, 99, 30, 10, -7, 10])
    assert counts.tolist() == [2] and gk[0].tolist() == [10, 30, 0, 0] and score[0, :2].tolist() == [2, 6]
    gk, _, counts, _, _ = answer(d, keys, [1, 1], 2, cand_keys=[20, 30, 5], cand_offsets=[0, 2, 3])   # per-bag lists; bag 1 names no group
    assert counts.tolist() == [2, 0] and gk.tolist() == [[20, 30], [0, 0]]
    assert answer(d, keys, [2], 2, cand_keys=[])[2].tolist() == [0]


def test_assert_ties_bags_refuses_a_sum_that_may_round():
    mr.assert_ties_bags(np.full((4, 3), 2 ** 21, F), [0, 4])
    with pytest.raises(AssertionError, match="exact range"):
        mr.assert_ties_bags(np.full((9, 3), 2 ** 21, F), [0, 9])
    with pytest.raises(AssertionError, match="grid"):
        mr.assert_ties_bags(np.full((1, 3), 0.5, F), [0, 1])
    mr.assert_ties_bags(np.full((1, 3), 0.5, F), [0, 1], grid=1 / 256)


# ---- planted faults on the model, each caught by the comparator
SIZES = [1, 3, 4, 5, 9, 0]
K = 6


@pytest.fixture(scope="module")
def ties():
    X, Q, d32 = gr.ties_table(0, 257, 8, sum(SIZES), seed=1)
    keys = gr.layouts(257, seed=1)["n / 8 groups"]
    vis = np.ones((sum(SIZES), 257), bool)
    vis[:, ::7] = False
    vis[3, keys == keys[5]] = False   # one group invisible to one vector of the bag of 3 only
    off = mr.bag_offsets(SIZES)
    mr.assert_ties_bags(d32.T, off)
    return d32.T.copy(), vis, keys, off, mr.numpy_multi(d32.T, vis, keys, off, K)


@pytest.fixture(scope="module")
def continuous():
    rng = np.random.default_rng(7)
    d = rng.standard_normal((sum(SIZES), 400)).astype(F) * F(37.0)
    keys = rng.integers(0, 40, 400).astype(np.int64)
    off = mr.bag_offsets(SIZES)
    return d, None, keys, off, mr.numpy_multi(d, None, keys, off, K)


def test_the_true_model_passes(ties, continuous):
    for d, vis, keys, off, truth in (ties, continuous):
        mr.check_multi(truth, d, vis, keys, off, K)
        assert truth[2].max() == K


def pairwise(terms):
    t = [F(x) for x in terms]
    while len(t) > 1:
        t = [F(t[i] + t[i + 1]) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return F(F(0) + t[0])


def test_a_pairwise_or_reversed_sum_is_caught_on_a_continuous_table(continuous):
    d, vis, keys, off, truth = continuous
    for wrong in (pairwise, lambda terms: mr.seq_sum(list(terms)[::-1])):
        got = mr.numpy_multi(d, vis, keys, off, K, summed=wrong)
        with pytest.raises(AssertionError, match="score"):
            mr.same(got, truth)


def test_a_reordered_sum_is_not_seen_on_a_table_of_ties(ties):
    d, vis, keys, off, truth = ties   # (what assert_ties_bags promises: the ties pin everything but the order of the sum)
    mr.same(mr.numpy_multi(d, vis, keys, off, K, summed=pairwise), truth)


def test_minimum_by_distance_with_ties_to_the_larger_row_is_caught(ties):
    d, vis, keys, off, truth = ties

    def larger_row(dv, v, ks):
        return {g: int(np.flatnonzero(v & (ks == g) & (dv == dv[r]))[-1]) for g, r in mr.minima_by_group(dv, v, ks).items()}
    got = mr.numpy_multi(d, vis, keys, off, K, minima=larger_row)
    mr.same(got[:3], truth[:3])   # (scores, keys, counts agree: only the matches tell)
    with pytest.raises(AssertionError, match="match_ids"):
        mr.same(got, truth)


def test_a_non_qualifying_group_admitted_with_its_missing_term_as_zero_is_caught(ties):
    d, vis, keys, off, truth = ties
    d0 = d.copy()
    miss = np.broadcast_to(keys == keys[5], d.shape) & (np.arange(d.shape[0]) == 3)[:, None]
    v2 = vis | miss
    d0[miss] = 0
    with pytest.raises(AssertionError):
        mr.same(mr.numpy_multi(d0, v2, keys, off, K), truth)


def test_ties_by_the_larger_key_are_caught():
    d = np.array([[1, 2, 2, 1, 7], [2, 1, 1, 2, 7]], F)   # four groups at score 3, one at 14
    keys = np.array([5, 6, 7, 8, 9], np.int64)
    truth = answer(d, keys, [2], 3)
    assert truth[0].tolist() == [[5, 6, 7]]
    flipped = answer(d, -keys, [2], 3)   # the same table under the opposite key order: what ties to the LARGER key return
    got = (-flipped[0],) + flipped[1:]
    assert got[0].tolist() == [[8, 7, 6]]
    with pytest.raises(AssertionError, match="group_keys"):
        mr.same(got, truth)


def test_a_repeated_candidate_returned_twice_is_caught(ties):
    d, vis, keys, off, _ = ties
    cand = np.array([keys[0], keys[1], keys[0]], np.int64)
    truth = mr.numpy_multi(d, vis, keys, off, K, cand_keys=cand)
    assert truth[2][0] == 2
    got = [a.copy() for a in truth]
    got[0][0, 2], got[1][0, 2], got[2][0] = got[0][0, 0], got[1][0, 0], 3
    with pytest.raises(AssertionError):
        mr.same(got, truth)


def test_scores_from_minus_zero_are_caught():
    d = np.array([[-0.0, 1.0], [-0.0, 2.0]], F)   # (DOT_PRODUCT of a zero vector: -0.0f)
    truth = answer(d, [1, 2], [2], 2)
    assert not np.signbit(truth[1]).any() and not np.signbit(truth[4]).any()   # +0.0f + -0 = +0; a match distance reads as key_dist does
    got = answer(d, [1, 2], [2], 2, summed=lambda terms: mr.seq_sum(terms, start=F(-0.0)))
    with pytest.raises(AssertionError, match="score"):
        mr.same(got, truth)


@pytest.mark.parametrize("which,pad", [(0, 7), (1, F(0)), (3, 0), (4, F(0))])
def test_unpadded_unused_slots_are_caught(ties, which, pad):
    d, vis, keys, off, _ = ties
    truth = mr.numpy_multi(d, vis, keys, off, K, cand_keys=keys[:3])   # at most 3 groups: slots are unused
    got = [a.copy() for a in truth]
    if which < 2:
        got[which][0, K - 1] = pad
    else:
        got[which][K * off[1] - 1] = pad   # bag 0's last slot
    with pytest.raises(AssertionError, match=mr.NAMES[which]):
        mr.same(got, truth)


def test_the_match_layout_transposed_is_caught(ties):
    d, vis, keys, off, truth = ties
    got = [a.copy() for a in truth]
    for j in range(len(SIZES)):
        lo, t = int(off[j]), SIZES[j]
        got[3][K * lo:K * (lo + t)] = mr.matches(truth[3], off, K, j).T.reshape(-1)
    with pytest.raises(AssertionError, match="match_ids"):
        mr.same(got, truth)


def test_an_id_map_not_applied_to_the_matches_is_caught(ties):
    d, vis, keys, off, truth = ties
    mapped = truth[:3] + (np.where(truth[3] >= 0, truth[3] * 8 + 3, -1), truth[4])
    mr.check_multi(mapped, d, vis, keys, off, K, base=3, stride=8)
    with pytest.raises(AssertionError, match="match_ids"):
        mr.check_multi(truth, d, vis, keys, off, K, base=3, stride=8)


# ---- the host plan
def test_host_plan_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "multi_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "multi_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "multi_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "multi_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower().replace("__hipcc__", "")   # no HIP type in the host header
    assert int(re.search(r"constexpr int64_t MULTI_MAX_BAG = (\d+);", src).group(1)) == 1024
    assert int(re.search(r"constexpr int64_t MULTI_CHUNK = (\d+);", src).group(1)) == 256


# ---- the kernels
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_multi_kernels_use_no_scratch_and_the_figures_design_md_states(tmp_path):
    """the labels, the work list, the gather in its 16-byte and scalar forms, the sum and top-k in five list widths and two forms, the result
    conversion: none with scratch memory - the filter program's 16-entry stack of the gather included.  Static LDS: 32 bytes in the work list's
    scan, none elsewhere (the gather's four vectors are dynamic LDS)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "multi.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "multi.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    count = lambda part: len([k for k in usage if part in k])   # noqa: E731
    assert count("multi_gather_kernel") == 2 and count("multi_sum_topk_kernel") == 10, list(usage)
    for one in ("multi_labels_kernel", "multi_worklist_kernel", "multi_finalize_kernel"):
        assert count(one) == 1, (one, list(usage))
    assert len(usage) == 15, list(usage)   # (and nothing else: no kernel of another unit is compiled again here)
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (k, u)
        lds = u["LDS Size [bytes/block]"]
        if "gather_kernel" in k:
            assert lds == 0 and u["VGPRs"] <= 168 and u["Occupancy [waves/SIMD]"] >= 3, (k, u)   # (a gather hides HBM latency with its wavefronts)
        elif "worklist_kernel" in k:
            assert lds == 32 and u["VGPRs"] <= 80, (k, u)
        else:
            assert lds == 0 and u["VGPRs"] <= 80 and u["Occupancy [waves/SIMD]"] >= 6, (k, u)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.14" in design and "3 wavefronts per SIMD" in design and "at most 80 VGPRs" in design and "32 bytes of static LDS" in design
    unit = open(src).read()
    assert "asm" not in re.sub(r"//.*", "", unit)   # ordinary C++ atomics and stores only


# ---- the entry point: declared, listed, exported, wrapped
def test_symbol_is_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert re.search(r"int32_t eps_index_search_multi\(eps_index\* h, const float\* vectors, const int64_t\* q_offsets, int64_t nq, const int64_t\* cand_keys,\s*"
                     r"const int64_t\* cand_offsets, int64_t n_cand, int32_t k, int64_t scratch_bytes, int64_t\* group_keys_out, float\* score_out,\s*"
                     r"int32_t\* counts_out, int64_t\* match_ids_out, float\* match_dist_out\);", hdr)
    assert re.search(r"eps_index_search_multi\s+\(new\)", hdr)
    lib = C.CDLL(build())
    L = _lib.load()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert "eps_index_search_multi" in _lib.EXPORTS and hasattr(lib, "eps_index_search_multi")
    assert _lib._lib.eps_index_search_multi.restype is i32
    assert list(_lib._lib.eps_index_search_multi.argtypes) == [vp, vp, vp, i64, vp, vp, i64, i32, i64, vp, vp, vp, vp, vp]
    assert L.eps_index_search_multi(None, None, None, 0, None, None, 0, 1, 0, None, None, None, None, None) == 30000   # no handle
    assert '"multi.hip"' in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()


def test_wrapper_rejects_bad_out_buffers_before_any_pointer_reaches_the_library():
    from vectordb_amd.index import GpuIndex, multi_matches
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim = 4
    ix._keep = {}
    bags = [np.zeros((2, 4), F), np.zeros((0, 4), F), np.zeros((3, 4), F)]   # nq = 3, T = 5
    k = 2
    good = (np.empty((3, k), np.int64), np.empty((3, k), F), np.empty(3, np.int32), np.empty(k * 5, np.int64), np.empty(k * 5, F))
    for which, bad in ((0, np.empty((3, k), np.int32)), (0, np.empty((k, 3), np.int64)), (1, np.empty((3, k), np.float64)), (2, np.empty(3, np.int64)),
                       (3, np.empty(k * 5 - 1, np.int64)), (3, np.empty((k, 5), np.int64)), (4, np.empty(k * 5, np.float64)),
                       (4, np.empty(2 * k * 5, F)[::2]), (0, np.empty((3, 2 * k), np.int64)[:, ::2])):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError):
            ix.search_multi(bags, k, out=tuple(out))
    with pytest.raises(ValueError):
        ix.search_multi(bags, k, out=good[:4])   # one buffer short
    with pytest.raises(ValueError):
        ix.search_multi(bags, k, cand_offsets=[0, 0, 0, 0])   # offsets without keys
    with pytest.raises(ValueError):
        ix.search_multi(bags, k, cand_keys=[1, 2], cand_offsets=[0, 1, 2])   # nq + 1 entries are needed
    with pytest.raises(ValueError):
        ix.search_multi((np.zeros((5, 4), F), np.array([0, 3, 2, 5])), k)   # decreasing offsets
    flat = np.arange(k * 5)
    assert multi_matches(flat, [0, 2, 2, 5], k, 0).tolist() == [[0, 1], [2, 3]] and multi_matches(flat, [0, 2, 2, 5], k, 2).tolist() == [[4, 5, 6], [7, 8, 9]]
    assert multi_matches(flat, [0, 2, 2, 5], k, 1).shape == (k, 0)
    ix.h = None
