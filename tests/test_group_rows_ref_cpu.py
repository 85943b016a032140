"""CPU side of GpuIndex.search_group_rows (eps_index_search_group_rows): the model the GPU tests trust (tests/group_rows_ref.py) against
hand-written cases and planted faults; the symbol declared, listed and exported; csrc/group_rows.hip compiled for gfx950 with its registers,
scratch (none) and LDS recorded; the host plan (csrc/group_rows_host.hpp) through its stand-alone check under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import group_rows_ref as grr
import groups_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def col(*d):
    return np.array(d, F)[:, None]


# ---- hand-written cases: one query, distances given
#            row:  0  1  2  3  4  5  6  7
D = col(5, 1, 3, 1, 2, 9, 0, 2)
KEYS = np.array([7, 7, 8, 9, 8, -3, 9, 7], np.int64)
# group 9: rows 6 (0), 3 (1); group 7: rows 1 (1), 7 (2), 0 (5); group 8: rows 4 (2), 2 (3); group -3: row 5 (9)


def test_m_above_the_groups_size_and_m_of_one():
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(D, KEYS, 3, 4)
    assert gk.tolist() == [[9, 7, 8]] and rc.tolist() == [[2, 3, 2]] and gs.tolist() == [[2, 3, 2]] and cnt.tolist() == [3]
    assert ids.tolist() == [[[6, 3, -1, -1], [1, 7, 0, -1], [4, 2, -1, -1]]]
    assert dist[0, 1, :3].tolist() == [1, 2, 5] and np.isposinf(dist[0, 0, 2:]).all() and np.isposinf(dist[0, 1, 3])
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(D, KEYS, 3, 1)   # m = 1: the representatives of search_groups
    g = gr.numpy_groups(D, KEYS, 3)
    assert np.array_equal(ids[:, :, 0], g[0]) and np.array_equal(dist[:, :, 0], g[1]) and np.array_equal(gk, g[2]) and np.array_equal(cnt, g[3])
    assert rc.tolist() == [[1, 1, 1]] and gs.tolist() == [[2, 3, 2]]   # the size counts every visible row, kept or not
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(D, KEYS, 2, 2)   # m below a group's size: cut at m, in key order
    assert ids.tolist() == [[[6, 3], [1, 7]]] and rc.tolist() == [[2, 2]] and gs.tolist() == [[2, 3]]


def test_k_above_the_number_of_groups_pads_whole_slots():
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(D, KEYS, 6, 2)
    assert cnt.tolist() == [4] and gk.tolist() == [[9, 7, 8, -3, 0, 0]] and rc.tolist() == [[2, 2, 2, 1, 0, 0]] and gs.tolist() == [[2, 3, 2, 1, 0, 0]]
    assert (ids[0, 4:] == -1).all() and np.isposinf(dist[0, 4:]).all() and ids[0, 3].tolist() == [5, -1]


def test_an_invisible_group_and_a_deleted_representative():
    vis = np.ones(8, bool)
    vis[[6, 3]] = False   # group 9 entirely invisible: no group of this query
    vis[1] = False        # group 7's representative deleted: row 7 takes over, the size drops to 2
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(D, KEYS, 4, 3, visible=vis)
    assert gk.tolist() == [[8, 7, -3, 0]] and cnt.tolist() == [3]
    assert ids.tolist() == [[[4, 2, -1], [7, 0, -1], [5, -1, -1], [-1, -1, -1]]] and gs.tolist() == [[2, 2, 1, 0]]


def test_a_group_visible_only_through_nan_rows_and_nan_last_inside_a_group():
    d = col(NAN, 2, INF, NAN, NAN, -0.0, NAN)
    keys = np.array([1, 1, 2, 3, 3, 4, 2], np.int64)
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(d, keys, 5, 3)
    assert gk.tolist() == [[4, 1, 2, 3, 0]] and cnt.tolist() == [4] and rc.tolist() == [[1, 2, 2, 2, 0]]
    assert ids.tolist() == [[[5, -1, -1], [1, 0, -1], [2, 6, -1], [3, 4, -1], [-1, -1, -1]]]   # NaN after +inf, NaN ties to the smaller row
    assert np.isnan(dist[0, 1, 1]) and np.isposinf(dist[0, 2, 0]) and np.isnan(dist[0, 3, :2]).all()
    grr.same((ids, dist, gk, rc, gs, cnt), tuple(a.copy() for a in (ids, dist, gk, rc, gs, cnt)))   # a NaN equals a NaN


def test_equal_distances_inside_a_group_go_to_the_smaller_row():
    d = col(4, 4, 4, 4, 4, 4, 4)
    keys = np.array([30, 10, 30, 20, 10, 30, 30], np.int64)
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(d, keys, 3, 3)
    assert gk.tolist() == [[30, 10, 20]] and ids.tolist() == [[[0, 2, 5], [1, 4, -1], [3, -1, -1]]] and gs.tolist() == [[4, 2, 1]]


def test_a_visibility_per_query_gives_sizes_per_query():
    d = np.array([[1, 9], [2, 8], [3, 7], [4, 6]], F)
    keys = np.array([5, 5, 5, 6], np.int64)
    vis = np.array([[1, 0], [1, 1], [1, 0], [1, 1]], bool)   # (a program on @distance judges per query)
    ids, dist, gk, rc, gs, cnt = grr.numpy_group_rows(d, keys, 2, 2, visible=vis)
    assert gs.tolist() == [[3, 1], [1, 1]] and gk.tolist() == [[5, 6], [6, 5]] and ids[1].tolist() == [[3, -1], [1, -1]]


# ---- planted faults on the model's output, each caught by `same`; the true model passes the same check
@pytest.fixture(scope="module")
def case():
    n, nq = 400, 6
    X, Q, d32 = gr.ties_table(0, n, 8, nq, seed=3)   # dim 8, coordinates -8..8: many equal distances
    keys = gr.layouts(n, seed=3)["n / 8 groups"] * 7 - 100
    vis = np.random.default_rng(3).random(n) < 0.7
    return d32, keys, vis


K, M = 7, 5


@pytest.fixture(scope="module")
def truth(case):
    d32, keys, vis = case
    ans = grr.numpy_group_rows(d32, keys, K, M, vis)
    assert (ans[3] == M).any() and (ans[4] > M).any() and (ans[3] < M).any()   # groups cut at m and groups below m both occur
    return ans


def copy(ans):
    return [a.copy() for a in ans]


def test_the_true_model_passes(case, truth):
    d32, keys, vis = case
    grr.check_group_rows(truth, d32, keys, K, M, vis)
    for k, m in ((1, 1), (64, 2), (7, 64)):
        grr.check_group_rows(grr.numpy_group_rows(d32, keys, k, m, vis), d32, keys, k, m, vis)


def test_the_mth_row_lost_at_a_chunk_boundary_is_caught(case, truth):
    d32, keys, vis = case
    got = copy(truth)
    q, s = np.argwhere(truth[3] == M)[0]
    got[0][q, s, M - 1], got[1][q, s, M - 1] = -1, INF   # the last row of a full group never arrived ...
    got[3][q, s] = M - 1                                 # ... and the count agrees with what did
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(got, d32, keys, K, M, vis)


def test_rows_ordered_by_row_inside_a_group_are_caught(case, truth):
    d32, keys, vis = case
    got = copy(truth)
    changed = False
    for q, s in np.argwhere(truth[3] > 1):
        c = truth[3][q, s]
        o = np.argsort(truth[0][q, s, :c])
        got[0][q, s, :c], got[1][q, s, :c] = truth[0][q, s, :c][o], truth[1][q, s, :c][o]
        changed |= not np.array_equal(o, np.arange(c))
    assert changed
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(got, d32, keys, K, M, vis)


def test_ties_to_the_larger_row_are_caught(case):
    d32, _, vis = case
    keys = gr.layouts(400, seed=3)["extreme keys"]   # four groups of about a hundred rows: equal distances inside every group
    k, m = 3, 40
    truth = grr.numpy_group_rows(d32, keys, k, m, vis)
    got = copy(truth)
    swapped = 0
    for q, s in np.argwhere(truth[3] > 1):
        for e in range(truth[3][q, s] - 1):
            if gr.bits(got[1][q, s, e]) == gr.bits(got[1][q, s, e + 1]):
                got[0][q, s, e], got[0][q, s, e + 1] = got[0][q, s, e + 1], got[0][q, s, e]
                swapped += 1
                break
    assert swapped, "no tie inside a group in this table: pick another seed"
    grr.check_group_rows(truth, d32, keys, k, m, vis)
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(got, d32, keys, k, m, vis)


def test_slot_zero_not_the_representative_is_caught(case, truth):
    d32, keys, vis = case
    got = copy(truth)
    q, s = np.argwhere(truth[3] > 1)[0]
    got[0][q, s, [0, 1]], got[1][q, s, [0, 1]] = truth[0][q, s, [1, 0]], truth[1][q, s, [1, 0]]
    assert got[0][q, s, 0] != gr.numpy_groups(d32, keys, K, vis)[0][q, s]
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(got, d32, keys, K, M, vis)


def test_sizes_that_count_invisible_rows_are_caught(case, truth):
    d32, keys, vis = case
    got = copy(truth)
    all_rows = grr.numpy_group_rows(d32, keys, 400, 1)   # every group, every row visible: the groups' full sizes
    full = {int(g): int(z) for g, z in zip(all_rows[2][0], all_rows[4][0])}
    got[4] = np.array([[full[int(g)] if c else 0 for g, c in zip(gq, cq)] for gq, cq in zip(truth[2], truth[3])], np.int64)
    assert (got[4] != truth[4]).any()
    with pytest.raises(AssertionError, match="group_sizes"):
        grr.check_group_rows(got, d32, keys, K, M, vis)


def test_row_counts_not_clipped_to_m_are_caught(case, truth):
    d32, keys, vis = case
    got = copy(truth)
    got[3] = truth[4].astype(np.int32)
    with pytest.raises(AssertionError, match="row_counts"):
        grr.check_group_rows(got, d32, keys, K, M, vis)


def test_a_row_of_group_k_plus_one_leaking_in_is_caught(case, truth):
    d32, keys, vis = case
    more = grr.numpy_group_rows(d32, keys, K + 1, M, vis)
    assert (more[5] == K + 1).all()
    got = copy(truth)
    q, s = np.argwhere(truth[3] < M)[0]   # a group with a free slot takes the next group's representative
    c = truth[3][q, s]
    got[0][q, s, c], got[1][q, s, c] = more[0][q, K, 0], more[1][q, K, 0]
    got[3][q, s] += 1
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(got, d32, keys, K, M, vis)
    with pytest.raises(AssertionError, match="shape"):   # ... or the whole group as a slot of its own
        grr.check_group_rows(more, d32, keys, K, M, vis)


@pytest.mark.parametrize("which, pad", [(0, 0), (1, 0.0), (2, -1), (3, -1), (4, -1)])
def test_unused_slots_not_padded_are_caught(case, which, pad):
    d32, keys, vis = case
    truth = grr.numpy_group_rows(d32, keys, 64, M, vis)   # k above the visible groups: whole slots unused
    assert (truth[5] < 64).all() and (truth[3] < M).any()
    got = copy(truth)
    free = truth[0] == -1 if which < 2 else truth[3] == 0
    got[which][free] = pad
    with pytest.raises(AssertionError, match=grr.NAMES[which]):
        grr.check_group_rows(got, d32, keys, 64, M, vis)


def test_groups_ordered_by_key_not_by_representative_are_caught(case, truth):
    d32, keys, vis = case
    got = copy(truth)
    for q in range(len(truth[5])):
        o = np.argsort(truth[2][q], kind="stable")
        for a in range(5):
            got[a][q] = truth[a][q][o]
    assert not np.array_equal(got[2], truth[2])
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(got, d32, keys, K, M, vis)


def test_an_id_map_is_undone_by_the_check(case, truth):
    d32, keys, vis = case
    grr.check_group_rows(grr.mapped(truth, 3, 8), d32, keys, K, M, vis, base=3, stride=8)
    with pytest.raises(AssertionError, match="ids"):
        grr.check_group_rows(truth, d32, keys, K, M, vis, base=3, stride=8)


# ---- the host plan
def test_host_plan_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "group_rows_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "group_rows_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "group_rows_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "group_rows_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()   # no HIP type in the host header
    assert int(re.search(r"constexpr int32_t GROUP_ROWS_MAX_M = (\d+);", src).group(1)) == 1024
    assert int(re.search(r"constexpr int64_t GROUP_ROWS_MAX_ANSWER = (\d+);", src).group(1)) == 65536


# ---- the kernels
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_group_rows_kernels_use_no_scratch_and_the_lds_design_md_states(tmp_path):
    """the three set-up kernels, the work list, the gather in five list widths and its 16-byte and scalar forms, five widths of the merge and the
    result conversion: none with scratch memory - the filter program's 16-entry stack of the gather included.  Static LDS: 16 bytes in the two
    one-workgroup scans, 4 * 64 * KPL * 8 bytes in the merge, none in the gather (its query is dynamic LDS: the dimension, rounded up to 4 floats)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "group_rows.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "group_rows.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    assert count("group_rows_gather_kernel") == 10 and count("group_rows_merge_kernel") == 5, list(usage)
    for one in ("group_rows_hist_kernel", "group_rows_offsets_kernel", "group_rows_scatter_kernel", "group_rows_worklist_kernel", "group_rows_finalize_kernel"):
        assert count(one) == 1, (one, list(usage))
    assert len(usage) == 20, list(usage)   # (and nothing else: no kernel of another unit is compiled again here)
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256, (k, u)
        lds = u["LDS Size [bytes/block]"]
        if "gather_kernel" in k:
            assert lds == 0 and u["Occupancy [waves/SIMD]"] >= 2, (k, u)   # (a gather hides HBM latency with its wavefronts)
        elif "merge_kernel" in k:
            kpl = int(re.search(r"merge_kernelILi(\d+)E", k).group(1))
            assert lds == 4 * 64 * kpl * 8, (k, u)
        elif "offsets_kernel" in k or "worklist_kernel" in k:
            assert lds == 16, (k, u)
        else:
            assert lds == 0, (k, u)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4 x 64 x KPL x 8 bytes" in design and "3.13" in design
    unit = open(src).read()
    assert "asm" not in re.sub(r"//.*", "", unit)   # ordinary C++ atomics and stores only


# ---- the entry point: declared, listed, exported, wrapped
def test_symbol_is_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert re.search(r"int32_t eps_index_search_group_rows\(eps_index\* h, const float\* queries, int64_t nq, int32_t k, int32_t m, const eps_search_params\* p, "
                     r"int32_t engine,\s*int32_t page_rows, int64_t scratch_bytes, int64_t\* ids_out, float\* dist_out, int64_t\* group_keys_out,\s*"
                     r"int32_t\* row_counts_out, int64_t\* group_sizes_out, int32_t\* counts_out\);", hdr)
    lib = C.CDLL(build())
    L = _lib.load()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert "eps_index_search_group_rows" in _lib.EXPORTS and hasattr(lib, "eps_index_search_group_rows")
    assert _lib._lib.eps_index_search_group_rows.restype is i32
    assert list(_lib._lib.eps_index_search_group_rows.argtypes) == [vp, vp, i64, i32, i32, C.POINTER(_lib.SearchParams), i32, i32, i64, vp, vp, vp, vp, vp, vp]
    assert L.eps_index_search_group_rows(None, None, 0, 1, 1, None, 0, 0, 0, None, None, None, None, None, None) == 30000   # no handle
    assert '"group_rows.hip"' in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()


def test_the_wrapper_exists():
    from vectordb_amd.index import GpuIndex
    assert callable(getattr(GpuIndex, "search_group_rows", None))


def test_wrapper_rejects_bad_out_buffers_before_any_pointer_reaches_the_library():
    from vectordb_amd.index import GpuIndex
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim = 4
    ix._keep = {}
    Q = np.zeros((3, 4), F)
    good = (np.empty((3, 5, 2), np.int64), np.empty((3, 5, 2), F), np.empty((3, 5), np.int64), np.empty((3, 5), np.int32), np.empty((3, 5), np.int64),
            np.empty(3, np.int32))
    for which, bad in ((0, np.empty((3, 5, 2), np.int32)), (0, np.empty((3, 5), np.int64)), (1, np.empty((3, 2, 5), F)), (2, np.empty((3, 5), F)),
                       (3, np.empty((3, 5), np.int64)), (4, np.empty((3, 5), np.int32)), (5, np.empty(3, np.int64)),
                       (0, np.empty((3, 5, 4), np.int64)[:, :, ::2]), (4, np.empty((3, 10), np.int64)[:, ::2])):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError):
            ix.search_group_rows(Q, 5, 2, out=tuple(out))
    with pytest.raises(ValueError):
        ix.search_group_rows(Q, 5, 2, out=good[:5])   # one buffer short
    with pytest.raises(KeyError):
        ix.search_group_rows(Q, 5, 2, engine="walk")
    ix.h = None
