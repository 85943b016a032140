"""CPU side of GpuIndex.search_groups (eps_index_search_groups): the model the GPU tests trust (tests/groups_ref.py) against hand-written cases
and planted faults; the three symbols declared, listed and exported; csrc/groups.hip compiled for gfx950 with its registers, scratch (none) and
LDS recorded; the host side (csrc/groups_host.hpp) through its stand-alone check under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import groups_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def col(*d):
    return np.array(d, F)[:, None]


# ---- hand-written cases: one query, distances given
def test_hand_written_cases():
    #            row:  0  1  2  3  4  5  6  7
    d = col(5, 1, 3, 1, 2, 9, 0, 2)
    keys = np.array([7, 7, 8, 9, 8, -3, 9, 7], np.int64)
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 3)
    # group 9: rows 3, 6 -> row 6 (0); group 7: rows 0, 1, 7 -> row 1 (1); group 8: rows 2, 4 -> row 4 (2); group -3: row 5 (9)
    assert ids.tolist() == [[6, 1, 4]] and dist.tolist() == [[0, 1, 2]] and gk.tolist() == [[9, 7, 8]] and cnt.tolist() == [3]
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 6)   # k beyond the groups: padding -1 / +inf / key 0, the count says which slots are used
    assert ids.tolist() == [[6, 1, 4, 5, -1, -1]] and gk.tolist() == [[9, 7, 8, -3, 0, 0]] and cnt.tolist() == [4] and np.isposinf(dist[0, 4:]).all()
    vis = np.ones(8, bool)
    vis[[6, 1]] = False   # two representatives deleted: the groups' next rows take over (row 3 at 1, row 7 at 2)
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 4, visible=vis)
    assert ids.tolist() == [[3, 4, 7, 5]] and dist.tolist() == [[1, 2, 2, 9]] and gk.tolist() == [[9, 8, 7, -3]]
    vis[[3]] = False      # group 9 entirely invisible: it is no group of this query
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 4, visible=vis)
    assert ids.tolist() == [[4, 7, 5, -1]] and cnt.tolist() == [3]
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 4, visible=np.zeros(8, bool))
    assert cnt.tolist() == [0] and (ids == -1).all() and (gk == 0).all()


def test_ties_go_to_the_smaller_row_inside_and_across_groups():
    d = col(4, 4, 4, 4, 4, 4)
    keys = np.array([30, 10, 30, 20, 10, 20], np.int64)
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 3)
    assert ids.tolist() == [[0, 1, 3]] and gk.tolist() == [[30, 10, 20]]   # by row, not by key or label


def test_nan_sorts_after_inf_and_a_group_of_nans_is_still_a_group():
    d = col(NAN, 2, INF, NAN, NAN, -0.0)
    keys = np.array([1, 1, 2, 3, 3, 4], np.int64)
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 5)
    assert ids.tolist() == [[5, 1, 2, 3, -1]] and cnt.tolist() == [4] and np.isnan(dist[0, 3]) and gk.tolist() == [[4, 1, 2, 3, 0]]
    gr.same((ids, dist, gk, cnt), (ids.copy(), dist.copy(), gk.copy(), cnt.copy()))   # a NaN equals a NaN


def test_extreme_keys_and_a_visibility_per_query():
    d = np.array([[1, 9], [2, 8], [3, 7], [4, 6]], F)
    keys = np.array([gr.I64_MIN, gr.I64_MAX, gr.I64_MIN, 0], np.int64)
    vis = np.array([[1, 0], [1, 1], [1, 1], [1, 1]], bool)   # (a program that reads @distance judges per query)
    ids, dist, gk, cnt = gr.numpy_groups(d, keys, 2, visible=vis)
    assert ids.tolist() == [[0, 1], [3, 2]] and gk.tolist() == [[gr.I64_MIN, gr.I64_MAX], [0, gr.I64_MIN]]


def test_ties_tables_are_checked_before_use():
    for metric in (0, 1, 2):
        X, Q, d32 = gr.ties_table(metric, 200, 20, 5, seed=metric)
        assert d32.shape == (200, 5)
    rng = np.random.default_rng(0)
    with pytest.raises(AssertionError, match="not a table of ties"):
        gr.assert_ties_table(rng.random((50, 8), dtype=F), rng.random((2, 8), dtype=F), 0)
    with pytest.raises(AssertionError, match="not a table of ties"):
        gr.assert_ties_table(np.full((4, 8), 9, F), np.zeros((1, 8), F), 0)


def test_layouts_are_what_they_are_called():
    lay = gr.layouts(3000, seed=1)
    assert len(np.unique(lay["one group"])) == 1 and len(np.unique(lay["every row its own"])) == 3000
    assert 300 <= len(np.unique(lay["n / 8 groups"])) <= 375
    sizes = np.unique(lay["zipf"], return_counts=True)[1]
    assert sizes.max() > 500 and (sizes == 1).sum() > 50
    assert set(lay["extreme keys"].tolist()) == {gr.I64_MIN, -1, 0, gr.I64_MAX}
    assert gr.layouts(1)["zipf"].shape == (1,)


# ---- planted faults: an engine with the fault answers, check_groups refuses; the true model passes the same check
@pytest.fixture(scope="module")
def case():
    n, nq = 400, 6
    X, Q, d32 = gr.ties_table(0, n, 8, nq, seed=3)   # dim 8, coordinates -8..8: many equal distances
    keys = gr.layouts(n, seed=3)["n / 8 groups"] * 7 - 100
    vis = np.random.default_rng(3).random(n) < 0.7
    return d32, keys, vis


def faulty(d32, keys, k, vis, rep=None, order=None, hide_group_of_deleted=False, nan_first=False, full_count=False, pad_key=None, dist_for_filter=None):
    """the rule with one thing done wrong; rows in answer order per query, then packed like an answer"""
    n, nq = d32.shape
    v2 = gr.rr.visible2(n, nq, vis)
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F)
    gk = np.zeros((nq, k), np.int64) if pad_key is None else np.full((nq, k), pad_key, np.int64)
    cnt = np.zeros(nq, np.int32)
    labels = np.unique(keys, return_inverse=True)[1]
    for q in range(nq):
        d = d32[:, q]
        rows = np.flatnonzero(v2[:, q])
        if hide_group_of_deleted:   # a group whose overall closest row is hidden disappears
            best = {}
            for r in np.arange(n)[gr.key_order(d, np.arange(n))].tolist():
                best.setdefault(int(keys[r]), r)
            rows = np.array([r for r in rows.tolist() if v2[best[int(keys[r])], q]], np.int64)
        reps = []
        for g in np.unique(keys[rows]):
            mine = rows[keys[rows] == g]
            if rep == "smallest id":
                reps.append(mine.min())
            elif nan_first:
                dd = np.where(np.isnan(d[mine]), -np.inf, d[mine])
                reps.append(mine[np.lexsort((mine, dd))[0]])
            else:
                reps.append(mine[gr.key_order(d[mine], mine)[0]])
        reps = np.array(reps, np.int64)
        if order == "label":
            o = np.lexsort((labels[reps], d[reps]))
        elif nan_first:
            o = np.lexsort((reps, np.where(np.isnan(d[reps]), -np.inf, d[reps])))
        else:
            o = gr.key_order(d[reps], reps)
        a = reps[o][:k]
        m = len(a)
        ids[q, :m], dist[q, :m], gk[q, :m] = a, d[a], keys[a]
        cnt[q] = k if full_count else m
    return ids, dist, gk, cnt


def test_the_true_model_passes(case):
    d32, keys, vis = case
    for k in (1, 7, 64):
        gr.check_groups(gr.numpy_groups(d32, keys, k, vis), d32, keys, k, vis)
        gr.check_groups(faulty(d32, keys, k, vis), d32, keys, k, vis)   # (the fault-free setting of the faulty engine is the model)


def test_representative_by_smallest_id_is_caught(case):
    d32, keys, vis = case
    with pytest.raises(AssertionError, match="ids|dist"):
        gr.check_groups(faulty(d32, keys, 7, vis, rep="smallest id"), d32, keys, 7, vis)


def test_ties_between_groups_broken_by_label_are_caught(case):
    d32, keys, vis = case
    perm = np.random.default_rng(1).permutation(keys.max() - keys.min() + 1)
    keys2 = perm[keys - keys.min()].astype(np.int64)   # labels in no relation to rows
    got = faulty(d32, keys2, 64, vis, order="label")
    assert not np.array_equal(got[0], gr.numpy_groups(d32, keys2, 64, vis)[0]), "no tie between groups in this table: pick another seed"
    with pytest.raises(AssertionError, match="ids"):
        gr.check_groups(got, d32, keys2, 64, vis)


def test_a_deleted_representative_hiding_its_group_is_caught(case):
    d32, keys, vis = case
    with pytest.raises(AssertionError, match="ids|counts"):
        gr.check_groups(faulty(d32, keys, 64, vis, hide_group_of_deleted=True), d32, keys, 64, vis)


def test_a_nan_row_taken_as_closest_is_caught(case):
    d32, keys, vis = case
    d = d32.copy()
    d[np.flatnonzero(vis)[::9]] = NAN
    gr.check_groups(gr.numpy_groups(d, keys, 7, vis), d, keys, 7, vis)
    with pytest.raises(AssertionError, match="ids|dist"):
        gr.check_groups(faulty(d, keys, 7, vis, nan_first=True), d, keys, 7, vis)


def test_a_count_of_k_where_fewer_groups_exist_is_caught(case):
    d32, keys, vis = case
    assert len(np.unique(keys[vis])) < 64
    with pytest.raises(AssertionError, match="counts"):
        gr.check_groups(faulty(d32, keys, 64, vis, full_count=True), d32, keys, 64, vis)


def test_a_padding_key_taken_for_a_group_is_caught(case):
    d32, keys, vis = case
    with pytest.raises(AssertionError, match="group_keys"):
        gr.check_groups(faulty(d32, keys, 64, vis, pad_key=-1), d32, keys, 64, vis)
    # ... and a real group whose key IS 0 is told from padding by the count alone
    k0 = keys - keys[np.flatnonzero(vis)[0]]
    ids, dist, gk, cnt = gr.numpy_groups(d32, k0, 64, vis)
    assert all((gk[q, :cnt[q]] == 0).sum() == 1 for q in range(len(cnt)))


def test_at_distance_read_as_zero_is_caught(case):
    d32, keys, _ = case
    t = F(np.sort(d32, axis=0)[60].min())
    vis = d32 <= t                       # `@distance <= t`, judged per (row, query)
    vis0 = np.zeros_like(d32) <= t       # the same program with @distance read as 0: every row passes
    got = gr.numpy_groups(d32, keys, 64, vis0)
    gr.check_groups(gr.numpy_groups(d32, keys, 64, vis), d32, keys, 64, vis)
    with pytest.raises(AssertionError, match="ids|counts"):
        gr.check_groups(got, d32, keys, 64, vis)


def test_an_id_map_is_undone_by_the_check(case):
    d32, keys, vis = case
    ids, dist, gk, cnt = gr.numpy_groups(d32, keys, 7, vis)
    gr.check_groups((np.where(ids >= 0, ids * 8 + 3, -1), dist, gk, cnt), d32, keys, 7, vis, base=3, stride=8)
    with pytest.raises(AssertionError, match="ids"):
        gr.check_groups((ids, dist, gk, cnt), d32, keys, 7, vis, base=3, stride=8)


# ---- the entry points: declared, listed, exported
def test_symbols_are_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert re.search(r"int32_t eps_index_set_groups\(eps_index\* h, const int64_t\* keys, int64_t n\);", hdr)
    assert re.search(r"int32_t eps_index_search_groups\(eps_index\* h, const float\* queries, int64_t nq, int32_t k, const eps_search_params\* p, int32_t engine, "
                     r"int32_t page_rows,\s*int64_t scratch_bytes, int64_t\* ids_out, float\* dist_out, int64_t\* group_keys_out, int32_t\* counts_out\);", hdr)
    assert re.search(r"int32_t eps_index_groups_info\(eps_index\* h, int64_t\* n_groups, int64_t\* largest_group, int32_t\* last_engines, int64_t\* last_scan_queries\);", hdr)
    assert "aggregation.hpp" in hdr and "#define EPS_GROUPS_AUTO 0" in hdr and "#define EPS_GROUPS_PAGES 1" in hdr and "#define EPS_GROUPS_SCAN 2" in hdr
    lib = C.CDLL(build())
    L = _lib.load()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    for name in ("eps_index_set_groups", "eps_index_search_groups", "eps_index_groups_info"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(_lib._lib, name).restype is i32
    assert list(_lib._lib.eps_index_set_groups.argtypes) == [vp, vp, i64]
    assert list(_lib._lib.eps_index_search_groups.argtypes) == [vp, vp, i64, i32, C.POINTER(_lib.SearchParams), i32, i32, i64, vp, vp, vp, vp]
    assert L.eps_index_set_groups(None, None, 0) == 30000   # no handle
    assert L.eps_index_search_groups(None, None, 0, 1, None, 0, 0, 0, None, None, None, None) == 30000
    assert L.eps_index_groups_info(None, None, None, None, None) == 30000
    assert '"groups.hip"' in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "groups_host.hpp")).read()
    assert int(re.search(r"constexpr int32_t GROUPS_MAX_K = (\d+);", src).group(1)) == 1024
    assert "hip" not in re.sub(r"//.*", "", src).lower()   # no HIP type in the host header
    unit = open(os.path.join(ROOT, "vectordb_amd", "csrc", "groups.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", unit)   # ordinary C++ atomics only


def test_wrapper_checks_before_any_pointer_reaches_the_library():
    from vectordb_amd.index import GpuIndex
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim = 4
    ix._keep = {}
    Q = np.zeros((3, 4), F)
    good = (np.empty((3, 5), np.int64), np.empty((3, 5), F), np.empty((3, 5), np.int64), np.empty(3, np.int32))
    for which, bad in ((0, np.empty((3, 5), np.int32)), (1, np.empty((3, 4), F)), (2, np.empty((3, 5), F)), (3, np.empty(3, np.int64)),
                       (2, np.empty((3, 10), np.int64)[:, ::2])):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError):
            ix.search_groups(Q, 5, out=tuple(out))
    with pytest.raises(KeyError):
        ix.search_groups(Q, 5, engine="walk")
    ix.h = None


# ---- the kernels
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_groups_kernels_use_no_scratch_and_fit_the_lds_budget(tmp_path):
    """the page kernel (two 4096-slot tables in LDS), the compaction, the gather, the scan in its 16-byte and scalar forms, five widths of the
    read-back, the scatter and the key look-up: none with scratch memory - the filter program's 16-entry stack of the scan included - and
    static LDS inside 64 KB"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "groups.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "groups.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    assert count("groups_first_kernel") == 1 and count("groups_min_scan_kernel") == 2 and count("groups_table_topk_kernel") == 5, list(usage)
    assert count("groups_compact_kernel") == 1 and count("groups_gather_kernel") == 1 and count("groups_scatter_kernel") == 1 and count("groups_keys_kernel") == 1
    assert len(usage) == 12, list(usage)   # (and nothing else: no kernel of another unit is compiled again here)
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256 and u["LDS Size [bytes/block]"] <= 65536, (k, u)
        if "groups_min_scan_kernel" in k:
            assert u["Occupancy [waves/SIMD]"] >= 2, (k, u)   # (the scan hides HBM latency with its wavefronts)
        if "groups_first_kernel" in k:
            assert 32768 <= u["LDS Size [bytes/block]"] <= 33792, (k, u)   # labels + positions of 4096 slots, the wavefronts' counts


def test_host_side_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "groups_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "groups_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "groups_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
