"""CPU side of GpuSparseIndex (eps_sparse_index_*): the sequential model the GPU tests trust (tests/sparse_ref.py) reproduces the reference's own
bits on every pair of the golden fixture; on tables of ties it equals the dense numpy result and fp64; the conditions the GPU tests lean on are
asserted; planted faults are caught by the comparator; the symbols are declared, listed and exported; csrc/sparse.hip compiles for gfx950 without
scratch memory and within the LDS the plan promises; the host planning (csrc/sparse_host.hpp) passes its stand-alone check under the address and
undefined-behaviour sanitizers.

tests/golden/sparse_reference_distances.npz was recorded once: the reference's engine/db/vector.cpp and engine/utils/json.cpp compiled with
`g++ -std=c++17 -O3 -I engine` (no -march, so no fused multiply-add) and linked with a driver that reads the CSR of sparse_ref.fixture_tables() and
writes GetL2DistSqr(row, query), GetCosineDist(row, query), GetInnerProductDist(row, query) for every pair; `bits[row, query, metric]` holds their
uint32 images.  Neither the driver nor anything compiled from the reference is part of the repository."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sparse_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_reference_distances.npz")
METRICS = (sr.L2, sr.COSINE, sr.DOT)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    X = (z["x_offsets"], z["x_indices"], z["x_values"])
    Q = (z["q_offsets"], z["q_indices"], z["q_values"])
    return X, Q, z["bits"]


# ---- the model is the reference
def test_the_fixture_holds_what_it_should(golden):
    X, Q, ref = golden
    Xf, Qf = sr.fixture_tables()
    for a, b in zip(X + Q, Xf + Qf):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    n, nq = sr.n_rows(X), sr.n_rows(Q)
    assert ref.shape == (n, nq, 3) and ref.dtype == np.uint32 and n == 300 + len(sr.hand_vectors()) and nq == 7 + len(sr.hand_vectors())
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert X[1].max() == 2 ** 31 - 2 and X[1].min() == 0
    lens = np.diff(X[0])
    assert lens.min() == 0 and lens.max() == 60 and np.diff(Q[0]).min() == 0 and 20 <= np.diff(Q[0]).max() <= 40


def test_the_model_equals_the_reference_on_every_pair(golden):
    X, Q, ref = golden
    nan = 0
    for metric in METRICS:
        got = sr.dist_table(X, Q, metric)
        want = ref[:, :, metric].view(F)
        assert np.array_equal(np.isnan(got), np.isnan(want)), metric
        nan += int(np.isnan(want).sum())
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (metric, int((got[ok].view(np.uint32) != want[ok].view(np.uint32)).sum()))
    assert nan > 0   # an empty row or query under COSINE


def test_the_fixture_tells_a_fused_multiply_add(golden):
    X, Q, ref = golden
    for metric in (sr.L2, sr.DOT):
        fused = sr.dist_table(X, Q, metric, fma=True)
        assert (sr.bits(fused) != sr.bits(ref[:, :, metric].view(F))).sum() > 100


# ---- tables of ties
@pytest.mark.parametrize("metric", METRICS)
def test_ties_tables_model_equals_dense_and_fp64(metric):
    X, Q = sr.ties_table(257, 9, seed=3 + metric)
    seq = sr.dist_table(X, Q, metric)
    d32 = sr.dist_dense(X, Q, metric, F)
    d64 = sr.dist_dense(X, Q, metric, np.float64)
    assert np.array_equal(sr.bits(seq), sr.bits(d32))
    if metric == sr.COSINE:
        # dot and norms are exact integers; the epilogue is three correctly rounded fp32 operations, which fp64 would round differently
        assert np.isnan(d32).any() and np.array_equal(np.isnan(d32), np.isnan(d64))
        ok = ~np.isnan(d32)
        assert np.allclose(d32[ok], d64[ok], rtol=0, atol=4e-7)
        Xd, Qd = sr.dense_images(X, Q, np.float64)
        assert np.array_equal((sr.dense_images(X, Q, F)[0] @ sr.dense_images(X, Q, F)[1].T).astype(np.float64), Xd @ Qd.T)
    else:
        assert np.array_equal(d32.astype(np.float64), d64)
    # the table is what it claims: stored zeros, the two ends of the index range, empty rows, ties
    assert (X[2] == 0).any() and X[1].min() == 0 and X[1].max() == sr.DIM_MAX - 1 and (np.diff(X[0]) == 0).any() and np.diff(X[0]).max() <= 40
    assert all(len(np.unique(sr.bits(d32[:, j]))) < 257 for j in range(9))


def test_piece_table_has_every_edge_length():
    P, qmax = sr.host_constant("SPARSE_PIECE"), sr.host_constant("SPARSE_MAX_QUERY_NNZ")
    assert qmax >= 4096
    lens = sr.piece_lengths()
    assert len(lens) == 130
    for want in (P - 1, P, P + 1, 2 * P + 3):
        assert want in lens, want
    assert lens[0] == P - 1 and lens[129] == 2 * P + 3          # first and last
    assert lens[9] == P + 1 and max(lens[1:9]) < 16               # between short rows
    # rows 64 .. 68 start a wavefront's round; their ends fall on multiples of the piece
    ends = np.cumsum(lens[64:69])
    assert ends.tolist() == [P, P + 200, 2 * P, 2 * P, 4 * P]
    X, Q = sr.piece_table()
    assert np.diff(X[0]).tolist() == lens and np.diff(Q[0]).tolist() == [0, 1, qmax, 37]
    for metric in (sr.L2, sr.DOT):
        assert np.array_equal(sr.dist_dense(X, Q, metric, F).astype(np.float64), sr.dist_dense(X, Q, metric, np.float64))
    # the model on the rows around the edges, against the dense image
    some = [0, 1, 9, 20, 31, 64, 66, 67, 68, 129]
    sub = sr.csr([sr.row(X, r) for r in some])
    Qs = sr.csr([sr.row(Q, j) for j in (0, 1, 3)])
    for metric in METRICS:
        assert np.array_equal(sr.bits(sr.dist_table(sub, Qs, metric)), sr.bits(sr.dist_dense(X, Q, metric, F)[some][:, [0, 1, 3]]))


def test_a_fused_multiply_add_changes_a_returned_key_of_the_continuous_table():
    X, Q = sr.cont_table()
    assert sr.n_rows(X) == 300 and sr.n_rows(Q) == 7
    assert np.abs(X[2]).min() >= 0.25 and np.abs(X[2]).max() < 4   # no denormals anywhere near
    for metric in METRICS:
        want = sr.topk(sr.dist_table(X, Q, metric), 10)
        fused = sr.topk(sr.dist_table(X, Q, metric, fma=True), 10)
        with pytest.raises(AssertionError, match="differ"):
            sr.same_answer(fused, want)


# ---- planted faults on an answer
@pytest.fixture(scope="module")
def ties():
    X, Q = sr.ties_table(257, 9, seed=21)
    return X, Q, {m: sr.dist_dense(X, Q, m, F) for m in METRICS}


def test_the_numpy_answer_passes(ties):
    X, Q, D = ties
    for metric in METRICS:
        for k in (1, 10, 300):
            sr.same_answer(sr.topk(sr.dist_table(X, Q, metric), k), sr.topk(D[metric], k))


def test_l2_without_the_longer_sides_tail_is_caught(golden):
    X, Q, ref = golden
    want = sr.topk(ref[:, :, sr.L2].view(F), 10)
    with pytest.raises(AssertionError, match="differ"):
        sr.same_answer(sr.topk(sr.dist_table(X, Q, sr.L2, drop_tail=True), 10), want)


def test_cosine_with_a_norm_summed_in_fp64_is_caught(golden):
    X, Q, ref = golden
    want = sr.topk(ref[:, :, sr.COSINE].view(F), 10)
    with pytest.raises(AssertionError, match="differ"):
        sr.same_answer(sr.topk(sr.dist_table(X, Q, sr.COSINE, norm64=True), 10), want)


def test_a_tie_in_the_wrong_id_order_is_caught(ties):
    X, Q, D = ties
    want = sr.topk(D[sr.L2], 64)
    ids, dist, counts = (a.copy() for a in want)
    hit = [(j, e) for j in range(9) for e in range(63) if dist[j, e] == dist[j, e + 1]]
    assert hit, "no tie: pick another seed"
    j, e = hit[0]
    ids[j, e], ids[j, e + 1] = ids[j, e + 1], ids[j, e]
    with pytest.raises(AssertionError, match="ids differ"):
        sr.same_answer((ids, dist, counts), want)


def test_a_nan_ranked_first_is_caught(ties):
    X, Q, D = ties
    d = D[sr.COSINE]
    assert np.isnan(d).any()
    want = sr.topk(d, 257)
    assert np.isnan(want[1][:, -1]).all() and not np.isnan(want[1][:, 0]).any() and (want[2] == 257).all()   # NaN rows are rows, and rank last
    wrong = sr.topk(np.where(np.isnan(d), F(-np.inf), d), 257)
    ids, dist, counts = wrong
    dist = np.where(np.isneginf(dist), F(np.nan), dist)
    with pytest.raises(AssertionError, match="differ"):
        sr.same_answer((ids, dist, counts), want)


def test_a_deleted_row_returned_is_caught(ties):
    X, Q, D = ties
    full = sr.topk(D[sr.DOT], 10)
    vis = np.ones(257, bool)
    vis[full[0][4, 2]] = False
    want = sr.topk(D[sr.DOT], 10, visible=vis)
    assert full[0][4, 2] not in want[0][4]
    with pytest.raises(AssertionError, match="ids differ"):
        sr.same_answer(full, want)
    # everything deleted: counts 0 and padding
    ids, dist, counts = sr.topk(D[sr.DOT], 10, visible=np.zeros(257, bool))
    assert (counts == 0).all() and (ids == -1).all() and np.isposinf(dist).all()


def test_a_count_one_short_is_caught(ties):
    X, Q, D = ties
    want = sr.topk(D[sr.L2], 300)   # k > n
    assert (want[2] == 257).all() and (want[0][:, 257:] == -1).all()
    ids, dist, counts = (a.copy() for a in want)
    counts[3] -= 1
    with pytest.raises(AssertionError, match="counts differ"):
        sr.same_answer((ids, dist, counts), want)
    ids[3, 256], dist[3, 256] = -1, np.inf
    with pytest.raises(AssertionError, match="counts differ"):
        sr.same_answer((ids, dist, counts), want)


def test_the_id_map_is_applied_by_topk(ties):
    X, Q, D = ties
    a, b = sr.topk(D[sr.L2], 5), sr.topk(D[sr.L2], 5, base=3, stride=8)
    assert np.array_equal(a[0] * 8 + 3, b[0]) and np.array_equal(a[1], b[1])


# ---- the entry points: declared, listed, exported
SYMBOLS = ("create", "destroy", "last_error", "set_stream", "synchronize", "attach_csr", "row_count", "set_id_map", "set_deleted", "search", "last_stats")


def test_symbols_are_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert "typedef struct eps_sparse_index eps_sparse_index;" in hdr
    assert re.search(r"int32_t eps_sparse_index_search\(eps_sparse_index\* h, const int64_t\* q_offsets, const int32_t\* q_indices, const float\* q_values, "
                     r"int64_t nq,\s*int32_t k, int64_t\* ids_out, float\* dist_out, int32_t\* counts_out\);", hdr)
    assert "int32_t eps_sparse_index_attach_csr(eps_sparse_index* h, const int64_t* offsets, const int32_t* indices, const float* values, int64_t n);" in hdr
    for cite in ("db/index/index.cpp:22-34", "db/vector.cpp:7-96", "db/execution/vec_search_executor.cpp:742", "db/table_segment_mvp.cpp:526-550"):
        assert cite in hdr, cite
    lib = C.CDLL(build())
    L = _lib.load()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    for s in SYMBOLS:
        name = "eps_sparse_index_" + s
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
        assert getattr(_lib._lib, name).argtypes is not None, name
    raw = _lib._lib
    assert list(raw.eps_sparse_index_search.argtypes) == [vp, vp, vp, vp, i64, i32, vp, vp, vp] and raw.eps_sparse_index_search.restype is i32
    assert list(raw.eps_sparse_index_attach_csr.argtypes) == [vp, vp, vp, vp, i64]
    assert raw.eps_sparse_index_row_count.restype is i64 and raw.eps_sparse_index_last_error.restype is C.c_char_p
    # a NULL handle
    assert L.eps_sparse_index_search(None, None, None, None, 0, 1, None, None, None) == 30000
    assert L.eps_sparse_index_attach_csr(None, None, None, None, 0) == 30000
    assert L.eps_sparse_index_set_deleted(None, None, 0) == 30000 and L.eps_sparse_index_set_id_map(None, 0, 1) == 30000
    assert L.eps_sparse_index_set_stream(None, None) == 30000 and L.eps_sparse_index_synchronize(None) == 30000
    assert L.eps_sparse_index_last_stats(None, None) == 30000 and L.eps_sparse_index_destroy(None) == 30000
    assert L.eps_sparse_index_row_count(None) == -1 and L.eps_sparse_index_last_error(None) == b"null handle"
    assert L.eps_sparse_index_create(0, 0, 0, None) == 30000
    h = vp()
    assert L.eps_sparse_index_create(0, 0, 0, C.byref(h)) == 30000 and L.eps_sparse_index_create(2 ** 31, 0, 0, C.byref(h)) == 30000   # 1 <= dim <= 2^31 - 1
    assert L.eps_sparse_index_create(8, 3, 0, C.byref(h)) == 30000 and not h.value
    build_py = open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()
    assert '"sparse.hip"' in build_py and '"sparse_index.cpp"' in build_py
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "sparse_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()   # no HIP type in the planning header
    import vectordb_amd
    assert vectordb_amd.GpuSparseIndex.__name__ == "GpuSparseIndex"


def test_wrapper_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer is refused before either is touched"""
    from vectordb_amd.sparse_index import GpuSparseIndex, queries_from_dicts
    ix = GpuSparseIndex.__new__(GpuSparseIndex)
    ix.dim = 100
    ix._keep = {}
    ix.h = None
    off, idx, val = np.array([0, 2, 3], np.int64), np.array([1, 5, 7], np.int32), np.array([1, 2, 3], F)
    good = (np.empty((2, 5), np.int64), np.empty((2, 5), F), np.empty(2, np.int32))
    for which, bad in ((0, np.empty((2, 5), np.int32)), (1, np.empty((2, 4), F)), (2, np.empty(2, np.int64)), (0, np.empty((2, 10), np.int64)[:, ::2]),
                       (2, np.empty(3, np.int32))):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError, match="out"):
            ix.search((off, idx, val), 5, out=tuple(out))
    for k in (0, 1025, -1):
        with pytest.raises(ValueError, match="k must be"):
            ix.search((off, idx, val), k)
    with pytest.raises(ValueError, match="differ in length"):
        ix.search((off, idx, val[:2]), 5)
    with pytest.raises(ValueError, match=r"offsets\[-1\]"):
        ix.search((np.array([0, 2, 4], np.int64), idx, val), 5)
    with pytest.raises(ValueError, match="1-D"):
        ix.search((off, idx.reshape(3, 1), val), 5)
    with pytest.raises(ValueError, match="numeric"):
        ix.search((off, np.array([1.5, 2, 3]), val), 5)
    with pytest.raises(ValueError, match="offsets"):
        ix.attach_csr(np.zeros(0, np.int64), idx[:0], val[:0])
    with pytest.raises(ValueError, match="differ in length"):
        ix.attach_csr(off, idx, val[:1])
    with pytest.raises(ValueError, match="indices and 1 values"):
        ix.search([{"indices": [1, 2], "values": [1.0]}], 5)
    q = queries_from_dicts([{"indices": [1, 9], "values": [0.5, 2.0]}, {"indices": [], "values": []}, {"indices": [2 ** 31 - 2], "values": [1.0]}])
    assert q[0].tolist() == [0, 2, 2, 3] and q[1].dtype == np.int32 and q[1].tolist() == [1, 9, 2 ** 31 - 2] and q[2].dtype == F


# ---- the kernels
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_sparse_kernels_use_no_scratch_and_the_planned_lds(tmp_path):
    """the validation pass and {1, 2, 4 queries x KPL 1, 2; 1 query x KPL 4, 8, 16} of the scan: only sparse_* kernels, no scratch memory, at most
    256 registers, static LDS within SPARSE_STATIC_LDS - so that with the plan's dynamic share a workgroup stays within SPARSE_LDS_BUDGET <= 160 KB"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "sparse.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "sparse.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    scan = {k: v for k, v in usage.items() if "sparse_scan_kernel" in k}
    val = {k: v for k, v in usage.items() if "sparse_validate_kernel" in k}
    assert len(scan) == 9 and len(val) == 1 and len(usage) == 10, list(usage)   # only sparse_* kernels
    budget = sr.host_constant("SPARSE_LDS_BUDGET")
    static = sr.host_constant("SPARSE_STATIC_LDS")
    assert budget <= 160 * 1024 and static + sr.host_constant("SPARSE_MAX_QUERY_NNZ") * 8 <= budget
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256, (k, u)
        assert u["LDS Size [bytes/block]"] <= static, (k, u)   # (the staged queries are dynamic LDS: the plan's lds_dynamic, checked by sparse_host_check)
    text = open(src).read()
    assert "#pragma clang fp contract(off)" in text and "fmaf" not in text   # the sums are a multiply and an add
    assert "__global__" not in re.sub(r"//.*", "", open(os.path.join(ROOT, "vectordb_amd", "csrc", "sparse_index.cpp")).read())


def test_host_planning_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "sparse_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "sparse_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "sparse_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
