"""CPU side of the inverted lists of GpuSparseIndex (eps_sparse_index_build_inverted; csrc/sparse_inverted.hip): the term-at-a-time model the GPU
tests trust (tests/sparse_inv_ref.py) equals the sequential model and the reference's recorded bits; each planted fault changes a counted number of
compared words or ids on the table meant to catch it; the four entry points are declared, listed and exported; the new source compiles for gfx950
without scratch memory and within the LDS the plan promises; the host planning (csrc/sparse_inv_host.hpp) passes its stand-alone check under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sparse_inv_ref as si
import sparse_ref as sr

ROOT = sr.ROOT
F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_reference_distances.npz")
METRICS = (sr.COSINE, sr.DOT)
T = si.inv_constant("SPARSE_INV_TILE_ROWS")


@pytest.fixture(scope="module")
def golden():
    """the first 300 rows x 7 queries of the fixture (the recipe's table; the hand-made vectors reach 2^31 - 2, beyond a dense directory)"""
    z = np.load(GOLDEN)
    X = (z["x_offsets"][:301].copy(), z["x_indices"][:z["x_offsets"][300]], z["x_values"][:z["x_offsets"][300]])
    Q = (z["q_offsets"][:8].copy(), z["q_indices"][:z["q_offsets"][7]], z["q_values"][:z["q_offsets"][7]])
    return X, Q, z["bits"][:300, :7]


# ---- the layout
def test_transpose_is_the_table_by_column():
    X, _ = sr.cont_table()
    off, rows, values = si.transpose(X, 400)
    assert off[0] == 0 and off[400] == len(X[1]) and (np.diff(off) >= 0).all() and rows.dtype == np.int32 and values.dtype == F
    back = set()
    for c in range(400):
        r = rows[off[c]:off[c + 1]]
        assert (np.diff(r) > 0).all()   # strictly ascending inside a column
        for rr, v in zip(r, values[off[c]:off[c + 1]]):
            xi, xv = sr.row(X, rr)
            assert xv[np.searchsorted(xi, c)].view(np.uint32) == v.view(np.uint32)   # the CSR's value bits
            back.add((int(rr), c))
    assert len(back) == len(X[1])
    E = sr.csr([([], [])] * 3)
    off, rows, values = si.transpose(E, 8)
    assert off.tolist() == [0] * 9 and len(rows) == 0 and len(values) == 0


# ---- the model against the reference's bits
def test_the_model_equals_the_sequential_model_on_the_continuous_table():
    X, Q = sr.cont_table()
    for metric in METRICS:
        assert si.changed_words(si.dist_terms(X, Q, metric, 400), sr.dist_table(X, Q, metric)) == 0, metric
    assert np.isnan(si.dist_terms(X, Q, sr.COSINE, 400)).any()   # an empty row or query


def test_the_model_equals_the_references_recorded_words(golden):
    X, Q, ref = golden
    for metric in METRICS:
        want = ref[:, :, metric].view(F)
        got = si.dist_terms(X, Q, metric, 400)
        assert got.shape == (300, 7) and si.changed_words(got, want) == 0, (metric, si.changed_words(got, want))


def test_the_model_equals_the_dense_image_on_the_ties_table():
    X, Q = sr.ties_table(1000, 33, seed=1, dim=2 ** 24)
    assert X[1].min() == 0 and X[1].max() == 2 ** 24 - 1 and (np.diff(X[0]) == 0).any()
    for metric in METRICS:
        want = sr.dist_dense(X, Q, metric, F)
        assert si.changed_words(si.dist_terms(X, Q, metric, 2 ** 24), want) == 0, metric
    assert np.isnan(sr.dist_dense(X, Q, sr.COSINE, F)).any()   # empty rows: COSINE's NaN


# ---- planted faults: each changes a counted number of compared words or ids on the table meant to catch it
def test_terms_in_descending_order_change_recorded_words(golden):
    X, Q, ref = golden
    changed = si.changed_words(si.dist_terms(X, Q, sr.DOT, 400, descending=True), ref[:, :, sr.DOT].view(F))
    assert 0 < changed < 2100, changed   # (most pairs have too few common terms for the order to show)
    want = sr.topk(ref[:, :, sr.DOT].view(F), 300)
    got = sr.topk(si.dist_terms(X, Q, sr.DOT, 400, descending=True), 300)
    assert (sr.bits(got[1]) != sr.bits(want[1])).sum() > 0


def test_a_fused_product_changes_recorded_words(golden):
    X, Q, ref = golden
    for metric in METRICS:
        changed = si.changed_words(si.dist_terms(X, Q, metric, 400, fma=True), ref[:, :, metric].view(F))
        assert changed > 0, (metric, changed)   # (COSINE's 1 - x absorbs most of the last-bit changes; DOT shows hundreds)
    Xc, Qc = sr.cont_table()
    with pytest.raises(AssertionError, match="differ"):
        sr.same_answer(sr.topk(si.dist_terms(Xc, Qc, sr.DOT, 400, fma=True), 10), sr.topk(sr.dist_table(Xc, Qc, sr.DOT), 10))


def test_untouched_rows_skipped_change_ids_and_counts():
    X, Q = sr.ties_table(257, 9, seed=21, dim=2 ** 24)
    for metric in METRICS:
        want = sr.topk(sr.dist_dense(X, Q, metric, F), 257)
        dist, offered = si.dist_terms(X, Q, metric, 2 ** 24, skip_untouched=True)
        assert si.changed_words(dist, sr.dist_dense(X, Q, metric, F)) == 0 and not offered.all()
        ids = np.full((9, 257), -1, np.int64)
        counts = np.zeros(9, np.int32)
        for j in range(9):
            one = sr.topk(dist[:, j:j + 1], 257, visible=offered[:, j])
            ids[j], counts[j] = one[0][0], one[2][0]
        assert (ids != want[0]).sum() > 0 and (counts != want[2]).sum() > 0, metric


def test_a_tiles_last_row_dropped_changes_words_of_the_tile_table():
    X, Q, (A, B, Cc) = si.tile_table(T + 1, T)
    lens = np.diff(Q[0]).tolist()
    assert lens == [0, 1, 64, 65, 4096]
    off, rows, values = si.transpose(X, 2 ** 24)
    assert off[A + 1] - off[A] == T + 1 and rows[off[B]:off[B + 1]].tolist() == [T - 1, T] and off[Cc + 1] == off[Cc]
    for j in range(1, 5):
        assert {A, B, Cc} <= set(sr.row(Q, j)[0].tolist()) or (j == 1 and sr.row(Q, j)[0].tolist() == [A])
    for metric in METRICS:
        want = sr.dist_dense(X, Q, metric, F)
        assert si.changed_words(si.dist_terms(X, Q, metric, 2 ** 24), want) == 0
        changed = si.changed_words(si.dist_terms(X, Q, metric, 2 ** 24, drop_tile_last=T), want)
        assert changed >= 2, (metric, changed)   # rows T - 1 and T: a tile's last row and the table's


# ---- the entry points: declared, listed, exported
SYMBOLS = ("build_inverted", "drop_inverted", "inverted_info", "get_inverted")


def test_symbols_are_declared_listed_and_exported():
    from vectordb_amd import _lib
    from vectordb_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    for decl in ("int32_t eps_sparse_index_build_inverted(eps_sparse_index* h);", "int32_t eps_sparse_index_drop_inverted(eps_sparse_index* h);",
                 "int32_t eps_sparse_index_inverted_info(const eps_sparse_index* h, int64_t* columns, int64_t* postings, int64_t* longest_column, "
                 "int32_t* last_engine);",
                 "int32_t eps_sparse_index_get_inverted(eps_sparse_index* h, int64_t* col_offsets, int32_t* rows, float* values);"):
        assert decl in hdr, decl
    for text in ("db/vector.cpp:11-47", "8 * nnz + 8 * (dim + 1)"):
        assert text in hdr, text
    lib = C.CDLL(build())
    L = _lib.load()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    for s in SYMBOLS:
        name = "eps_sparse_index_" + s
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(_lib._lib, name).argtypes is not None, name
    raw = _lib._lib
    assert list(raw.eps_sparse_index_build_inverted.argtypes) == [vp] and list(raw.eps_sparse_index_drop_inverted.argtypes) == [vp]
    assert list(raw.eps_sparse_index_inverted_info.argtypes) == [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    assert list(raw.eps_sparse_index_get_inverted.argtypes) == [vp, vp, vp, vp]
    # a NULL handle
    assert L.eps_sparse_index_build_inverted(None) == 30000 and L.eps_sparse_index_drop_inverted(None) == 30000
    assert L.eps_sparse_index_inverted_info(None, None, None, None, None) == 30000 and L.eps_sparse_index_get_inverted(None, None, None, None) == 30000
    from vectordb_amd import GpuSparseIndex
    for m in SYMBOLS[:3] + ("inverted_arrays",):
        assert callable(getattr(GpuSparseIndex, m)), m


def test_build_py_names_the_new_source():
    from vectordb_amd import build
    assert "sparse_inverted.hip" in build.SOURCES and '"sparse_inverted.hip"' in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "sparse_inv_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()   # no device type in the planning header
    assert si.inv_constant("SPARSE_INV_MAX_DIM") == 2 ** 24 and T == 2048


# ---- the kernels
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_inverted_kernels_use_no_scratch_and_the_planned_lds(tmp_path):
    """sparse_inverted_kernel at every KPL and the five build kernels of the file: no scratch memory, at most 256 registers; the search kernel declares
    no static LDS beyond SPARSE_INV_STATIC_LDS, so that with the plan's dynamic share at the longest query a workgroup stays within
    SPARSE_LDS_BUDGET"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "sparse_inverted.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-c", src,
                        "-o", str(tmp_path / "sparse_inverted.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    search = {k: v for k, v in usage.items() if "sparse_inverted_kernel" in k}
    build = {k: v for k, v in usage.items() if re.search(r"sparse_inv_(expand|scan|longest|digits|scatter)_kernel", k)}
    assert len(search) == 5 and len(build) == 5 and len(usage) == 10, list(usage)   # only these kernels: no library's come with the file
    budget = sr.host_constant("SPARSE_LDS_BUDGET")
    static = si.inv_constant("SPARSE_INV_STATIC_LDS")
    dynamic = sr.host_constant("SPARSE_MAX_QUERY_NNZ") * 8 + sr.host_constant("SPARSE_BLOCK_WAVES") * T * 4   # the plan's share at the longest query
    assert budget <= 160 * 1024 and static + dynamic <= budget
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256, (k, u)
    for k, u in search.items():
        assert u["LDS Size [bytes/block]"] <= static, (k, u)   # (accumulators and the staged query are dynamic LDS: checked by sparse_inv_host_check)
    text = open(src).read()
    assert text.count("#pragma clang fp contract(off)") >= 2 and "fmaf" not in text and "__fma" not in text
    assert text.index("#pragma clang fp contract(off)") < text.index("namespace eps")   # at file scope, in front of every kernel


def test_host_planning_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "sparse_inv_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "sparse_inv_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "sparse_inv_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
