"""CPU side of GpuIndex.search_hybrid (eps_index_search_hybrid; csrc/hybrid.hip): the model the GPU tests trust (tests/hybrid_ref.py) against a direct
fp64 evaluation on a table of ties; the host plan and LDS layout (csrc/hybrid_host.hpp) under the address and undefined-behaviour sanitizers; the new
source compiles for gfx950 without scratch memory and with no LDS beyond the plan's dynamic share."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hybrid_ref as hr
import sparse_ref as sr

ROOT = sr.ROOT
F = np.float32


def host_constant(name):
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "hybrid_host.hpp")).read()
    return int(re.search(r"constexpr \w+ %s = (\d+);" % name, src).group(1))


@pytest.mark.parametrize("w_dense,w_sparse", [(1.0, 1.0), (0.5, 2.0), (0.0, 1.0), (-1.0, 0.25)])
def test_the_model_equals_fp64_on_a_table_of_ties(w_dense, w_sparse):
    """small integers and power-of-two weights: every product and sum is exact, so fp64 decides the order, the ties and the values"""
    rng = np.random.default_rng(3)
    D, S = rng.integers(-3, 4, size=(5, 40)).astype(F), rng.integers(-3, 4, size=(5, 40)).astype(F)
    S[1, 7] = D[2, 9] = np.nan      # a NaN row is a row, after +inf
    S[3, 2], D[3, 3] = np.inf, -0.0
    visible = rng.random(40) < 0.8
    for k in (1, 7, 40):
        ids, score, dense, sparse, counts = hr.topk(D, S, w_dense, w_sparse, k, visible, base=5, stride=3)
        for j in range(5):
            with np.errstate(all="ignore"):
                s64 = w_dense * D[j].astype(np.float64) + w_sparse * S[j].astype(np.float64)
            rows = sorted(np.flatnonzero(visible), key=lambda r: (np.isnan(s64[r]), 0.0 if np.isnan(s64[r]) else s64[r], r))[:k]
            m = len(rows)
            assert counts[j] == m == min(k, visible.sum()) and ids[j, :m].tolist() == [5 + 3 * r for r in rows] and (ids[j, m:] == -1).all()
            assert np.array_equal(hr.canon(score[j, :m]), hr.canon(s64[rows].astype(F))) and np.isinf(score[j, m:]).all()
            assert np.array_equal(hr.canon(dense[j, :m]), hr.canon(D[j, rows])) and np.array_equal(hr.canon(sparse[j, :m]), hr.canon(S[j, rows]))


def test_the_score_is_three_rounded_operations():
    """where fp64 and a fused multiply-add would differ from two rounded products and a rounded add, the model takes the latter"""
    D, S = np.asarray([[F(1) + F(2.0 ** -23)]], F), np.asarray([[F(-1)]], F)
    w = F(1) + F(2.0 ** -23)
    assert hr.score(D, S, w, w)[0, 0] == F(F(w * D[0, 0]) + F(w * S[0, 0])) != F(np.float64(w) * np.float64(D[0, 0]) + np.float64(F(w * S[0, 0])))


def test_host_plan_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "hybrid_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "hybrid_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "hybrid_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_hybrid_kernels_use_no_scratch_and_the_planned_lds(tmp_path):
    """hybrid_tile_kernel at every (NQ, KPL, VEC4), the two forms of hybrid_parts_kernel and the empty-table fill: no scratch memory, at most 256
    registers, no static LDS - the plan's dynamic share (checked by hybrid_host_check) is all a workgroup takes"""
    from vectordb_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert "hybrid.hip" in build.SOURCES
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "hybrid.hip")
    r = subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS["hybrid.hip"] + ["-c", src, "-o", str(tmp_path / "hybrid.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
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
    assert sum("hybrid_tile_kernel" in k for k in usage) == 18 and sum("hybrid_parts_kernel" in k for k in usage) == 2 and len(usage) == 21, list(usage)
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256 and u["LDS Size [bytes/block]"] <= host_constant("HYB_STATIC_LDS"), (k, u)
    assert host_constant("HYB_LDS_BUDGET") <= 80 * 1024 and host_constant("HYB_TILE_ROWS") == 512 and host_constant("HYB_MAX_QUERY_NNZ") == 1024
    text = open(src).read()
    assert text.count("#pragma clang fp contract(off)") >= 3 and text.index("#pragma clang fp contract(off)") < text.index("namespace eps")
