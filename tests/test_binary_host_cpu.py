"""CPU side of GpuBinaryIndex (eps_binary_index_*): the host planning (csrc/binary_host.hpp) passes its stand-alone check under the address and
undefined-behaviour sanitizers; the wrapper refuses wrong buffers before a pointer reaches the library; csrc/binary.hip compiles for gfx950 into
exactly the forms the plan can choose, none of them with scratch memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_planning_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "binary_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "binary_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "binary_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_wrapper_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer is refused before either is touched"""
    from vectordb_amd.binary_index import GpuBinaryIndex
    with pytest.raises(ValueError, match="dim must be"):
        GpuBinaryIndex(0)
    with pytest.raises(ValueError, match="dim must be"):
        GpuBinaryIndex(65537)
    ix = GpuBinaryIndex.__new__(GpuBinaryIndex)
    ix.dim, ix.W, ix._keep, ix.h = 70, 3, {}, None
    q = np.zeros((2, 3), np.uint32)
    for k in (0, 1025, -1):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k)
    for bad, what in ((np.zeros((2, 2), np.uint32), "shape"), (np.zeros(3, np.uint32), "shape"), (np.zeros((2, 3), np.uint64), "uint32"),
                      (np.zeros((2, 3), np.float32), "uint32")):
        with pytest.raises(ValueError, match=what):
            ix.search(bad, 5)
        with pytest.raises(ValueError, match=what):
            ix.attach_rows(bad)
    good = (np.empty((2, 5), np.int64), np.empty((2, 5), np.int32), np.empty(2, np.int32))
    for which, bad in ((0, np.empty((2, 5), np.int32)), (1, np.empty((2, 5), np.float32)), (1, np.empty((2, 4), np.int32)), (2, np.empty(3, np.int32)),
                       (0, np.empty((2, 10), np.int64)[:, ::2])):
        out = list(good)
        out[which] = bad
        with pytest.raises(ValueError, match="out"):
            ix.search(q, 5, out=tuple(out))
    for bad, what in ((np.zeros((2, 69), np.float32), "shape"), (np.zeros(70, np.float32), "shape"), (np.zeros((2, 70), complex), "numeric")):
        with pytest.raises(ValueError, match=what):
            ix.attach_signs(bad)
        with pytest.raises(ValueError, match=what):
            ix.pack_signs(bad)
    with pytest.raises(ValueError, match="out"):
        ix.pack_signs(np.zeros((2, 70), np.float32), out=np.zeros((3, 3), np.uint32))
    with pytest.raises(ValueError, match="uint8"):
        ix.set_deleted(np.zeros(4, np.int32))
    import torch
    with pytest.raises(ValueError, match="contiguous rows"):   # a device-kind tensor whose rows are not contiguous
        ix.attach_rows(torch.zeros((3, 2), dtype=torch.int32).t())


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_binary_kernels_use_no_scratch_and_are_the_forms_the_plan_chooses(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "binary.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
                        "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "binary.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    assert sum("binary_pack_kernel" in k for k in usage) == 1 and sum("binary_finalize_kernel" in k for k in usage) == 1
    for k, u in usage.items():
        assert "binary_" in k and u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 256 and u["Occupancy [waves/SIMD]"] >= 2, (k, u)
    forms = {tuple(int(v) for v in re.search(r"binary_scan_kernelILi(\d+)ELi(\d+)E", k).groups()) for k in usage if "binary_scan_kernel" in k}
    # what binary_plan can choose: KPL from k, the narrowest tile of {4, 8, 16, 32} that holds the batch within 32 / KPL (at least 4)
    kpl = lambda k: 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16
    tile = lambda nq, p: min(t for t in (4, 8, 16, 32) if t >= min(nq, max(4, 32 // p)))
    assert forms == {(tile(nq, kpl(k)), kpl(k)) for k in range(1, 1025) for nq in range(1, 40)}
    assert len(usage) == len(forms) + 2
