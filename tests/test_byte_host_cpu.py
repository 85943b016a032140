"""CPU side of GpuByteIndex: csrc/byte_host.hpp's plan and integer terms pass their stand-alone check under ASan / UBSan; the wrapper refuses wrong
buffers before a pointer reaches the library; csrc/byte.hip compiles for gfx950 into exactly the plan's six forms, none with scratch memory."""
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
    exe = str(tmp_path / "byte_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "byte_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "byte_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_wrapper_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer is refused before either is touched"""
    from vectordb_amd.byte_index import GpuByteIndex
    for dim in (0, 4097):
        with pytest.raises(ValueError, match="dim must be"):
            GpuByteIndex(dim)
    with pytest.raises(ValueError, match="COSINE"):
        GpuByteIndex(8, "COSINE")
    ix = GpuByteIndex.__new__(GpuByteIndex)
    ix.dim, ix.dtype, ix._keep, ix.h = 70, "int8", {}, None
    q = np.zeros((2, 70), np.int8)
    for k in (0, 1025, -1):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k)
    for bad, what in ((np.zeros((2, 69), np.int8), "shape"), (np.zeros(70, np.int8), "shape"), (np.zeros((2, 70), np.uint8), "int8"),
                      (np.zeros((2, 70), np.float32), "int8")):
        with pytest.raises(ValueError, match=what):
            ix.search(bad, 5)
        with pytest.raises(ValueError, match=what):
            ix.attach_rows(bad)
    with pytest.raises(ValueError, match="out"):
        ix.search(q, 5, out=(np.empty((2, 5), np.int64), np.empty((2, 4), np.int32), np.empty(2, np.int32)))
    with pytest.raises(ValueError, match="uint8"):
        ix.set_deleted(np.zeros(4, np.int32))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_byte_kernels_use_no_scratch_and_are_the_six_forms(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "byte.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
                        "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "byte.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    assert sum("byte_prepare_kernel" in k for k in usage) == 1 and sum("byte_finalize_kernel" in k for k in usage) == 1
    for k, u in usage.items():   # (a 256-thread workgroup: one wavefront per SIMD has 512 registers)
        assert "byte_" in k and u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] + u["AGPRs"] <= 512, (k, u)
    forms = {tuple(int(v) for v in re.search(r"byte_scan_kernelILi(\d+)ELi(\d+)E", k).groups()) for k in usage if "byte_scan_kernel" in k}
    assert forms == {(2, 1), (1, 1), (1, 2), (1, 4), (1, 8), (1, 16)}
    assert len(usage) == len(forms) + 2
