"""CPU side of GpuHalfIndex: csrc/half_host.hpp's rounding, plan and seed rule pass their stand-alone check under ASan / UBSan; the wrapper refuses
wrong buffers before a pointer reaches the library; csrc/half.hip compiles for gfx950 into exactly the plan's forms, none with scratch memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rounding_and_planning_are_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "half_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "half_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "half_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_wrapper_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer is refused before either is touched"""
    from vectordb_amd.half_index import GpuHalfIndex
    for dim in (0, 4097):
        with pytest.raises(ValueError, match="dim must be"):
            GpuHalfIndex(dim)
    with pytest.raises(ValueError, match="dtype must be"):
        GpuHalfIndex(8, dtype="float32")
    for dtype, host, wrong in (("float16", "float16", np.uint16), ("bfloat16", "uint16", np.float16)):
        ix = GpuHalfIndex.__new__(GpuHalfIndex)
        ix.dim, ix.dtype, ix.dev_dtype, ix.host_dtype, ix._keep, ix.h = 70, dtype, dtype, host, {}, None
        q = np.zeros((2, 70), host)
        for k in (0, 1025, -1):
            with pytest.raises(ValueError, match="k must be"):
                ix.search(q, k)
        for bad, what in ((np.zeros((2, 69), host), "shape"), (np.zeros(70, host), "shape"), (np.zeros((2, 70), wrong), host), (np.zeros((2, 70), np.float32), host)):
            with pytest.raises(ValueError, match=what):
                ix.search(bad, 5)
            with pytest.raises(ValueError, match=what):
                ix.attach_rows(bad)
        for call in (ix.attach_floats, ix.convert_floats):
            with pytest.raises(ValueError, match="float32"):
                call(q)
            with pytest.raises(ValueError, match="shape"):
                call(np.zeros((2, 71), np.float32))
        with pytest.raises(ValueError, match="out"):
            ix.search(q, 5, out=(np.empty((2, 5), np.int64), np.empty((2, 4), np.float32), np.empty(2, np.int32)))
        with pytest.raises(ValueError, match="uint8"):
            ix.set_deleted(np.zeros(4, np.int32))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_half_kernels_use_no_scratch_and_are_the_plans_forms(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "vectordb_amd", "csrc", "half.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
                        "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "half.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    for one in ("half_prepare_kernel", "half_convert_kernel", "half_seed_kernel", "half_finalize_kernel"):
        assert sum(one in k for k in usage) == 1
    for k, u in usage.items():   # (a 256-thread workgroup: one wavefront per SIMD has 512 registers)
        assert "half_" in k and u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] + u["AGPRs"] <= 512, (k, u)
    forms = {tuple(int(v) for v in re.search(r"half_scan_kernelILi(\d+)ELi(\d+)ELb([01])E", k).groups()) for k in usage if "half_scan_kernel" in k}
    kpl = lambda k: 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16
    plan = {(min(4 if k <= 64 else 2 if k <= 128 else 1, by_d, by_q), kpl(k), bf) for k in (64, 128, 256, 512, 1024) for by_d in (4, 2, 1) for by_q in (4, 2, 1)
            for bf in (0, 1)}
    assert forms == plan and len(forms) == 16
    assert len(usage) == len(forms) + 4
