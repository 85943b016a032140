"""CPU side of GpuIndex.search_filters (eps_index_search_filters): tests/filters_ref.py on hand-written rows, the refusals that need no
device, and the host planning (csrc/filters_host.hpp) under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import numpy as np
import pytest

import exact_ref as er
import filters_ref as fr
import range_ref as rr
import select_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_reference_on_hand_written_rows():
    dt, off = sr.row_layout([("flag", "bool"), ("tenant", "i32"), ("score", "f64")])
    rows = np.zeros(6, dt)
    rows["tenant"] = [17, 18, 17, 17, 19, 18]
    rows["score"] = [0.1, 0.5, 0.9, 0.5, 0.5, 0.2]
    progs = [[], [("const", 0)], [("i32", off["tenant"]), ("const", 17), ("=",)],
             [("f64", off["score"]), ("const", 0.25), (">=",), ("f64", off["score"]), ("const", 0.75), ("<",), ("and",)]]
    masks = fr.program_masks(6, progs, rows)
    assert masks.T.tolist() == [[True] * 6, [False] * 6, [True, False, True, True, False, False], [False, True, False, True, True, False]]
    masks = fr.program_masks(6, progs, rows, np.array([True, True, True, False, True, True]))   # row 3 deleted
    assert masks[:, 2].tolist() == [True, False, True, False, False, False] and masks[:, 0].tolist() == [True, True, True, False, True, True]
    X = np.stack([np.arange(6, dtype=F), np.zeros(6, F), np.zeros(6, F)], 1)
    Q, qp = np.zeros((5, 3), F), [2, 0, 1, 3, 2]   # rows on a line, queries at 0: the answer is the visible rows in row order
    d32 = rr.dist32(X, Q, 0)
    ids, dist, counts, visible = fr.numpy_filters(d32, masks, qp, 3)
    assert ids.tolist() == [[0, 2, -1], [0, 1, 2], [-1, -1, -1], [1, 4, -1], [0, 2, -1]]
    assert counts.tolist() == [2, 3, 0, 2, 2] and visible.tolist() == [2, 5, 0, 2, 2]
    ref = er.Ref(X, Q, 0)
    assert fr.check_filters(ids, dist, counts, visible, ref, masks, qp, 3, exact=True) == 0


def test_refusals_that_need_no_device():
    from vectordb_amd import _lib
    from vectordb_amd.index import GpuIndex
    L = _lib.load()
    assert L.eps_index_search_filters(None, None, 0, 1, None, None, None, 1, None, None, 0, 0, 0, 0, None, None, None, None) == 30000   # no handle
    assert L.eps_index_filters_info(None, None, None, 0, None) == 30000
    ix = GpuIndex.__new__(GpuIndex)   # no handle, no library: the wrapper's own checks
    ix.dim, ix._keep, ix.h = 4, {}, None
    with pytest.raises(ValueError, match="nq = 3"):
        ix.search_filters(np.zeros((3, 4), F), 5, [[]], [0, 0])
    with pytest.raises(ValueError, match="between 1 and 64"):
        ix.search_filters(np.zeros((3, 4), F), 5, [[]] * 65, [0, 0, 0])


def test_host_planning_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "filters_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "filters_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "filters_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
