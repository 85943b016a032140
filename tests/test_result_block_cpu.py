"""CPU side of what the serving calls share: the layout of their result block (csrc/result_block.hpp, a stand-alone program under the sanitizers)
and the Python wrapper's one helper for result arrays (vectordb_amd/index.py: _results over a call's spec) - on every call's spec, with no library
behind the handle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from vectordb_amd.index import GpuIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_result_block_layout_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "result_block_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "result_block_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "result_block_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the wrapper: every call's results, written here by hand from the public header
NQ, DIM, K, M, CAP = 3, 4, 5, 2, 6
SPECS = {
    "search": [("ids", (NQ, K), "int64"), ("dist", (NQ, K), "float32"), ("counts", (NQ,), "int32")],
    "search_range": [("ids", (NQ, CAP), "int64"), ("dist", (NQ, CAP), "float32"), ("counts", (NQ,), "int32"), ("totals", (NQ,), "int64")],
    "search_among": [("ids", (NQ, K), "int64"), ("dist", (NQ, K), "float32"), ("counts", (NQ,), "int32")],
    "search_groups": [("ids", (NQ, K), "int64"), ("dist", (NQ, K), "float32"), ("group_keys", (NQ, K), "int64"), ("counts", (NQ,), "int32")],
    "search_group_rows": [("ids", (NQ, K, M), "int64"), ("dist", (NQ, K, M), "float32"), ("group_keys", (NQ, K), "int64"),
                          ("row_counts", (NQ, K), "int32"), ("group_sizes", (NQ, K), "int64"), ("counts", (NQ,), "int32")],
}
Q = np.zeros((NQ, DIM), np.float32)


class NoLibrary:   # every entry point answers EPS_OK and touches nothing
    def __getattr__(self, name):
        return lambda *a: 0


class Dev:   # what the wrapper takes for a device tensor: anything with data_ptr()
    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, "torch." + dtype

    def data_ptr(self):
        return 0

    def is_contiguous(self):
        return True


@pytest.fixture
def ix():
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim, ix.h, ix.L, ix._keep = DIM, None, NoLibrary(), {}
    return ix


def run(ix, name, out):
    if name == "search":
        return ix.search(Q, K, out=out)
    if name == "search_range":
        return ix.search_range(Q, 1.0, CAP, out=out)
    if name == "search_among":
        return ix.search_among(Q, np.arange(9), K, out=out)
    if name == "search_groups":
        return ix.search_groups(Q, K, out=out)
    return ix.search_group_rows(Q, K, M, out=out)


def good(name):
    return [np.empty(shape, dtype) for _, shape, dtype in SPECS[name]]


@pytest.mark.parametrize("name", sorted(SPECS))
def test_results_are_allocated_from_the_spec(ix, name):
    got = run(ix, name, None)
    assert len(got) == len(SPECS[name])
    for a, (what, shape, dtype) in zip(got, SPECS[name]):
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.dtype(dtype) and a.flags["C_CONTIGUOUS"], (name, what)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_a_correct_out_is_taken_as_it_is(ix, name):
    out = good(name)
    got = run(ix, name, tuple(out))
    assert len(got) == len(out) and all(a is b for a, b in zip(got, out))


@pytest.mark.parametrize("name", sorted(SPECS))
def test_a_wrong_buffer_is_refused_by_call_and_name(ix, name):
    for i, (what, shape, dtype) in enumerate(SPECS[name]):
        wide = shape[:-1] + (2 * shape[-1],)
        bad = {"dtype": np.empty(shape, "float64" if dtype != "float64" else "int64"),
               "dtype of the same width": np.empty(shape, {"int64": "uint64", "int32": "float32", "float32": "int32"}[dtype]),
               "shape": np.empty(shape[:-1] + (shape[-1] + 1,), dtype),
               "rank": np.empty(shape + (1,), dtype),
               "stride": np.empty(wide, dtype)[..., ::2]}
        assert bad["stride"].shape == shape and not bad["stride"].flags["C_CONTIGUOUS"]
        for why, b in bad.items():
            out = good(name)
            out[i] = b
            with pytest.raises(ValueError, match=r"^%s: out\[%s\] " % (name, what)):
                run(ix, name, tuple(out))
    with pytest.raises(ValueError, match="^%s: " % name):
        run(ix, name, tuple(good(name)[:-1]))   # one buffer short


@pytest.mark.parametrize("name", sorted(set(SPECS) - {"search"}))
def test_a_mixed_set_is_refused(ix, name):
    for i, (what, shape, dtype) in enumerate(SPECS[name]):
        out = good(name)
        out[i] = Dev(shape, dtype)
        with pytest.raises(ValueError, match="^%s: .* must all be NumPy arrays or all be device tensors" % name):
            run(ix, name, tuple(out))
    assert len(run(ix, name, tuple(Dev(shape, dtype) for _, shape, dtype in SPECS[name]))) == len(SPECS[name])   # all of one kind: taken


def test_search_leaves_mixed_kinds_to_the_library(ix):
    """host queries may come with device results, and the C ABI refuses a mixed set itself"""
    out = good("search")
    out[1] = Dev((NQ, K), "float32")
    assert run(ix, "search", tuple(out))[1] is out[1]
    with pytest.raises(AssertionError, match="device queries need"):
        ix.search(Dev((NQ, DIM), "float32"), K)


def test_the_single_buffer_check_names_its_call():
    from vectordb_amd.index import _check_out
    with pytest.raises(ValueError, match=r"^search: out\[ids\]"):
        _check_out(np.empty((3, 4), np.int32), "ids", (3, 4), "int64")
    with pytest.raises(ValueError, match=r"^search_groups: out\[group_keys\]"):
        _check_out(np.empty((3, 4), np.int32), "group_keys", (3, 4), "int64", who="search_groups")
