"""CPU side of GpuIndex.search_range (eps_index_search_range): the reference the GPU tests trust (tests/range_ref.py) fed with numpy's own fp32 answer -
it passes, within the cap on undecided rows - and with planted faults, each of which it must catch; the wrapper's output check; the symbol's
declaration.  The continuous cases here are the ones tests/test_gpu_search_range.py runs on the device: this file keeps the run that shows the
radii sit in gaps wide enough for the band."""
import os
import re

import numpy as np
import pytest

import exact_ref as er
import range_ref as rr
from vectordb_amd.index import GpuIndex, _check_range_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CONT = ("embedding-like", 3000, 96, 40)   # the continuous table of the GPU tests; radii midway between the 20th and 21st neighbour
CONT_K = 20


@pytest.fixture(scope="module")
def cont():
    X, Q = er.make(*CONT)
    return X, Q, {m: er.Ref(X, Q, m) for m in (0, 1)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("cap", [64, 8])
def test_numpy_fp32_answer_passes_within_the_cap(cont, metric, cap):
    X, Q, refs = cont
    ref = refs[metric]
    radius = rr.midway_radii(ref, CONT_K)
    ans = rr.numpy_range(rr.dist32(X, Q, metric), radius, cap)
    und, must = rr.check_range(*ans, ref, radius, cap, what="numpy metric %d" % metric)
    print("metric %d cap %d: %d undecided rows, %d certain members" % (metric, cap, und, must))
    assert must >= (CONT_K - 1) * ref.nq
    rr.assert_cap(und, must)
    assert ((ans[3] > cap).all() if cap < CONT_K else (ans[3] <= cap).all())   # (cap 8: the total > cap branch; cap 64: the complete answers)


@pytest.mark.parametrize("metric", [0, 2])
def test_uniform_table_of_the_8_bit_case_stays_within_the_cap(metric):
    """tests/test_gpu_search_range.py::test_uniform_rows_run_the_8_bit_form: the same table, radii and cap, fed with numpy's fp32 answer"""
    X, Q = er.make("uniform", 3000, 96, 40)
    ref = er.Ref(X, Q, metric)
    radius = rr.midway_radii(ref, CONT_K)
    und, must = rr.check_range(*rr.numpy_range(rr.dist32(X, Q, metric), radius, 64), ref, radius, 64)
    print("uniform metric %d: %d undecided rows, %d certain members" % (metric, und, must))
    rr.assert_cap(und, must)


# ---- planted faults on a table without a band: integers, radii at half-integers
@pytest.fixture(scope="module")
def ints():
    X, Q = er.make("integers -8..8", 400, 19, 6)
    ref = er.Ref(X, Q, 0)
    d32 = rr.dist32(X, Q, 0)
    assert np.array_equal(d32.astype(np.float64), ref.d64)
    radius = (np.sort(d32, axis=0)[30] + F(0.5)).astype(F)
    return ref, d32, radius


def answer(ints, cap):
    ref, d32, radius = ints
    return [a.copy() for a in rr.numpy_range(d32, radius, cap)]


def test_integer_answer_passes_with_no_band(ints):
    ref, d32, radius = ints
    for cap in (64, 8):
        und, must = rr.check_range(*answer(ints, cap), ref, radius, cap)
        assert und == 0 and must >= 31 * ref.nq


def test_a_dropped_member_is_caught(ints):
    ref, d32, radius = ints
    ids, dist, counts, totals = answer(ints, 64)
    m = counts[2]
    ids[2, 5:m - 1], dist[2, 5:m - 1] = ids[2, 6:m].copy(), dist[2, 6:m].copy()
    ids[2, m - 1], dist[2, m - 1] = -1, np.inf
    counts[2] -= 1
    totals[2] -= 1
    with pytest.raises(AssertionError, match="outside|not returned"):
        rr.check_range(ids, dist, counts, totals, ref, radius, 64)
    totals[2] += 1   # ... and with the total left right, the count gives it away
    with pytest.raises(AssertionError, match="count"):
        rr.check_range(ids, dist, counts, totals, ref, radius, 64)


def test_an_added_non_member_is_caught(ints):
    ref, d32, radius = ints
    ids, dist, counts, totals = answer(ints, 64)
    m = counts[1]
    out = np.flatnonzero(d32[:, 1] > radius[1])
    row = out[np.argmin(d32[out, 1])]   # the closest row beyond the radius, with its own true distance
    ids[1, m], dist[1, m] = row, d32[row, 1]
    counts[1] += 1
    totals[1] += 1
    with pytest.raises(AssertionError, match="beyond the radius"):
        rr.check_range(ids, dist, counts, totals, ref, radius, 64)


def test_equal_distances_in_the_wrong_id_order_are_caught(ints):
    ref, d32, radius = ints
    ids, dist, counts, totals = answer(ints, 64)
    hit = [(q, e) for q in range(ref.nq) for e in range(counts[q] - 1) if dist[q, e] == dist[q, e + 1]]
    assert hit, "the table has no tie inside an answer: pick another seed"
    q, e = hit[0]
    ids[q, e], ids[q, e + 1] = ids[q, e + 1], ids[q, e]
    with pytest.raises(AssertionError, match="out of order"):
        rr.check_range(ids, dist, counts, totals, ref, radius, 64)


def test_a_total_off_by_one_is_caught(ints):
    ref, d32, radius = ints
    for cap in (64, 8):   # (cap 8: counts = cap either way, only the total's own range can tell)
        for delta in (1, -1):
            ids, dist, counts, totals = answer(ints, cap)
            totals[3] += delta
            if cap == 64:
                counts[3] += delta   # (keep counts = min(totals, cap): the total's range has to catch it, not the structure)
                if delta > 0:
                    ids[3, counts[3] - 1], dist[3, counts[3] - 1] = ids[3, 0] + 0, dist[3, counts[3] - 2]
            with pytest.raises(AssertionError):
                rr.check_range(ids, dist, counts, totals, ref, radius, cap)
    ids, dist, counts, totals = answer(ints, 8)
    totals[3] += 1
    with pytest.raises(AssertionError, match="total"):
        rr.check_range(ids, dist, counts, totals, ref, radius, 8)


@pytest.mark.parametrize("metric", [0, 1])
def test_a_distance_two_ulp_beyond_the_bound_is_caught(cont, metric):
    X, Q, refs = cont
    ref = refs[metric]
    radius = rr.midway_radii(ref, CONT_K)
    ids, dist, counts, totals = [a.copy() for a in rr.numpy_range(rr.dist32(X, Q, metric), radius, 64)]
    B = ref.bound("free")
    row = ids[4, 0]
    edge = F(ref.d64[row, 4] - B[row, 4])   # the closest row's distance, pushed DOWN: it stays first and within the radius
    if float(edge) >= ref.d64[row, 4] - B[row, 4]:
        edge = np.nextafter(edge, F(-np.inf))
    dist[4, 0] = np.nextafter(np.nextafter(edge, F(-np.inf)), F(-np.inf))
    with pytest.raises(AssertionError, match="bound"):
        rr.check_range(ids, dist, counts, totals, ref, radius, 64)


def test_a_program_that_reads_the_distance_judges_per_query(ints):
    ref, d32, radius = ints
    vis = d32 < (radius - F(10))[None, :]   # `@distance < r2`, r2 < r: visibility is per (row, query)
    ans = rr.numpy_range(d32, radius, 64, visible=vis)
    assert (ans[3] < rr.numpy_range(d32, radius, 64)[3]).all()
    rr.check_range(*ans, ref, radius, 64, visible=vis)
    with pytest.raises(AssertionError, match="total|not visible"):
        rr.check_range(*rr.numpy_range(d32, radius, 64), ref, radius, 64, visible=vis)


# ---- the wrapper's output check
def bufs(nq=3, cap=5):
    return [np.empty((nq, cap), np.int64), np.empty((nq, cap), np.float32), np.empty(nq, np.int32), np.empty(nq, np.int64)]


def test_output_check_accepts_what_the_abi_assumes():
    _check_range_out(*bufs(), 3, 5)


@pytest.mark.parametrize("which,bad", [
    (0, np.empty((3, 5), np.int32)), (1, np.empty((3, 5), np.float64)), (2, np.empty(3, np.int64)), (3, np.empty(3, np.int32)),   # dtypes
    (0, np.empty((3, 4), np.int64)), (1, np.empty((2, 5), np.float32)), (2, np.empty(4, np.int32)), (3, np.empty((3, 1), np.int64)),   # shapes
    (0, np.empty((3, 10), np.int64)[:, ::2]), (1, np.empty((5, 3), np.float32).T), (3, np.empty(6, np.int64)[::2]),   # strides
])
def test_output_check_refuses(which, bad):
    b = bufs()
    b[which] = bad
    with pytest.raises(ValueError, match="search_range: out"):
        _check_range_out(*b, 3, 5)


def test_output_check_refuses_mixed_kinds():
    class Dev:   # what the wrapper takes for a device tensor: anything with data_ptr()
        dtype, shape = "torch.int64", (3,)

        def data_ptr(self):
            return 0

        def is_contiguous(self):
            return True

    b = bufs()
    b[3] = Dev()
    with pytest.raises(ValueError, match="all"):
        _check_range_out(*b, 3, 5)


def test_search_range_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer is refused before either is touched"""
    ix = GpuIndex.__new__(GpuIndex)
    ix.dim = 4
    b = bufs()
    b[1] = np.empty((3, 5), np.float64)
    with pytest.raises(ValueError):
        ix.search_range(np.zeros((3, 4), np.float32), 1.0, 5, out=tuple(b))
    with pytest.raises(KeyError):
        ix.search_range(np.zeros((3, 4), np.float32), 1.0, 5, flat_engine="triton")
    ix.h = None


def test_symbol_is_declared_and_listed():
    from vectordb_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "epsilla_gfx950.h")).read()
    assert re.search(r"int32_t eps_index_search_range\(eps_index\* h, const float\* queries, int64_t nq, const float\* radius, int32_t cap, "
                     r"const eps_search_params\* p,\s*int64_t\* ids_out, float\* dist_out, int32_t\* counts_out, int64_t\* totals_out\);", hdr)
    assert "eps_index_search_range" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr int RANGE_MAX_CAP = (\d+);", src).group(1)) == 8192
    assert "range.hip" in open(os.path.join(ROOT, "vectordb_amd", "build.py")).read()
