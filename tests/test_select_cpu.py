"""CPU side of GpuIndex.select (eps_index_select): the wrapper's output check, the geometry the GPU tests name their edge sizes from, and the numpy
evaluator those tests trust (tests/select_ref.py), on rows written by hand."""
import os
import re

import numpy as np
import pytest

import select_ref as sr
from vectordb_amd.index import GpuIndex, _check_select_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_output_check_accepts_what_the_abi_assumes():
    _check_select_out(np.empty(7, np.int64), np.zeros(2, np.int64), 7)
    _check_select_out(np.empty(0, np.int64), np.zeros(2, np.int64), 0)


@pytest.mark.parametrize("ids,counts,limit", [
    (np.empty(7, np.int32), np.zeros(2, np.int64), 7),           # dtype of ids
    (np.empty(7, np.int64), np.zeros(2, np.int32), 7),           # dtype of counts
    (np.empty(6, np.int64), np.zeros(2, np.int64), 7),           # too short
    (np.empty(8, np.int64), np.zeros(2, np.int64), 7),           # not the shape asked for
    (np.empty((7, 1), np.int64), np.zeros(2, np.int64), 7),      # rank
    (np.empty(7, np.int64), np.zeros(1, np.int64), 7),           # counts holds count AND total
    (np.empty(14, np.int64)[::2], np.zeros(2, np.int64), 7),     # strided ids
    (np.empty(7, np.int64), np.zeros(4, np.int64)[::2], 7),      # strided counts
])
def test_output_check_refuses(ids, counts, limit):
    with pytest.raises(ValueError, match="select: out"):
        _check_select_out(ids, counts, limit)


def test_output_check_refuses_mixed_kinds():
    class Dev:   # what the wrapper takes for a device tensor: anything with data_ptr()
        dtype, shape = "torch.int64", (2,)

        def data_ptr(self):
            return 0

        def is_contiguous(self):
            return True

    with pytest.raises(ValueError, match="both"):
        _check_select_out(np.empty(3, np.int64), Dev(), 3)


def test_select_checks_before_any_pointer_reaches_the_library():
    """no handle, no library: a wrong buffer is refused before either is touched"""
    ix = GpuIndex.__new__(GpuIndex)
    with pytest.raises(ValueError):
        ix.select(0, 5, out=(np.empty(5, np.float64), np.zeros(2, np.int64)))
    ix.h = None


def test_geometry_named_by_the_gpu_tests_is_the_kernels():
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr int SEL_ROWS = (\d+);", src).group(1)) == sr.SEL_ROWS
    assert int(re.search(r"constexpr int SEL_SCAN_THREADS = (\d+);", src).group(1)) == sr.SEL_SCAN_THREADS


# ---- the evaluator, one case per opcode class, on rows written by hand
ROW = np.dtype([("i8", np.int8), ("flag", np.uint8), ("i16", np.int16), ("i32", np.int32), ("i64", np.int64), ("f32", np.float32), ("pad", np.int32),
                ("f64", np.float64)])
OFF = {name: ROW.fields[name][1] for name in ROW.names}
ROWS = np.zeros(4, ROW)
ROWS["i8"] = [-128, -1, 0, 127]
ROWS["flag"] = [0, 1, 2, 255]
ROWS["i16"] = [-32768, -2, 3, 32767]
ROWS["i32"] = [-7, 7, -2147483648, 2147483647]
ROWS["i64"] = [-(2 ** 53) - 1, 5, -5, 2 ** 62]
ROWS["f32"] = [0.1, -0.0, np.inf, np.nan]
ROWS["f64"] = [0.1, 1e300, -1e-300, 7.5]


def test_loads_widen_to_double():
    for name in ("i8", "i16", "i32", "i64", "f32", "f64"):
        got = sr.eval_program([(name, OFF[name])], ROWS)
        want = ROWS[name].astype(np.float64)
        assert np.array_equal(got, want, equal_nan=True), name
    assert sr.eval_program([("i64", OFF["i64"])], ROWS)[0] == float(-(2 ** 53))   # (rounded as (double)int64 rounds: to even)
    assert list(sr.eval_program([("f32", OFF["f32"]), ("f64", OFF["f64"]), ("=",)], ROWS)) == [0.0, 0.0, 0.0, 0.0]   # 0.1f is not 0.1


def test_bool_is_byte_not_zero():
    assert list(sr.eval_program([("bool", OFF["flag"])], ROWS)) == [0.0, 1.0, 1.0, 1.0]


def test_constants_and_distance():
    assert list(sr.eval_program([("const", 2.5)], ROWS)) == [2.5] * 4
    assert list(sr.eval_program([("dist",)], ROWS)) == [0.0] * 4
    assert list(sr.eval_program([("dist",), ("const", 1), ("<",)], ROWS)) == [1.0] * 4


def test_arithmetic():
    i32 = ("i32", OFF["i32"])
    assert list(sr.eval_program([i32, ("const", 1), ("+",)], ROWS)) == [-6.0, 8.0, -2147483647.0, 2147483648.0]   # no int32 wrap
    assert list(sr.eval_program([i32, ("const", 1), ("-",)], ROWS)) == [-8.0, 6.0, -2147483649.0, 2147483646.0]
    assert list(sr.eval_program([i32, ("const", 0.5), ("*",)], ROWS)) == [-3.5, 3.5, -1073741824.0, 1073741823.5]
    got = sr.eval_program([i32, ("i8", OFF["i8"]), ("/",)], ROWS)   # row 2 divides by zero
    assert got[0] == -7.0 / -128.0 and got[1] == -7.0 and got[2] == -np.inf and got[3] == 2147483647.0 / 127.0


def test_mod_is_fmod():
    """the sign follows the dividend, fractions survive, x % 0 is NaN (and NaN is not 'non-zero equal to anything')"""
    got = sr.eval_program([("i32", OFF["i32"]), ("const", 4), ("%",)], ROWS)
    assert list(got) == [-3.0, 3.0, -0.0, 3.0] and np.signbit(got[2])
    assert list(sr.eval_program([("f64", OFF["f64"]), ("const", 2), ("%",)], ROWS)) == [0.1, 0.0, -1e-300, 1.5]
    assert np.isnan(sr.eval_program([("i32", OFF["i32"]), ("const", 0), ("%",)], ROWS)).all()


def test_comparisons_in_double():
    i8, c0 = ("i8", OFF["i8"]), ("const", 0)
    want = {"<": [1, 1, 0, 0], "<=": [1, 1, 1, 0], "=": [0, 0, 1, 0], "<>": [1, 1, 0, 1], ">=": [0, 0, 1, 1], ">": [0, 0, 0, 1]}
    for op, w in want.items():
        assert list(sr.eval_program([i8, c0, (op,)], ROWS)) == [float(x) for x in w], op
    # NaN: every comparison but <> is false
    f32 = ("f32", OFF["f32"])
    assert sr.eval_program([f32, f32, ("=",)], ROWS)[3] == 0.0 and sr.eval_program([f32, f32, ("<>",)], ROWS)[3] == 1.0
    assert sr.eval_program([f32, c0, ("=",)], ROWS)[1] == 1.0   # -0.0 == 0


def test_logic_treats_non_zero_as_true():
    flag, i8 = ("bool", OFF["flag"]), ("i8", OFF["i8"])   # truth: flag 0 1 1 1, i8 1 1 0 1
    assert list(sr.eval_program([flag, i8, ("and",)], ROWS)) == [0.0, 1.0, 0.0, 1.0]
    assert list(sr.eval_program([flag, i8, ("or",)], ROWS)) == [1.0, 1.0, 1.0, 1.0]
    assert list(sr.eval_program([i8, ("not",)], ROWS)) == [0.0, 0.0, 1.0, 0.0]
    assert list(sr.eval_program([flag, i8, ("=b",)], ROWS)) == [0.0, 1.0, 0.0, 1.0]
    assert list(sr.eval_program([flag, i8, ("<>b",)], ROWS)) == [1.0, 0.0, 1.0, 0.0]
    assert sr.eval_program([("f32", OFF["f32"]), ("not",)], ROWS)[3] == 0.0   # NaN != 0: true, so NOT gives 0 (st != 0.0 ? 0 : 1)


def test_visible_rows_combines_bitset_column_and_program():
    deleted = np.array([0b0010], np.uint8)   # row 1
    vis = sr.visible_rows(4, deleted=deleted)
    assert list(vis) == [True, False, True, True]
    vis = sr.visible_rows(4, int_filter=(ROWS["i16"], ">=", -2))
    assert list(vis) == [False, True, True, True]
    vis = sr.visible_rows(4, deleted=deleted, program=[("i32", OFF["i32"]), ("const", 0), (">",)], rows=ROWS)
    assert list(vis) == [False, False, False, True]
    ids, total = sr.expected(np.array([1, 0, 1, 1, 0, 1], bool), 1, 2, base=3, stride=8)
    assert list(ids) == [2 * 8 + 3, 3 * 8 + 3] and total == 4
    ids, total = sr.expected(np.array([1, 0, 1], bool), 5, 2)
    assert len(ids) == 0 and total == 2
