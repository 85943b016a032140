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


def test_distance_is_what_the_caller_hands_over():
    """`dist` is the per-row value of @distance (a search's judging sites); None reads 0 (select, mask launch, pre-filter call)"""
    d = np.array([0.0, 2.5, np.inf, np.nan])
    assert np.array_equal(sr.eval_program([("dist",)], ROWS, dist=d), d, equal_nan=True)
    assert list(sr.eval_program([("dist",), ("const", 2.5), ("<=",)], ROWS, dist=d)) == [1.0, 1.0, 0.0, 0.0]
    assert list(sr.eval_program([("dist",), ("i8", OFF["i8"]), ("*",)], ROWS, dist=np.array([1.0, 2.0, 3.0, 0.5]))) == [-128.0, -2.0, 0.0, 63.5]
    assert list(sr.visible_rows(4, program=[("dist",), ("const", 1), (">",)], rows=ROWS, dist=d)) == [False, True, True, False]
    assert list(sr.visible_rows(4, program=[("dist",), ("const", 1), (">",)], rows=ROWS)) == [False] * 4


# ---- the packed layout of the reference's attribute rows, and one hand-written row per edge value
# {BOOL, DOUBLE, TINYINT, BIGINT, SMALLINT, FLOAT}: the double sits at byte 1, the int64 at byte 10 (tests/test_gpu_filter_program.py runs the
# same fields on the device); `n` (INT) rides behind them for the i32 load
FIELDS = [("b", "bool"), ("w", "f64"), ("t", "i8"), ("big", "i64"), ("s", "i16"), ("x", "f32")]
PACKED, PO = sr.row_layout(FIELDS + [("n", "i32")])
DEFAULTS = dict(b=1, w=1.5, t=3, big=7, s=5, x=2.5, n=-9)
B_, W_, T_, BIG_, S_, X_, N_ = (("bool", PO["b"]), ("f64", PO["w"]), ("i8", PO["t"]), ("i64", PO["big"]), ("i16", PO["s"]), ("f32", PO["x"]),
                                ("i32", PO["n"]))
NAN, INF = float("nan"), float("inf")
DENORM = float(np.float32(2.0 ** -149))   # the smallest fp32 denormal


def c(v):
    return ("const", v)


def test_row_layout_packs_as_the_reference_does():
    assert (PO["b"], PO["w"], PO["t"], PO["big"], PO["s"], PO["x"], PO["n"]) == (0, 1, 9, 10, 18, 20, 24) and PACKED.itemsize == 28
    dt, off = sr.row_layout(FIELDS)
    assert dt.itemsize == 24 and off == {k: PO[k] for k in off}
    dt, off = sr.row_layout(FIELDS, align=True)
    assert all(off[name] % dt.fields[name][0].itemsize == 0 for name in off) and off["w"] == 8 and dt.itemsize % 8 == 0


# (program, the fields of the one row that differ from DEFAULTS, @distance or None, the final stack value - written by hand)
SIX = ("<", "<=", "=", "<>", ">=", ">")
CASES = (
    # NaN under every comparison: only <> is true
    [([W_, c(0), (op,)], dict(w=NAN), None, 1.0 if op == "<>" else 0.0) for op in SIX]
    + [([X_, c(0), (op,)], dict(x=NAN), None, 1.0 if op == "<>" else 0.0) for op in SIX]
    + [([c(0), W_, (op,)], dict(w=NAN), None, 1.0 if op == "<>" else 0.0) for op in SIX]
    + [
        ([W_], dict(w=NAN), None, NAN),                          # NaN as the final value: passes (st[0] != 0.0)
        ([X_, X_, ("-",)], dict(x=INF), None, NAN),              # inf - inf
        ([W_, c(1e308), (">",)], dict(w=INF), None, 1.0),
        ([W_, c(-1e308), ("<",)], dict(w=-INF), None, 1.0),
        ([X_, c(3.5e38), (">",)], dict(x=INF), None, 1.0),       # (beyond the largest fp32)
        ([c(1), W_, ("/",)], dict(w=0.0), None, INF),            # 1 / 0
        ([c(-1), W_, ("/",)], dict(w=0.0), None, -INF),          # -1 / 0
        ([c(1), W_, ("/",)], dict(w=-0.0), None, -INF),          # 1 / -0
        ([c(0), W_, ("/",)], dict(w=0.0), None, NAN),            # 0 / 0
        ([T_, W_, ("%",)], dict(w=0.0), None, NAN),              # x % 0
        ([T_, c(3), ("%",)], dict(t=-7), None, -1.0),            # -7 % 3 = -1: the sign of the dividend
        ([T_, S_, ("%",)], dict(t=7, s=-3), None, 1.0),          # 7 % -3 = 1
        ([W_, c(2), ("%",)], dict(w=7.5), None, 1.5),            # fractions survive
        ([BIG_, c(2 ** 53), ("=",)], dict(big=2 ** 53 + 1), None, 1.0),    # (double)int64 rounds: equal after the conversion
        ([BIG_, c(2 ** 53), (">",)], dict(big=2 ** 53 + 1), None, 0.0),
        ([BIG_, c(2 ** 53 + 4), ("=",)], dict(big=2 ** 53 + 3), None, 1.0),   # (to even: 2^53 + 3 -> 2^53 + 4)
        ([BIG_, c(2 ** 40), ("=",)], dict(big=2 ** 40 + 1), None, 0.0),    # (through a float it would be 2^40)
        ([BIG_, c(-2.0 ** 63), ("=",)], dict(big=-2 ** 63), None, 1.0),    # int64 min is a double
        ([BIG_, c(2.0 ** 63), ("=",)], dict(big=2 ** 63 - 1), None, 1.0),  # int64 max rounds up to 2^63
        ([BIG_, c(0), ("<",)], dict(big=-2 ** 63), None, 1.0),
        ([T_, c(-128), ("=",)], dict(t=-128), None, 1.0),
        ([T_, c(0), ("<",)], dict(t=-128), None, 1.0),           # (read unsigned it would be 128)
        ([S_, c(-32768), ("=",)], dict(s=-32768), None, 1.0),
        ([S_, c(0), ("<",)], dict(s=-32768), None, 1.0),         # (read unsigned it would be 32768)
        ([N_, c(-9), ("=",)], dict(), None, 1.0),
        ([N_, c(-2147483648), ("=",)], dict(n=-2 ** 31), None, 1.0),
        ([X_, c(0), (">",)], dict(x=DENORM), None, 1.0),         # the smallest fp32 denormal is > 0 ...
        ([X_, c(2.0 ** -149), ("=",)], dict(x=DENORM), None, 1.0),   # ... and widens exactly
        ([X_], dict(x=DENORM), None, 2.0 ** -149),
        ([X_, c(0), ("=",)], dict(x=-0.0), None, 1.0),           # -0.0 = 0 ...
        ([X_], dict(x=-0.0), None, -0.0),                        # ... and as a boolean it is false
        ([X_, ("not",)], dict(x=-0.0), None, 1.0),
        ([W_, c(0), ("=",)], dict(w=-0.0), None, 1.0),
        ([W_, ("not",)], dict(w=-0.0), None, 1.0),
        ([B_], dict(b=0), None, 0.0),                            # a bool is its byte != 0
        ([B_], dict(b=1), None, 1.0),
        ([B_], dict(b=2), None, 1.0),
        ([B_], dict(b=255), None, 1.0),
        ([B_, c(1), ("=",)], dict(b=2), None, 1.0),              # (it loads as 1.0, not as 2.0)
        ([T_, S_, ("+",)], dict(), None, 8.0),
        ([T_, S_, ("-",)], dict(), None, -2.0),
        ([W_, X_, ("*",)], dict(), None, 3.75),
        ([BIG_, c(2), ("/",)], dict(), None, 3.5),
        ([T_, c(3), ("<",)], dict(), None, 0.0),
        ([T_, c(3), ("<=",)], dict(), None, 1.0),
        ([T_, c(3), (">=",)], dict(), None, 1.0),
        ([T_, c(3), (">",)], dict(), None, 0.0),
        ([T_, c(4), ("<=",)], dict(t=5), None, 0.0),
        ([T_, c(3), ("<>",)], dict(), None, 0.0),
        ([T_, ("not",)], dict(), None, 0.0),                     # NOT of a number that is not a boolean: 3 is true (1 - x would give -2: true)
        ([W_, ("not",)], dict(w=0.5), None, 0.0),
        ([W_, ("not",)], dict(w=NAN), None, 0.0),                # NaN != 0: true
        ([B_, T_, ("and",)], dict(t=0), None, 0.0),
        ([B_, T_, ("and",)], dict(b=2, t=-1), None, 1.0),
        ([B_, T_, ("or",)], dict(b=0, t=0), None, 0.0),
        ([B_, T_, ("or",)], dict(b=0, t=-1), None, 1.0),
        ([B_, T_, ("=b",)], dict(b=2), None, 1.0),               # 1.0 and 3.0 are both true (`=` says 0)
        ([B_, T_, ("=",)], dict(b=2), None, 0.0),
        ([B_, S_, c(0), (">",), ("=b",)], dict(b=0, s=-4), None, 1.0),
        ([B_, T_, ("<>b",)], dict(b=2), None, 0.0),
        ([B_, T_, ("<>b",)], dict(b=0), None, 1.0),
        ([W_, X_, ("<>b",)], dict(w=NAN, x=-0.0), None, 1.0),    # NaN is true, -0.0 is false
        ([("dist",)], dict(), None, 0.0),
        ([("dist",)], dict(), 2.5, 2.5),
        ([("dist",), X_, ("*",), c(6.25), ("=",)], dict(), 2.5, 1.0),
        ([("dist",), c(2.5), (">",)], dict(), 2.5, 0.0),         # at the exact distance > and >= part
        ([("dist",), c(2.5), (">=",)], dict(), 2.5, 1.0),
    ])


def one_row(**fields):
    r = np.zeros(1, PACKED)
    for name, v in dict(DEFAULTS, **fields).items():
        r[name] = v
    return r


@pytest.mark.parametrize("i", range(len(CASES)))
def test_hand_written_rows(i):
    prog, fields, dist, want = CASES[i]
    got = sr.eval_program(prog, one_row(**fields), None if dist is None else np.array([dist]))[0]
    if want != want:
        assert got != got, (prog, fields, got)
    else:
        assert got == want and np.signbit(got) == np.signbit(want), (prog, fields, got, want)
    passes = sr.visible_rows(1, program=prog, rows=one_row(**fields), dist=None if dist is None else np.array([dist]))[0]
    assert passes == (want != 0.0), (prog, fields)   # (a NaN passes: NaN != 0.0)


def test_every_opcode_has_a_hand_written_case():
    from vectordb_amd import _lib
    used = {ins[0] for prog, _, _, _ in CASES for ins in prog}
    assert used == set(_lib.FOP), (sorted(set(_lib.FOP) - used), sorted(used - set(_lib.FOP)))
    assert set(sr._LOADS) | {"bool"} <= used


# ---- what Index::set_filter_program_pitched must refuse and accept (tests/test_gpu_filter_program.py installs these over rows of STRIDE bytes).
# An instruction is (name | raw opcode, argument); `rows`: how many attribute rows are handed over, relative to the table
STRIDE = 24
USER_ERROR, UNSUPPORTED_ERROR = 30000, 50002
_WIDTH = {"i8": 1, "i16": 2, "i32": 4, "i64": 8, "f32": 4, "f64": 8, "bool": 1}
DEPTH16 = [c(1)] * 16 + [("+",)] * 15                               # 31 instructions, 16 values on the stack
LEN64 = [c(0)] + [c(1), ("+",)] * 31 + [("not",)]                   # 64 instructions
ACCEPTS = [("depth 16", DEPTH16), ("64 instructions", LEN64)] + [
    ("%s ends at the row's last byte" % name, [(name, STRIDE - w)]) for name, w in _WIDTH.items()]
REJECTS = [
    # (what, program, rows relative to the table, error code, words of last_error)
    ("depth 17", [c(1)] * 17 + [("+",)] * 16, 0, USER_ERROR, "stack depth"),
    ("65 instructions", [c(0)] + [c(1), ("+",)] * 32, 0, UNSUPPORTED_ERROR, "more than 64 instructions"),
    ("opcode 0", [(0, 0)], 0, USER_ERROR, "unknown opcode"),
    ("opcode 26", [c(1), c(1), (26, 0)], 0, USER_ERROR, "unknown opcode"),
    ("negative offset", [("i8", -1)], 0, USER_ERROR, "offset outside the row"),
    ("offset INT32_MAX", [("i64", 2 ** 31 - 1)], 0, USER_ERROR, "offset outside the row"),
    ("two values left", [c(1), c(2)], 0, USER_ERROR, "exactly one value"),
    ("binary operator on one value", [c(1), ("+",)], 0, USER_ERROR, "underflow"),
    ("not on an empty stack", [("not",)], 0, USER_ERROR, "underflow"),
    ("rows shorter than the table", [c(1)], -1, USER_ERROR, "shorter than the table"),
] + [("%s one byte past the row" % name, [(name, STRIDE - w + 1)], 0, USER_ERROR, "offset outside the row") for name, w in _WIDTH.items()]


def test_reject_and_accept_lists_are_what_they_claim():
    """stack discipline restated: depth and length of every listed program, from the list alone"""
    def walk(prog):
        sp = depth = 0
        for ins in prog:
            op = ins[0]
            if op in ("const", "dist", "bool") or op in _WIDTH:
                sp += 1
            elif op == "not":
                assert sp >= 1
            else:
                assert sp >= 2
                sp -= 1
            depth = max(depth, sp)
        return sp, depth
    assert walk(DEPTH16) == (1, 16) and walk(LEN64) == (1, 2) and len(LEN64) == 64
    by = {r[0]: r for r in REJECTS}
    assert walk(by["depth 17"][1]) == (1, 17) and len(by["depth 17"][1]) <= 64
    assert walk(by["65 instructions"][1]) == (1, 2) and len(by["65 instructions"][1]) == 65
    assert walk(by["two values left"][1]) == (2, 2)
    for name, w in _WIDTH.items():
        assert dict(ACCEPTS)["%s ends at the row's last byte" % name][0][1] + w == STRIDE
        assert by["%s one byte past the row" % name][1][0][1] + w == STRIDE + 1
