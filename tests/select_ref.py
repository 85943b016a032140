"""Reference for GpuIndex.select (eps_index_select): which rows are visible, restated in numpy.

The device judges a row with row_visible (csrc/device_common.hpp): deleted bit, then the int-column test, then the compiled program, evaluated on
a stack of doubles with `@distance` = 0 (a search's judging sites hand it the candidate's fp32 distance: `dist`) - ExprEvaluator's rules (query/expr/expr_evaluator.cpp:127-258: every number is a double, booleans are
0 / 1, MOD is fmod, a bool attribute is true iff its byte is non-zero).  Here the same program runs over ALL rows at once on a stack of float64
arrays; comparisons happen in double on both sides, so the two verdicts are equal bit for bit, no tolerance.  Checked on hand-written rows in
tests/test_select_cpu.py."""
import numpy as np

# geometry of csrc/select.hip (csrc/kernels.hpp): rows per block of the verdict / scatter launches, block counts per round of the scan's loop
SEL_ROWS = 1024
SEL_SCAN_THREADS = 512

_LOADS = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
_INT_OPS = {"<": np.less, "<=": np.less_equal, "==": np.equal, "=": np.equal, ">=": np.greater_equal, ">": np.greater, "!=": np.not_equal,
            "<>": np.not_equal}


def as_bytes(rows):
    """packed attribute rows (structured or 2-D array) as uint8 [n][stride]"""
    rows = np.ascontiguousarray(rows)
    return rows.view(np.uint8).reshape(rows.shape[0], -1)


# field sizes of the reference's packed attribute rows (FieldTypeSizeMVP; TableSegmentMVP::Init adds them up without padding,
# table_segment_mvp.cpp:84-86): a schema {BOOL, DOUBLE} puts the double at byte 1
_FIELDS = {"bool": np.uint8, "i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


def row_layout(fields, align=False):
    """fields: [(name, type)], type a key of _FIELDS -> (structured dtype, {name: byte offset}).  align=False: the reference's packing, one
    field right after the other; align=True: every field on a multiple of its size (the control layout).  Tests build their rows AND their
    programs' offsets from this one place."""
    dt = np.dtype([(name, _FIELDS[t]) for name, t in fields], align=align)
    return dt, {name: dt.fields[name][1] for name, _ in fields}


def eval_program(program, rows, dist=None):
    """program: postfix list as GpuIndex.set_filter_program takes it; rows: packed attribute rows; dist: what `@distance` reads per row
    (float64 [n]; the device pushes (double) of its fp32 distance, so callers pass d32.astype(np.float64)), None: 0, as in a select, a mask
    launch and a pre-filter call.  Returns the final stack value per row (float64 [n]); a row passes iff it is non-zero."""
    raw = as_bytes(rows)
    n = raw.shape[0]
    if dist is not None:
        dist = np.asarray(dist, np.float64)
        assert dist.shape == (n,)
    st = []
    with np.errstate(all="ignore"):
        for ins in program:
            op = ins[0]
            if op == "const":
                st.append(np.full(n, float(ins[1]), np.float64))
            elif op == "dist":
                st.append(np.zeros(n, np.float64) if dist is None else dist.copy())   # (None: LogicalEvaluate(root, id), no distance)
            elif op in _LOADS:
                dt = np.dtype(_LOADS[op])
                off = int(ins[1])
                st.append(np.ascontiguousarray(raw[:, off:off + dt.itemsize]).view(dt).reshape(n).astype(np.float64))
            elif op == "bool":
                st.append((raw[:, int(ins[1])] != 0).astype(np.float64))
            elif op == "not":
                st[-1] = (st[-1] == 0.0).astype(np.float64)
            else:
                b = st.pop()
                a = st[-1]
                if op == "+":
                    r = a + b
                elif op == "-":
                    r = a - b
                elif op == "*":
                    r = a * b
                elif op == "/":
                    r = a / b
                elif op == "%":
                    r = np.fmod(a, b)
                elif op == "<":
                    r = a < b
                elif op == "<=":
                    r = a <= b
                elif op == "=":
                    r = a == b
                elif op == "<>":
                    r = a != b
                elif op == ">=":
                    r = a >= b
                elif op == ">":
                    r = a > b
                elif op == "and":
                    r = (a != 0.0) & (b != 0.0)
                elif op == "or":
                    r = (a != 0.0) | (b != 0.0)
                elif op == "=b":
                    r = (a != 0.0) == (b != 0.0)
                elif op == "<>b":
                    r = (a != 0.0) != (b != 0.0)
                else:
                    raise ValueError("unknown instruction %r" % (op,))
                st[-1] = np.asarray(r, np.float64)
    assert len(st) == 1, "the program must leave exactly one value"
    return st[0]


def visible_rows(n, deleted=None, int_filter=None, program=None, rows=None, dist=None):
    """bool [n]: not deleted (bit i & 7 of byte i >> 3), passes `column <op> value` (int_filter = (values, op, value)), passes the program"""
    vis = np.ones(n, bool)
    if deleted is not None:
        vis &= np.unpackbits(np.asarray(deleted, np.uint8), bitorder="little")[:n] == 0
    if int_filter is not None:
        col, op, value = int_filter
        vis &= _INT_OPS[op](np.asarray(col)[:n].astype(np.int64), np.int64(value))
    if program:
        vis &= eval_program(program, rows[:n], dist)[:n] != 0.0
    return vis


def expected(visible, skip, limit, base=0, stride=1):
    """(ids of the window, total)"""
    return np.flatnonzero(visible)[skip:skip + limit].astype(np.int64) * stride + base, int(visible.sum())
