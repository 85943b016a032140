"""tests/mirror_ref.py - the fp64 reference the GPU pin tests (test_gpu_mirror_pin.py) hold the device to - checked on the CPU: fed a view
made by the numpy restatement of tests/test_bound_math.py (mirror, query, fold, threshold, rotate_rows; imported, not copied), every checker
accepts it and `must_pass => acc8 >= T` holds, which ties the reference to the arithmetic the CPU suite already proves; and every checker
has teeth - each single mutation of the view below makes the matching checker fail."""
import zlib

import numpy as np
import pytest

import mirror_ref as mr
import test_bound_math as bm

F = np.float32
N, D, NQ = 1500, 96, 9


def make(case, metric, rot):
    rng = np.random.default_rng(zlib.crc32(("%s %d %d" % (case, metric, rot)).encode()))
    X = bm.CASES[case](rng, N, D)
    if metric == 1:
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = np.stack([X[rng.integers(N)] + F(0.05) * rng.standard_normal(D).astype(F) if j % 3 else bm.CASES[case](rng, 1, D)[0] * F(3.0) - F(1.0)
                  for j in range(NQ)]).astype(F)
    if metric == 1:
        Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(F)
    view = mr.restated_view(X, Q, metric, rot=bool(rot))
    if view["restated"]["forced"].mean() > 0.01:
        assert metric != 0 and case in ("far from the origin", "tiny range")   # as in test_bound_math: the device declines such a table
        return X, Q, None   # (row constants beyond int32: no 8-bit mirror for this table, nothing to check)
    return X, Q, view


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("case", sorted(bm.CASES))
def test_the_reference_accepts_the_restatement(case, metric, rot):
    X, Q, view = make(case, metric, rot)
    if view is None:
        return
    mr.check_codes(view, X)
    mr.check_row_constants(view, X, metric)
    mr.check_query_constants(view, Q, metric)
    acc = mr.acc8(view)
    d64 = mr.dist64(X, Q, metric)
    for frac in (0.001, 0.02, 0.3):
        thr = np.sort(d64, axis=0)[int(frac * N)].astype(F)
        thr = np.where(thr.astype(np.float64) < np.sort(d64, axis=0)[int(frac * N)], np.nextafter(thr, F(np.inf)), thr)   # (rounded up: that row is inside)
        need = mr.must_pass(view, X, Q, metric, thr)
        assert need.sum() >= NQ * (int(frac * N) + 1)
        T = mr.thresholds8(view, thr)
        missed = need & ~(acc >= T[None, :])
        assert not missed.any(), (case, metric, rot, frac, np.argwhere(missed)[:4])
        if not view["fold"]:   # a table that folds is also sound in its table-wide form wherever rows are tested
            continue
        Tw = mr.thresholds8(view, thr, folded=False)
        ok = ~view["restated"]["forced"]
        assert not (need & ~(mr.acc8(view, folded=False) >= Tw[None, :]))[ok].any()


# ------------------------------------------------------------------------------------------------ teeth
def rejected(check, *a):
    try:
        check(*a)
    except AssertionError:
        return True
    return False


def mutated(view, **repl):
    v = dict(view)
    v.update(repl)
    return v


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_every_checker_rejects_its_mutation(metric, rot, capsys):
    case = "uniform"
    X, Q, view = make(case, metric, rot)
    mr.check_codes(view, X)
    mr.check_row_constants(view, X, metric)
    mr.check_query_constants(view, Q, metric)
    assert rejected(mr.check_row_constants, mutated(view, erow=view["erow"] * F(0.99)), X, metric), "erow x 0.99 accepted"
    assert rejected(mr.check_row_constants, mutated(view, hrow=view["hrow"] * F(0.99)), X, metric), "hrow x 0.99 accepted"
    # acc0 lowered by its fp32 allowance + 2: the amount below which check_row_constants cannot see (per table; printed for the record)
    allow = mr.acc0_allowance(view)
    low = view["acc0"].copy()
    low[:view["n"]] -= int(np.ceil(allow)) + 2
    with capsys.disabled():
        print("\n[mirror_ref] acc0 allowance, %s metric %d rot %d: %.2f accumulator units (+ 2 for ceil + 1)" % (case, metric, rot, allow))
    assert rejected(mr.check_row_constants, mutated(view, acc0=low), X, metric), "acc0 lowered by allowance + 2 accepted"
    qs = view["qstat"].copy()
    qs[:, 2] *= F(0.9)
    assert rejected(mr.check_query_constants, mutated(view, qstat=qs), Q, metric), "qstat[2] x 0.9 accepted"
    x8 = view["x8"].copy()
    r, c = 700, 41
    x8[r, c] += 2 if x8[r, c] < 100 else -2
    assert rejected(mr.check_codes, mutated(view, x8=x8), X), "one code off by 2 accepted"
    x8 = view["x8"].copy()
    x8[:, [3, 57]] = x8[:, [57, 3]]
    assert rejected(mr.check_codes, mutated(view, x8=x8), X), "two code columns swapped accepted"
    x8 = view["x8"].copy()
    x8[11, mr.cols(view) + (5 if mr.cols(view) + 5 < view["d_pad"] else -1)] = 1
    assert mr.cols(view) < view["d_pad"]
    assert rejected(mr.check_codes, mutated(view, x8=x8), X), "nonzero code in a padding column accepted"


def test_the_pass_comparison_rejects_a_wrong_tile():
    """check_pass - what (c) of the GPU file holds every launch to - accepts the lists that acc8 >= T gives and rejects: lists computed with
    T + 3 on a threshold placed at a row's accumulator, one row too many in a count, a duplicate id, an id beyond row_hi, an id before row_lo,
    a short list under a cap, a missing tie"""
    X, Q, view = make("uniform", 0, 0)
    acc = mr.acc8(view)
    lo, hi, cap = 256, 1300, 64
    T = np.sort(acc[lo:hi], axis=0)[::-1][16]          # every query's threshold sits on its 17th best row's accumulator
    T[5] = -(1 << 30)                                  # ... one lets every row of the range through: a full list

    def passed(T_used):
        want = acc[lo:hi] >= T_used[None, :]
        return want.sum(0), [lo + np.flatnonzero(want[:, j])[:cap] for j in range(want.shape[1])]

    cnt, lists = passed(T)
    assert cnt[5] == hi - lo > cap and (cnt[:5] >= 17).all()
    mr.check_pass(acc, lo, hi, T, cap, cnt, lists)
    assert rejected(mr.check_pass, acc, lo, hi, T, cap, *passed(T + 3)), "lists computed with T + 3 accepted"
    low = [l.copy() for l in lists]
    low[2][0] = lo + int(np.argmin(acc[lo:hi, 2]))     # the row furthest below query 2's threshold, in place of one that passed
    assert rejected(mr.check_pass, acc, lo, hi, T, cap, cnt, low), "a row below the threshold accepted"
    c2 = cnt.copy()
    c2[3] += 1
    assert rejected(mr.check_pass, acc, lo, hi, T, cap, c2, lists), "a count one too high accepted"
    dup = [l.copy() for l in lists]
    dup[1][-1] = dup[1][0]
    assert rejected(mr.check_pass, acc, lo, hi, T, cap, cnt, dup), "a duplicate id accepted"
    for row in (hi, lo - 1, view["n"] + 3):
        far = [l.copy() for l in lists]
        far[5][7] = row                                # (query 5 passes every row: only the range can object)
        assert rejected(mr.check_pass, acc, lo, hi, T, cap, cnt, far), "row %d outside [%d, %d) accepted" % (row, lo, hi)
    short = [l.copy() for l in lists]
    short[5] = short[5][:-1]
    assert rejected(mr.check_pass, acc, lo, hi, T, cap, cnt, short), "a short full list accepted"
    gone = [l.copy() for l in lists]
    gone[0] = gone[0][:-1]
    assert rejected(mr.check_pass, acc, lo, hi, T, cap, cnt, gone), "a missing row accepted"


def test_acc8_is_exact_integer_arithmetic():
    """the float64 BLAS product of full-range codes equals the int64 product: |dot| <= 127^2 d_pad < 2^53"""
    rng = np.random.default_rng(5)
    x8 = rng.integers(-127, 128, (600, 2048)).astype(np.int8)
    q8 = rng.integers(-127, 128, (40, 2048)).astype(np.int8)
    x8[0], q8[0] = 127, 127
    view = dict(n=600, x8=x8, q8=q8, acc0=np.arange(600, dtype=np.int32), fold=0)
    assert np.array_equal(mr.acc8(view), x8.astype(np.int64) @ q8.astype(np.int64).T + np.arange(600)[:, None])


def test_fp16_undecided_share_of_the_chosen_inputs():
    """(d) of the GPU file rests on this: with thresholds at the 0.3 % quantile of each query's approximate keys, the pairs whose accumulator
    lies within the band of the threshold are at most 0.1 % of all pairs - from the reference alone, no device"""
    for d in (33, 100, 256):
        X = np.random.default_rng(d).random((6000, d), dtype=F)
        Q = np.random.default_rng(d + 1).random((16, d), dtype=F)
        v = mr.host_view16(X, Q, 0)
        a = mr.approx16(v)
        Tq = np.sort(a, axis=0)[::-1][int(0.003 * len(X))]
        share = (np.abs(a - Tq[None, :]) <= mr.band16(v)).mean()
        assert share <= 1e-3, (d, share)
