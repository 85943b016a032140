"""What the DEVICE stores in its mirrors and what ONE launch of the filter kernel lets through, held to the fp64 reference of
tests/mirror_ref.py (GpuIndex.mirror_view / filter_pass: eps_index_mirror_view / eps_index_filter_pass).  Nothing here compares one
engine of the library with another: (a) the build's and the preparation kernels' arrays against fp64 norms and constants, (b) every pair
within an imposed threshold distance is reported (the library's contract, no tolerance), (c) the 8-bit tile reports exactly the pairs
whose integer accumulator reaches the threshold, (d) the fp16 tile decides every pair outside the accumulation band as the fp64 dot
product of its fp16 operands says, (e) neither entry leaves anything behind that a search could see.

A failing pair is printed with query, row, accumulator, threshold and tile coordinates (row // 256, row % 32, query column)."""
import numpy as np
import pytest

import mirror_ref as mr
import test_bound_math as bm
from helpers import data

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


from exact_ref import embedding_like, unit  # noqa: E402  (the tables both fp64 references are fed with)


def forced_row_table(rng, n, d):
    X = rng.random((n, d), dtype=F)
    X[n // 3, 5] = F(30000.0)   # its row constant leaves the accumulator's range: a forced row
    X[n // 2, 7] = F(40.0)      # a clamped value: the row carries its own residual
    return X


TABLES = {
    "uniform": lambda r, n, d: r.random((n, d), dtype=F),
    "gaussian": bm.CASES["gaussian"],
    "far from the origin": bm.CASES["far from the origin"],
    "columns with their own means": bm.CASES["columns with their own means"],
    "outliers and a forced row": forced_row_table,
    "embedding-like": embedding_like,
}


def make_queries(rng, X, nq, metric):
    d = X.shape[1]
    Q = np.stack([X[rng.integers(len(X))] + F(0.05) * rng.standard_normal(d).astype(F) for _ in range(nq)]).astype(F)
    Q[1] = X[rng.integers(len(X))] * F(40.0) - F(7.0)   # far outside the grid: clamped codes
    Q[2] = 0                                             # a zero query
    if metric == 1:
        Q[3:] = unit(Q[3:])
    return Q


def open_index(amd, X, metric):
    ix = amd.GpuIndex(X.shape[1], metric)
    ix.attach_rows(X)
    return ix


def view8(ix, Q):
    v = ix.mirror_view(8, Q)
    v["Q"] = Q
    return v


def pairs(mask):
    return set(map(tuple, np.argwhere(mask).tolist()))


explain = mr.explain_pairs


def check_view(v, X, Q, metric):
    mr.check_codes(v, X)
    mr.check_row_constants(v, X, metric)
    mr.check_query_constants(v, Q, metric)


def versus_restatement(v, X, metric):
    """(identity frame) the restatement on the view's own grid: the codes are the same fp32 sequence, and so - since the restatement sums R
    in the kernel's own order (test_bound_math.lane_dot) and divides through the reciprocal as the kernel does - is acc0: zero differences
    in both.  This is what sees an acc0 that is short by less than check_row_constants' fp32 allowance."""
    m = bm.mirror(X, metric, mu=np.asarray(v["mu8"][:v["dim"]], F), step=F(v["step"]))
    n = v["n"]
    dc = int((m["xi"] != v["x8"][:n, :v["dim"]]).sum())
    da = m["acc0"] - v["acc0"][:n].astype(np.int64)
    print("[pin] values that differ from the restatement: codes %d of %d, acc0 %d of %d" % (dc, m["xi"].size, int((da != 0).sum()), n))
    assert dc == 0, "%d codes differ from the restatement" % dc
    assert np.array_equal(m["forced"], np.isinf(v["erow"][:n]))
    bad = np.flatnonzero(da)
    assert len(bad) == 0, "acc0 differs from the restatement on %d of %d rows; row %d: device %d, restatement %d" % (
        len(bad), n, bad[0], v["acc0"][bad[0]], m["acc0"][bad[0]])


def sound_pass(ix, v, X, Q, metric, bits, fracs=(0.001, 0.02, 0.3)):
    """(b): every pair within the threshold distance is in the list the device returns"""
    n = len(X)
    d64 = mr.dist64(X, Q, metric)
    srt = np.sort(d64, axis=0)
    for frac in fracs:
        t64 = srt[int(frac * n)]          # exactly the distance of an existing row, rounded UP to fp32: that row is inside
        thr = t64.astype(F)
        thr = np.where(thr.astype(np.float64) < t64, np.nextafter(thr, F(np.inf)), thr).astype(F)
        need = mr.must_pass(v, X, Q, metric, thr)
        cnt, lists, T = ix.filter_pass(Q, bits, 0, n, n, thr, thr_is_distance=True)
        got = np.zeros_like(need)
        for j, rows in enumerate(lists):
            assert len(rows) == cnt[j] <= n and len(set(rows.tolist())) == len(rows)
            got[rows, j] = True
        missing = pairs(need & ~got)
        if missing:   # (accumulators and thresholds in ONE unit: fp16 thresholds are keys, T = s x accumulator)
            ref, Tacc = (mr.acc8(v), T) if bits == 8 else (mr.approx16(v), T.astype(np.float64) * (-0.5 if metric == 0 else -1.0))
            raise AssertionError("bits %d, quantile %g: %d pairs within the threshold were not reported: %s" % (bits, frac, len(missing), explain(missing, ref, Tacc)))
    return cnt


# ------------------------------------------------------------------------------------------------ (a) + (b)
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_stored_constants_and_soundness(amd, table, metric):
    rng = np.random.default_rng(sorted(TABLES).index(table) * 10 + metric)
    n, d, nq = 3001, 96, 12
    X = TABLES[table](rng, n, d)
    if metric == 1:
        X = unit(X)
    Q = make_queries(rng, X, nq, metric)
    ix = open_index(amd, X, metric)
    v = view8(ix, Q)
    assert v["n"] == n and v["n_pad"] == 3072 and v["d_pad"] == 512
    if not v["usable"]:   # IP / COSINE far from the origin: most row constants leave int32, the device declines the table - as the restatement does
        assert metric != 0 and table == "far from the origin" and bm.mirror(X, metric)["forced"].mean() > 0.01
    else:
        check_view(v, X, Q, metric)
        if table == "outliers and a forced row" and metric == 0:
            assert v["forced_rows"] == 1 and v["fold"] == 1 and np.isinf(v["erow"][n // 3]) and v["acc0b"][n // 3] == mr.ACC_FORCE
        if not v["rot"]:
            versus_restatement(v, X, metric)
        sound_pass(ix, v, X, Q, metric, 8)
        tile_on_this_table(ix, v, Q, "%s metric %d" % (table, metric))
    v16 = ix.mirror_view(16, Q)
    if v16["usable"]:
        sound_pass(ix, v16, X, Q, metric, 16)
    ix.close()


@pytest.mark.parametrize("rotate", [None, "0", "1"])
def test_embedding_like_rows_in_either_frame(amd, monkeypatch, rotate):
    if rotate is None:
        monkeypatch.delenv("EPS_MIRROR_ROTATE", raising=False)
    else:
        monkeypatch.setenv("EPS_MIRROR_ROTATE", rotate)
    rng = np.random.default_rng(77)
    n, d = 2500, 768
    X = embedding_like(rng, n, d)
    Q = embedding_like(rng, 8, d)
    ix = open_index(amd, X, 1)
    v = view8(ix, Q)
    assert v["usable"] and v["rot"] == (0 if rotate == "0" else 1), (rotate, v["rot"])
    check_view(v, X, Q, 1)
    if not v["rot"]:
        versus_restatement(v, X, 1)
    sound_pass(ix, v, X, Q, 1, 8)
    v16 = ix.mirror_view(16, Q)
    assert v16["usable"] and v16["version"] == 7
    sound_pass(ix, v16, X, Q, 1, 16)
    for m in (1, 17, 300):   # (c) on this table's operands: the rotated frame's codes, clamped where the grid cuts the tails
        T = mth_best(cached_acc8(v), 0, n, m)
        exact_sets(ix, v, Q, 0, n, T, 1024, what="embedding-like rotate %s m %d" % (rotate, m))
        exact_sets(ix, v, Q, 256, n, T + 1, 1024, what="embedding-like rotate %s m %d T + 1" % (rotate, m))
    ix.close()


@pytest.mark.parametrize("d", [1, 33, 100, 333, 512, 513, 768, 1000, 1536])
def test_every_row_width(amd, d):
    rng = np.random.default_rng(d)
    for n in (200, 777):   # n < 256; n not a multiple of 256
        X = rng.random((n, d), dtype=F)
        Q = make_queries(rng, X, 5, 0)
        ix = open_index(amd, X, 0)
        v = view8(ix, Q)
        assert v["usable"] and v["d_pad"] == max(512, (d + 255) // 256 * 256) and v["n_pad"] == (n + 255) // 256 * 256
        check_view(v, X, Q, 0)
        if not v["rot"]:
            versus_restatement(v, X, 0)
        sound_pass(ix, v, X, Q, 0, 8, fracs=(0.02, 0.3))
        v16 = ix.mirror_view(16, Q)   # v3 where d_pad is not a multiple of 128 or below 256, v7 otherwise; one row tile with a tail
        assert v16["usable"] and v16["d_pad"] == (d + 63) // 64 * 64 and v16["version"] == (3 if v16["d_pad"] % 128 or v16["d_pad"] < 256 else 7)
        sound_pass(ix, v16, X, Q, 0, 16, fracs=(0.02, 0.3))
        ix.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_rows_appended_after_the_grid_was_fixed(amd, metric):
    rng = np.random.default_rng(5 + metric)
    n, d = 2000, 96
    X = rng.random((n, d), dtype=F)
    Xa = np.concatenate([X[:150] + F(0.2) * np.sign(rng.standard_normal((150, d))).astype(F), X[150:300]])   # up to 20 % of the range outside the grid
    Q = make_queries(rng, X, 8, metric)
    ix = open_index(amd, X, metric)
    v0 = view8(ix, Q)
    ix.append_rows(Xa)
    rows = np.concatenate([X, Xa])
    v = view8(ix, Q)
    assert v["extended_rows"] == len(Xa) and v["n"] == len(rows) and v["step"] == v0["step"] and np.array_equal(v["mu8"], v0["mu8"])
    for name in ("x8", "acc0", "erow", "hrow"):   # constants of the old rows: unchanged byte for byte
        assert np.array_equal(v[name][:n].view(np.uint8), v0[name][:n].view(np.uint8)), name
    assert (np.abs(v["x8"][n:n + 150].astype(int)) == 127).any(), "no clamped code among the rows outside the grid"
    check_view(v, rows, Q, metric)
    versus_restatement(v, rows, metric)
    sound_pass(ix, v, rows, Q, metric, 8)
    tile_on_this_table(ix, v, Q, "appended rows metric %d" % metric)
    sound_pass(ix, ix.mirror_view(16, Q), rows, Q, metric, 16)
    ix.close()


def test_the_8bit_pass_is_not_vacuous(amd):
    """U[0,1) rows at d = 768, thr at the 0.1 % quantile: the device passes no more rows than the restatement's own pass count x 1.05 + 8 per
    query (the 5 % covers maxima that differ in the last bits; the restatement, not the kernel, sets the figure)"""
    n, d, nq = 20_000, 768, 16
    X, Q = data(n, d, 1), data(nq, d, 2)
    ix = open_index(amd, X, 0)
    v = view8(ix, Q)
    check_view(v, X, Q, 0)
    cnt = sound_pass(ix, v, X, Q, 0, 8, fracs=(0.001,))
    r = mr.restated_view(X, Q, 0, mu=np.asarray(v["mu8"][:d], F), step=F(v["step"]))
    t64 = np.sort(mr.dist64(X, Q, 0), axis=0)[int(0.001 * n)]
    thr = t64.astype(F)
    thr = np.where(thr.astype(np.float64) < t64, np.nextafter(thr, F(np.inf)), thr).astype(F)
    own = (mr.acc8(r) >= mr.thresholds8(r, thr)[None, :]).sum(0)
    print("[pin] rows passed per query, device / restatement:", cnt.tolist(), own.tolist())
    assert (cnt <= own * 1.05 + 8).all() and (cnt < n // 4).all(), (cnt, own)
    ix.close()


# ------------------------------------------------------------------------------------------------ (c)
def full_range_table(rng, n, d):
    """rows drawn uniformly on the grid's 255 levels per column with independent signs: every K-position carries its own information"""
    return (rng.integers(-127, 128, (n, d)).astype(F) / F(127.0)).astype(F)


def one_hot_table(rng, n, d):
    X = np.zeros((n, d), F)
    X[np.arange(n), np.arange(n) % d] = 1.0
    return X


def cached_acc8(v, folded=None):
    key = ("acc8", bool(v["fold"]) if folded is None else folded)
    if key not in v:
        v[key] = mr.acc8(v, folded)
    return v[key]


def exact_sets(ix, v, Q, lo, hi, T, cap, mode="ids", folded=None, what=""):
    """one pass with raw thresholds against acc8 >= T (mirror_ref.check_pass): the counts exactly, the lists as sets exactly (as a
    duplicate-free subset of cap entries when cap is smaller than the count)"""
    acc = cached_acc8(v, folded)
    cnt, lists, Tu = ix.filter_pass(Q, 8, lo, hi, cap, np.asarray(T, np.int32), mode=mode)
    assert np.array_equal(Tu, np.asarray(T, np.int32))
    mr.check_pass(acc, lo, hi, np.asarray(T, np.int64), cap, cnt, lists if mode == "ids" else [rows for _, rows in lists], what)
    return lists


def mth_best(acc, lo, hi, m):
    return np.sort(acc[lo:hi], axis=0)[::-1][m - 1]


def tile_on_this_table(ix, v, Q, what):
    """(c) on the operands of a table of (a) - clamped codes, the rotated frame, folded start values with clamped and forced rows: thresholds
    on the m-th best row's accumulator (every tie reported) and one unit above (none of them)"""
    n = v["n"]
    acc = cached_acc8(v)
    for lo, hi in ((0, n), (256, n - 100)):
        for m in (1, 17, 300):
            T = mth_best(acc, lo, hi, m)
            exact_sets(ix, v, Q, lo, hi, T, 1024, what="%s rows [%d, %d) m %d" % (what, lo, hi, m))
            exact_sets(ix, v, Q, lo, hi, T + 1, 1024, what="%s rows [%d, %d) m %d T + 1" % (what, lo, hi, m))


# every operand width x every batch shape (JQ = 1: <= 128 queries; JQ = 2 with a padded last query tile; several 256-query tiles) at 10 241
# rows; the two table sizes the ranges are meant for - 70 001 and 256 k + 1 = 262 145 rows - once each
SIZES = {(768, 257): 70_001, (512, 129): 256 * 1024 + 1}


@pytest.mark.parametrize("nq", [1, 31, 32, 33, 128, 129, 256, 257, 1100])
@pytest.mark.parametrize("d", [512, 768, 1024, 1536, 2048])
def test_the_8bit_tile_decides_what_its_operands_say(amd, d, nq):
    rng = np.random.default_rng(d + nq)
    n = SIZES.get((d, nq), 256 * 40 + 1)
    X = full_range_table(rng, n, d)
    Q = full_range_table(rng, nq, d)
    ix = open_index(amd, X, 0)
    v = view8(ix, Q)
    assert v["usable"] and v["d_pad"] == d and v["version"] == 7
    a, b = 3, n // 256 - 2
    acc = cached_acc8(v)
    for lo, hi in ((0, n), (256 * a, 256 * b), (256 * a, n), (256 * b, 256 * b + 256), (0, 256 * a + 77)):
        for m in (1, 17, 300):
            if m > hi - lo:
                continue
            T = mth_best(acc, lo, hi, m)
            what = "d %d nq %d rows [%d, %d) m %d" % (d, nq, lo, hi, m)
            exact_sets(ix, v, Q, lo, hi, T, 1024, what=what)              # ties at the boundary: all reported
            exact_sets(ix, v, Q, lo, hi, T + 1, 1024, what=what + " T + 1")   # ... and none of them one unit higher
    # thresholds that let everything / nothing through: exactly the rows of [lo, hi), no padding row, none beyond row_hi; cap < count
    T = mth_best(acc, 0, n, 17).copy()
    T[::3] = -(1 << 30)
    T[1::5] = 0x7FFFFFFF
    T[2::7] = 0x7F800000
    for lo, hi in ((0, n), (256 * b, n), (256, 256 * a + 5)):
        cap = 300 if nq > 300 else hi - lo
        exact_sets(ix, v, Q, lo, hi, T, cap, what="d %d nq %d rows [%d, %d) mixed thresholds" % (d, nq, lo, hi))
    ix.close()


@pytest.mark.parametrize("env", [{"EPS_MFMA_GROUPSYNC": "0"}, {"EPS_MFMA_SYNC_SHIFT": "0"}, {"EPS_MFMA_SYNC_SHIFT": "5"}])
def test_the_tile_under_the_group_switches(amd, monkeypatch, env):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    rng = np.random.default_rng(9)
    n, d, nq = 256 * 70 + 9, 768, 300
    X, Q = full_range_table(rng, n, d), full_range_table(rng, nq, d)
    ix = open_index(amd, X, 0)
    v = view8(ix, Q)
    for m in (1, 17, 300):
        exact_sets(ix, v, Q, 0, n, mth_best(cached_acc8(v), 0, n, m), 1024, what="%s m %d" % (env, m))
    ix.close()


def test_one_hot_rows_show_a_shifted_id(amd, monkeypatch):
    """rows that are zero except one column each (identity frame): a wrong K-offset or row permutation shows as a shifted id"""
    monkeypatch.setenv("EPS_MIRROR_ROTATE", "0")
    rng = np.random.default_rng(10)
    n, d, nq = 256 * 12 + 100, 768, 40
    X = one_hot_table(rng, n, d)
    Q = np.zeros((nq, d), F)
    Q[np.arange(nq), (np.arange(nq) * 37) % d] = 1.0
    ix = open_index(amd, X, 2)
    v = view8(ix, Q)
    check_view(v, X, Q, 2)
    assert not v["rot"]
    acc = mr.acc8(v)
    T = acc[(np.arange(nq) * 37) % d, np.arange(nq)]   # the accumulator of a row whose column is the query's (rows of one column are identical)
    lists = exact_sets(ix, v, Q, 0, n, T, 64, what="one-hot")
    for j, rows in enumerate(lists):
        assert set(np.flatnonzero(np.arange(n) % d == (j * 37) % d).tolist()) <= set(rows.tolist()), (j, rows)
    ix.close()


def test_a_forced_row_passes_every_threshold(amd):
    rng = np.random.default_rng(12)
    n, d, nq = 256 * 9 + 3, 768, 20
    X = forced_row_table(rng, n, d)
    Q = rng.random((nq, d), dtype=F)
    ix = open_index(amd, X, 0)
    v = view8(ix, Q)
    assert v["fold"] == 1 and v["forced_rows"] == 1
    check_view(v, X, Q, 0)
    for T in (mr.TQ_MAX8, mr.TQ_MAX8 - 1, 0):
        for rows in exact_sets(ix, v, Q, 0, n, np.full(nq, T, np.int64), n, what="forced row, T %d" % T):
            assert n // 3 in rows.tolist()
    # thresholds from distances are clamped to TQ_MAX8: a negative distance nothing can reach still reports the forced row, and only it
    cnt, lists, T = ix.filter_pass(Q, 8, 0, n, n, np.full(nq, -1e30, F), thr_is_distance=True)
    assert (T <= mr.TQ_MAX8).all() and all(rows.tolist() == [n // 3] for rows in lists), (T, cnt)
    ix.close()


def test_keys_and_dense_forms(amd):
    """keys mode: every (approximate distance, row) has the row in the reference set and the distance = C[q] - u x accumulator; dense mode:
    slot row - lo holds that row, for every row and query"""
    rng = np.random.default_rng(13)
    n, d, nq = 256 * 30 + 17, 768, 130
    for metric in (0, 2):
        X, Q = rng.random((n, d), dtype=F), rng.random((nq, d), dtype=F)
        ix = open_index(amd, X, metric)
        v = view8(ix, Q)
        acc = mr.acc8(v, folded=False)
        u, C = mr.key_unit(v), v["qstat"][:, 3].astype(np.float64)

        def keys_ok(dist, rows, j):
            ref = C[j] - u * acc[rows, j]
            # the kernel: (float)acc * s + C - the conversion of the integer, the product and the sum round once each (2^-24 relative to
            # |u acc|, |u acc| and the result), less where the compiler fuses the last two; L2 keys are clamped at 0
            tol = mr.EPS * (2.0 * np.abs(u * acc[rows, j]) + np.abs(ref)) * (1.0 + 1e-6)
            if metric == 0:
                ref = np.maximum(ref, 0.0)
            assert (np.abs(dist.astype(np.float64) - ref) <= tol).all(), (metric, j, np.abs(dist - ref).max(), tol.max())

        T = mth_best(acc, 0, n, 17)
        lists = exact_sets(ix, v, Q, 0, n, T, 512, mode="keys", folded=False, what="keys")
        for j, (dist, rows) in enumerate(lists):
            keys_ok(dist, rows, j)
        S0 = 4096
        cnt, lists, _ = ix.filter_pass(Q, 8, 256, 256 + S0, S0, None, mode="dense")
        assert (cnt == S0).all()
        for j, (dist, rows) in enumerate(lists):
            assert np.array_equal(rows, 256 + np.arange(S0)), j
            keys_ok(dist, rows, j)
        ix.close()


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("d,version", [(256, 7), (768, 7), (1024, 7), (33, 3), (100, 3), (192, 3)])
def test_the_fp16_tile_decides_what_its_operands_say(amd, d, version):
    n, nq = (100_000 if d >= 768 else 20_000), 32   # (m = 300 must lie within the 0.3 % quantile where the band is widest)
    X, Q = data(n, d, 20 + d), data(nq, d, 21 + d)
    host = mr.host_view16(X, Q, 0)
    a_host = np.sort(mr.approx16(host), axis=0)[::-1]
    worst = 0.0
    runs = []
    for m in (1, 17, 300, int(0.003 * n)):   # at or below the 0.3 % quantile of each query's approximate keys, where a stage's thresholds live
        Tq = a_host[m - 1]
        share = (np.abs(mr.approx16(host) - Tq[None, :]) <= mr.band16(host)).mean()
        assert share <= 1e-3, "undecided share %g of the chosen input (d %d, m %d): choose a tighter threshold" % (share, d, m)   # before the device is asked
        worst = max(worst, share)
        runs.append((m, Tq))
    ix = open_index(amd, X, 0)
    v = ix.mirror_view(16, Q)
    assert v["usable"] and v["version"] == version and v["d_pad"] == (d + 63) // 64 * 64
    assert np.array_equal(v["xh"][:n, :d], X.astype(np.float16)) and not v["xh"][n:].any() and not v["xh"][:, d:].any()
    assert np.array_equal(v["qh"][:, :d], Q.astype(np.float16)) and np.isneginf(v["start"][n:]).all()
    assert np.abs(v["start"][:n] + 0.5 * (X.astype(np.float64) ** 2).sum(1)).max() <= mr.rerank_slack(d) * v["xn"][:n].max()
    a = mr.approx16(v)
    band = mr.band16(v)
    seen = 0.0
    for m, Tq in runs:
        T = (F(-2.0) * Tq.astype(F)).astype(F)          # T in key space: the kernel compares acc >= T / s, s = -2 (exact)
        Tacc = T.astype(np.float64) * -0.5
        cnt, lists, _ = ix.filter_pass(Q, 16, 0, n, n, T)
        got = np.zeros(a.shape, bool)
        for j, rows in enumerate(lists):
            assert len(rows) == cnt[j] and len(set(rows.tolist())) == len(rows)
            got[rows, j] = True
        decided = np.abs(a - Tacc[None, :]) > band
        seen = max(seen, 1.0 - decided.mean())
        wrong = pairs(decided & (got != (a >= Tacc[None, :])))
        assert not wrong, "d %d m %d: %d decided pairs differ: %s" % (d, m, len(wrong), explain(wrong, a, Tacc))
    print("[pin] fp16 d %d: largest undecided share, host-computed %.5f %%, on the device's operands %.5f %%" % (d, 100 * worst, 100 * seen))
    assert seen <= 1e-3
    ix.close()


# ------------------------------------------------------------------------------------------------ (e)
def test_probes_leave_nothing_behind(amd):
    n, d = 70_000, 768
    X, Q = data(n, d, 30), data(64, d, 31)
    ix = open_index(amd, X, 0)

    def snapshot(q, engine):
        r = ix.search(q, 10, mode=amd.MODE_FLAT, flat_engine=engine)
        st = ix.stats()
        return r, (st["main_kernel_bits"], st["one_pass"])

    before = [snapshot(Q, amd.FLAT_MFMA_I8), snapshot(Q, amd.FLAT_MFMA), snapshot(Q[:1], amd.FLAT_MFMA_I8), snapshot(Q[:1], amd.FLAT_MFMA_I8)]
    assert before[3][1][1] == 1, before[3][1]
    st0 = ix.stats()
    ix.mirror_view(8, Q[:9])
    ix.mirror_view(16, Q[:9])
    ix.filter_pass(Q[:9], 8, 256, 5000, 64, np.full(9, -(1 << 30), np.int32))
    ix.filter_pass(Q[:9], 16, 0, n, 64, np.full(9, 1.0, F), thr_is_distance=True)
    assert ix.stats() == st0, "a probe changed the statistics of the last search"
    # the one-pass search right after a probe: still exact, and on its second repetition still the one-pass form
    stream = ix.search(Q[:1], 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    for rep in range(2):
        r, st = snapshot(Q[:1], amd.FLAT_MFMA_I8)
        assert all(np.array_equal(x, y) for x, y in zip(r, stream)), rep
    assert st[1] == 1, st
    after = [snapshot(Q, amd.FLAT_MFMA_I8), snapshot(Q, amd.FLAT_MFMA), snapshot(Q[:1], amd.FLAT_MFMA_I8), snapshot(Q[:1], amd.FLAT_MFMA_I8)]
    for (r0, s0), (r1, s1) in zip(before, after):
        assert s0 == s1 and all(np.array_equal(x, y) for x, y in zip(r0, r1))
    ix.close()


def test_probes_refuse_what_they_cannot_serve(amd):
    X = data(3000, 64, 1)
    grp = amd.GpuIndex(64, 0, devices=[0, 0])
    for s in range(2):
        grp.attach_shard_rows(s, X[s::2])
    for call in (lambda: grp.mirror_view(8, X[:2]), lambda: grp.filter_pass(X[:2], 8, 0, 256, 16, np.zeros(2, np.int32))):
        with pytest.raises(amd.EpsillaError) as e:
            call()
        assert e.value.code == 50002 and grp.L.eps_index_last_error_class(grp.h) == 0
    grp.close()
    ix = open_index(amd, X, 0)
    for bad in (dict(lo=100, hi=500), dict(lo=0, hi=3001), dict(lo=512, hi=512)):
        with pytest.raises(amd.EpsillaError) as e:
            ix.filter_pass(X[:2], 8, bad["lo"], bad["hi"], 16, np.zeros(2, np.int32))
        assert e.value.code == 30000
    with pytest.raises(amd.EpsillaError):
        ix.filter_pass(X[:2], 8, 0, 3000, 100, None, mode="dense")   # one slot per row of the range
    ix.close()
