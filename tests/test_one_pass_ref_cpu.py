"""tests/one_pass_ref.py catches what it is for.  A numpy model of the one-pass search's pass (vectordb_amd/csrc/stream8_kernel.hpp) on the
restatement's view of a small table (tests/mirror_ref.py restated_view): the chunks of 16 rows dealt to W model wavefronts, every wavefront's
first offer, then the chunks in a seeded random interleaving - each tested against the threshold the table gives at that moment, appended to
the wavefront's list of 32, offered where it beats the k-th slot.  It produces what GpuIndex.one_pass_probe returns.  The honest model passes
(a)-(e); every planted fault is caught, by the check it belongs to."""
import numpy as np
import pytest

import exact_ref as er
import mirror_ref as mr
import one_pass_ref as opr

F = np.float32
N, D, W, CH, CAP = 6005, 96, 47, 16, 32   # (n % 16 = 5: a partial last chunk; 8 chunks per wavefront)


def table_of(rng, metric, forced=True, d=D):
    X = rng.random((N, d), dtype=F)
    X[100:130] = X[99]                    # a run of identical rows
    if forced:
        X[N // 3, 5] = F(30000.0)         # its row constant leaves the accumulator's range: a forced row
        X[N // 2, 7] = F(40.0)            # a clamped value: the row carries its own residual, the table folds
    if metric == 1:
        X = er.unit(X)
    return X


def queries_of(rng, X, nq, metric):
    Q = np.stack([X[rng.integers(len(X))] + F(0.05) * rng.standard_normal(X.shape[1]).astype(F) for _ in range(nq)]).astype(F)
    Q[0] = X[N - 3]                       # the best row of query 0 lies in the partial last chunk
    if nq > 1:
        Q[1] = X[105]                     # ... of query 1 in the run of identical rows
    if metric == 1:
        Q = er.unit(Q)
    return Q


def device_kth(t, k, fault=None):
    """stream8_threshold_of's rank arithmetic, lane by lane (64 slots: one per lane; 128: lane l holds slots l and l + 64)"""
    t = np.asarray(t, np.int64)
    lane = np.arange(64)
    if fault == "rank":
        k = k + 1
    if len(t) == 64:
        rank = ((t[None, :] > t[:, None]) | ((t[None, :] == t[:, None]) & (lane[None, :] < lane[:, None]))).sum(1)
        return int(t[np.flatnonzero(rank == k - 1)[0]])
    v, v1 = t[:64], t[64:]
    first = (v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & (lane[None, :] < lane[:, None]))
    upper = (v1[None, :] >= v[:, None]) if fault == "tie" else (v1[None, :] > v[:, None])   # (honest: slot i + 64 never precedes slot `lane` on a tie)
    r0 = first.sum(1) + upper.sum(1)
    r1 = (v[None, :] >= v1[:, None]).sum(1) + ((v1[None, :] > v1[:, None]) | ((v1[None, :] == v1[:, None]) & (lane[None, :] < lane[:, None]))).sum(1)
    m0, m1 = np.flatnonzero(r0 == k - 1), np.flatnonzero(r1 == k - 1)
    return int(v[m0[0]]) if len(m0) else int(v1[m1[0] if len(m1) else 63])


def model_pass(view, k, visible, seed=0, fault=None):
    n, nq = view["n"], len(view["q8"])
    fold = bool(view["fold"])
    slots = 64 if k <= 16 else 128
    form = dict(pieces=view["d_pad"] // 256, matrix=0, width=1 if nq == 1 else (2 if nq == 2 else 4), wide=int(slots == 128), prep_in_kernel=0, slots=slots, waves=W,
                fold=int(fold), rot=0, masked=0, wave_cap=CAP, chunk=CH)
    acc = mr.acc8(view, folded=fold and fault != "acc0")
    if fault == "piece":   # lane group row % 16 = 5 loses K piece 1
        rows = np.flatnonzero(np.arange(n) % 16 == 5)
        acc[rows] -= np.asarray(view["x8"])[rows, 256:512].astype(np.int64) @ np.asarray(view["q8"])[:, 256:512].astype(np.int64).T
    margin = (np.asarray(view["acc0b"]).astype(np.int64) - np.asarray(view["acc0"]).astype(np.int64))[:n] if fold else np.zeros(n, np.int64)
    off = opr.int32_wrap(acc - (1 if fault == "margin" else 2) * margin[:, None])   # (the device's int arithmetic: a forced row's "margin" is 0x78000000)
    slot = opr.slot_of(np.arange(n), slots)
    if fault == "hash":
        slot = (slot + 1) & (slots - 1)
    live_n = n - n % 16 if fault == "tail" else n
    table = np.full((nq, slots), opr.S8_EMPTY, np.int64)
    probe = dict(form=form, k=k, qstat=np.asarray(view["qstat"], F), kth=np.zeros(nq, np.int64), T_final=np.zeros(nq, np.int64))
    memo = {}

    def threshold(q):
        gk = device_kth(table[q], k)
        if (q, gk) not in memo:
            probe["kth"][q] = gk
            memo[q, gk] = opr.restated_threshold(view, probe, q)[0]
        return memo[q, gk], gk

    def offer(q, r):
        if (visible[r] or fault == "hidden") and (acc[r, q] < opr.FORCE_LIMIT or fault == "forced"):
            table[q, slot[r]] = max(table[q, slot[r]], off[r, q])

    rng = np.random.default_rng(seed)
    chunks = [list(range(w, (n + CH - 1) // CH, W)) for w in range(W)]
    for w in rng.permutation(W):           # every wavefront offers the best unforced row of its first chunk before anything is tested
        rows = np.arange(chunks[w][0] * CH, min(n, chunks[w][0] * CH + CH))
        for q in range(nq):
            ok = rows[acc[rows, q] < opr.FORCE_LIMIT]
            if len(ok):
                offer(q, ok[np.argmax(acc[ok, q])])
    cnt = np.zeros((nq, W), np.int64)
    raw = np.zeros((nq, W, CAP), np.uint64)

    def test_chunk(w, c):
        rows = np.arange(c * CH, min(live_n, c * CH + CH))
        for q in range(nq):
            T, gk = threshold(q)
            for r in rows:
                a = int(acc[r, q])
                if a >= T:
                    if cnt[q, w] < CAP:
                        raw[q, w, cnt[q, w]] = np.uint64(((a & 0xFFFFFFFF) << 32) | int(r))
                    cnt[q, w] += 1
                if a > gk:
                    offer(q, r)

    for w in rng.permutation(W):           # the first chunks, then the stream in any order that keeps each wavefront's own
        test_chunk(w, chunks[w][0])
    todo = [w for w in range(W) for _ in chunks[w][1:]]
    at = [1] * W
    for w in rng.permutation(todo):
        test_chunk(w, chunks[w][at[w]])
        at[w] += 1
    for q in range(nq):
        probe["kth"][q] = device_kth(table[q], k, fault)
        probe["T_final"][q] = opr.restated_threshold(view, probe, q)[0]
    probe.update(raw_cnt=cnt, raw=raw, table=table)
    return probe


def case(metric, nq=3, forced=True, seed=0, hidden=0.2, d=D):
    rng = np.random.default_rng(100 * metric + seed)
    X = table_of(rng, metric, forced, d)
    Q = queries_of(rng, X, nq, metric)
    view = mr.restated_view(X, Q, metric)
    visible = rng.random(N) > hidden
    visible[N // 3] = True                # (the forced row is visible: only its start value keeps it out of the table)
    return X, Q, view, visible


_CASES = {}


def cached_case(metric, forced=True, d=D):
    if (metric, forced, d) not in _CASES:
        X, Q, view, visible = case(metric, forced=forced, d=d)
        _CASES[metric, forced, d] = (X, Q, view, visible, er.Ref(X, Q, metric))
    return _CASES[metric, forced, d]


@pytest.mark.parametrize("k", [1, 10, 16, 17, 64])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_the_honest_model_passes(metric, k):
    X, Q, view, visible, ref = cached_case(metric)
    if metric != 1:   # (unit rows have no outlier: COSINE runs the table-wide margin)
        assert view["fold"] == 1 and view["forced_rows"] >= 1, (view["fold"], view["forced_rows"])
    probe = model_pass(view, k, visible, seed=k)
    fig = opr.check_all(view, probe, visible, ref)
    print(opr.describe(probe, fig))
    assert fig["T_diff"] == 0   # (the model's T_final IS the restatement)
    # the checks had something to check: entries, a filled table, and - L2, where the toy table's margins leave the threshold some grip - lists that fit
    assert fig["entries"] > 0 and fig["filled"] >= min(k, 30) and (metric != 0 or k > 17 or fig["overflowed"] == 0)


@pytest.mark.parametrize("metric", [0, 2])
def test_the_honest_model_passes_on_a_table_that_does_not_fold(metric):
    X, Q, view, visible, ref = cached_case(metric, forced=False)
    assert view["fold"] == 0
    for k in (10, 17):
        opr.check_all(view, model_pass(view, k, visible, seed=3), visible, ref)
    opr.check_all(view, model_pass(view, 10, np.ones(N, bool), seed=4), None, ref)


def caught(tag, view, probe, visible, ref=None):
    with pytest.raises(AssertionError) as e:
        opr.check_all(view, probe, visible, ref)
    msg = str(e.value)
    assert msg.startswith(tag), msg
    return msg


@pytest.mark.parametrize("fault,tag", [("piece", "(a)"), ("acc0", "(a)"), ("hidden", "(b)"), ("forced", "(b)"), ("margin", "(b)"), ("rank", "(b)"), ("hash", "(b)"), ("tail", "(c)")])
def test_a_fault_in_the_pass_is_caught(fault, tag):
    # (a dropped K piece must leave the row a candidate to be seen in an ENTRY: 300 columns - the second 256-byte piece carries 44 of them)
    X, Q, view, visible, ref = cached_case(0, d=300 if fault == "piece" else D)
    opr.check_all(view, model_pass(view, 10, visible, seed=7), visible, ref)
    msg = caught(tag, view, model_pass(view, 10, visible, seed=7, fault=fault), visible, ref)
    print(msg)
    hint = dict(piece="without K piece 1", acc0="started from acc0", hidden="not visible", forced="forced", margin="ONE margin", rank="kth =", hash="whose slot is", tail="row %d " % (N - 3))[fault]
    assert hint in msg, msg
    if fault == "piece":
        assert "row % 16 = 5" in msg
    if fault == "tail":
        assert "query 0" in msg


def honest(k=10, seed=11):
    X, Q, view, visible, ref = cached_case(0)
    probe = model_pass(view, k, visible, seed=seed)
    opr.check_all(view, probe, visible, ref)
    return view, visible, ref, probe


def test_an_accumulator_off_by_one_is_caught():
    view, visible, ref, probe = honest()
    q, w = np.argwhere(probe["raw_cnt"] > 0)[5]
    probe["raw"][q, w, 0] += np.uint64(1 << 32)
    assert "difference 1" in caught("(a)", view, probe, visible, ref)


def test_a_row_exactly_at_the_threshold_must_be_listed():
    """a HIDDEN row (it never enters the table: nothing else changes) whose start value puts it exactly at T_final"""
    X, Q, view, visible, ref = cached_case(0)
    view = dict(view)
    probe = model_pass(view, 10, visible, seed=11)
    acc = opr.accumulators(view, probe)
    ovf = opr.overflowed(probe)
    q = 2
    r = next(int(r) for r in np.flatnonzero(~visible) if not ovf[q][opr.wave_of(r, probe["form"])] and acc[r, q] < probe["T_final"][q] and r not in (N // 3, N // 2))
    for name in ("acc0", "acc0b"):
        a = np.array(view[name])
        a[r] += int(probe["T_final"][q]) - int(acc[r, q])
        view[name] = a
    probe = model_pass(view, 10, visible, seed=11)
    acc = opr.accumulators(view, probe)
    assert acc[r, q] == probe["T_final"][q]
    opr.check_all(view, probe, visible)          # listed: the honest pass tests acc >= T
    w = int(opr.wave_of(r, probe["form"]))
    lst = probe["raw"][q, w, :probe["raw_cnt"][q, w]]
    keep = lst[(lst & np.uint64(0xFFFFFFFF)) != np.uint64(r)]
    assert len(keep) == len(lst) - 1
    probe["raw"][q, w, :len(keep)] = keep
    probe["raw_cnt"][q, w] -= 1
    msg = caught("(c)", view, probe, visible)
    assert "row %d " % r in msg and "exactly at the threshold" in msg, msg


def test_a_stale_looser_threshold_is_caught():
    view, visible, ref, probe = honest()
    # T_final as the table stood before its best slots arrived: the k-th slot of the table without its k largest values
    q = 0
    t = np.sort(probe["table"][q])[::-1]
    stale = dict(probe, kth=probe["kth"].copy())
    stale["kth"][q] = t[2 * probe["k"]]
    loose = opr.restated_threshold(view, stale, q)[0]
    assert loose < probe["T_final"][q] - opr.restated_threshold(view, probe, q)[1]
    probe["T_final"] = probe["T_final"].copy()
    probe["T_final"][q] = loose
    assert "query 0" in caught("(e)", view, probe, visible, ref)


def test_the_reversed_tie_rule_of_the_128_slot_table_is_caught():
    """two identical rows in slots l and l + 64 at ranks k - 1 and k of a 128-slot table: with `>=` where slot i + 64 is compared with slot `lane`
    both believe the other precedes them, no slot has rank k - 1, and the function returns whatever lane 63 holds"""
    k = 17
    rng = np.random.default_rng(5)
    X = table_of(rng, 0, forced=False)
    s128 = opr.slot_of(np.arange(N), 128)
    r1 = int(np.flatnonzero((s128 < 64) & (np.arange(N) < W * CH))[3])
    r2 = int(np.flatnonzero((s128 == s128[r1] + 64) & (np.arange(N) < W * CH))[0])   # both in first chunks: tested while the table is all but empty
    X[r2] = X[r1]
    Q = (X[[4000]] + F(0.05) * rng.standard_normal((1, D)).astype(F)).astype(F)
    view = mr.restated_view(X, Q, 0)
    acc = mr.acc8(view)[:, 0]
    assert acc[r1] == acc[r2]
    # visible: 16 rows above the pair (from later chunks), the pair, 30 rows below it - every one in a slot of its own, none in slot 127
    used = {int(s128[r1]), int(s128[r2]), 127}
    pick = []
    for want, rows in ((16, np.flatnonzero((acc > acc[r1]) & (np.arange(N) >= W * CH))), (30, np.flatnonzero(acc < acc[r1]))):
        got = 0
        for r in rows:
            if got < want and int(s128[r]) not in used:
                used.add(int(s128[r]))
                pick.append(int(r))
                got += 1
        assert got == want
    visible = np.zeros(N, bool)
    visible[pick + [r1, r2]] = True
    probe = model_pass(view, k, visible, seed=1)
    opr.check_all(view, probe, visible)
    assert probe["kth"][0] == acc[r1] and probe["table"][0, s128[r1]] == probe["table"][0, s128[r2]] == acc[r1]
    bad = model_pass(view, k, visible, seed=1, fault="tie")
    msg = caught("(b)", view, bad, visible)
    assert "kth =" in msg, msg
