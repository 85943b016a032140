"""What tests/test_gpu_stream_order.py is built from: WHEN a call reads its inputs and writes its outputs, not what it computes.

The device half (torch, imported where it is used):
  gate(stream, ms)        a chain of dependent 4096 x 4096 fp32 matmuls on `stream`, on tensors allocated once: the device is busy for about ms, the
                          host returns at once.  calibrate() times the matmul with events, once, and returns matmuls per millisecond.
  issued_behind(stream)   not stream.query(), read straight after a call returns: the call came back while the gate was still running.
  window(...)             the inputs of the call under test are valid ONLY at the call's own place in the stream:
                            1 before the gate the input tensors hold the decoy       4 on the stream, every output is cloned
                            2 behind the gate, on the stream, they receive the real  5 on the stream, the inputs receive the decoy again
                            3 the call under test is made                            6 the test ends in ONE stream.synchronize()
                          A read that comes too early or too late takes the decoy.
  gate_for(name, ...)     the gate's length is measured: the call sequence runs once warm without a gate, the host time to ISSUE it (perf_counter
                          around the calls, a sync on either side) times 4 - host jitter on a shared box - is the gate.  Both are printed with the
                          test's name; more than 0.5 s of gate means the sequence is too long for one test.
  pinned(shape, dtype)    a page-locked host array (torch.empty(...).pin_memory().numpy()).

The numpy half, used on the CPU before anything is launched (tests/test_stream_gate_cpu.py holds it to exact_ref and to planted swaps): tables of
small integers, whose L2 distances fp32 computes exactly in any order - so an answer is ids, distance BITS and counts, no tolerance - and the vacuity
condition of every case: for every query the decoy's exact answer differs from the real one in its FIRST id (differ_first); outputs start as -7."""
import math
import time
from contextlib import contextmanager

import numpy as np

import exact_ref as xr

F = np.float32
FILL = -7            # what every output holds before the call
MAX_GATE_S = 0.5
TABLE = "integers -8..8"


# ------------------------------------------------------------------------------------------------ numpy: exact answers on tables of small integers
def int_dists(X, Q):
    """exact L2 distances [n][nq] in fp64 (integers below 2^24: the fp32 distances of every engine, bit for bit)"""
    X, Q = np.asarray(X, np.float64), np.atleast_2d(np.asarray(Q, np.float64))
    d = (X * X).sum(axis=1)[:, None] + (Q * Q).sum(axis=1)[None, :] - 2.0 * (X @ Q.T)
    assert np.array_equal(d, np.rint(d)) and d.max(initial=0) < 2 ** 24 and d.min(initial=0) >= 0, "not a table of small integers"
    return d


def int_ref(X, Q):
    """exact_ref.Ref of (X, Q, L2) from int_dists (the same numbers as exact_ref.dist64 on such a table, without its n x nq x d temporaries)"""
    r = object.__new__(xr.Ref)
    Q = np.atleast_2d(Q)
    r.n, r.d, r.nq, r.metric = len(X), X.shape[1], len(Q), 0
    r.d64 = int_dists(X, Q)
    r.mag = r.d64
    return r


def _mask(n, nq, visible):
    """None, bool [n], or bool [n][nq] -> bool [n][nq] (or None)"""
    if visible is None:
        return None
    v = np.asarray(visible, bool)
    return v if v.ndim == 2 else np.repeat(v[:, None], nq, axis=1)


def topk_np(X, Q, k, visible=None, radius=None):
    """(ids [nq][k], dist [nq][k] fp32, counts int32 [nq], totals int64 [nq]): the k smallest (distance, row) over the visible rows - within
    radius[q] where one is given (totals: how many such rows there are); the rest -1 / +inf"""
    Q = np.atleast_2d(Q)
    n, nq = len(X), len(Q)
    assert n < (1 << 20)
    vis = _mask(n, nq, visible)
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F)
    counts = np.zeros(nq, np.int32)
    totals = np.zeros(nq, np.int64)
    rows = np.arange(n, dtype=np.int64)
    far = np.iinfo(np.int64).max
    for q0 in range(0, nq, 64):
        d = int_dists(X, Q[q0:q0 + 64])
        for j in range(d.shape[1]):
            q = q0 + j
            key = (d[:, j].astype(np.int64) << 20) | rows
            take = np.ones(n, bool) if vis is None else vis[:, q].copy()
            if radius is not None:
                take &= d[:, j].astype(F) <= F(radius[q])
            key[~take] = far
            totals[q] = int(take.sum())
            m = counts[q] = min(k, int(totals[q]))
            best = np.sort(np.partition(key, m - 1)[:m]) if m else key[:0]
            ids[q, :m] = best & ((1 << 20) - 1)
            dist[q, :m] = (best >> 20).astype(F)
    return ids, dist, counts, totals


def first_ids(X, Q, visible=None, radius=None):
    if visible is None and radius is None:      # (argmin: the first of equal minima, the smallest row)
        Q = np.atleast_2d(Q)
        return np.concatenate([int_dists(X, Q[q0:q0 + 64]).argmin(axis=0) for q0 in range(0, len(Q), 64)]).astype(np.int64)
    return topk_np(X, Q, 1, visible, radius)[0][:, 0]


def rows_mask(n, lists, nq):
    """ONE array of rows (every query's list) or nq of them -> bool [n][nq]"""
    m = np.zeros((n, nq), bool)
    for q in range(nq):
        m[np.asarray(lists if isinstance(lists, np.ndarray) else lists[q], np.int64), q] = True
    return m


def differ_first(real, decoy, what):
    """THE vacuity condition: the decoy's answer differs from the real one in every query's first id (real / decoy: first ids, or whole id arrays)"""
    real, decoy = np.asarray(real), np.asarray(decoy)
    if real.ndim > 1:
        real, decoy = real[:, 0], decoy[:, 0]
    assert real.shape == decoy.shape and real.size > 0, "%s: nothing to compare" % what
    eq = np.flatnonzero(real == decoy)
    assert len(eq) == 0, "%s: VACUOUS - the decoy gives query %d the first id %d of the real input too (%d of %d queries): change the decoy" % (
        what, eq[0], real[eq[0]], len(eq), real.size)


def same(got, want, what, names=("ids", "dist", "counts", "totals")):
    """ids, distance bit patterns, counts (, totals): no tolerance.  A failure says how the first differing query starts on both sides."""
    assert len(got) == len(want), "%s: %d arrays against %d" % (what, len(got), len(want))
    for g, w, name in zip(got, want, names):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s against %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == F:
            g, w = (g + F(0)).view(np.uint32), (w + F(0)).view(np.uint32)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s %s: %d of %d places differ, first at %s: got %r, expected %r" % (
            what, name, len(bad), g.size, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def starts_as_fill(outs, what):
    for o in outs:
        assert (np.asarray(o) == FILL).all(), "%s: an output does not start as %d" % (what, FILL)


def took(got_ids, real_ids, decoy_ids):
    """what a failed case read, for its message: 'real', 'decoy', 'a mix' or 'neither' (by first ids)"""
    g, r, d = (np.asarray(a).reshape(len(a), -1)[:, 0] for a in (got_ids, real_ids, decoy_ids))
    if (g == r).all():
        return "real"
    if (g == d).all():
        return "decoy"
    return "a mix" if ((g == r) | (g == d)).all() else "neither"


# ------------------------------------------------------------------------------------------------ device: the gate and the window
_G = {}


def _mats():
    import torch
    if "a" not in _G:
        _G["a"] = torch.rand(4096, 4096, device="cuda", dtype=torch.float32)
        _G["b"] = torch.eye(4096, device="cuda", dtype=torch.float32)      # (a x I: the chain's values stay what they are)
        _G["c"] = torch.empty_like(_G["a"])
        torch.cuda.synchronize()
    return _G["a"], _G["b"], _G["c"]


def _chain(n):
    import torch
    a, b, c = _mats()
    for _ in range(n):
        torch.mm(a, b, out=c)      # each reads what the one before wrote
        a, c = c, a


def calibrate():
    """matmuls of the gate per millisecond of device time (events around a chain, once)"""
    import torch
    if "per_ms" not in _G:
        _chain(4)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _chain(8)
        e1.record()
        torch.cuda.synchronize()
        _G["per_ms"] = 8.0 / max(e0.elapsed_time(e1), 1e-3)
        print("stream-gate: one 4096 x 4096 fp32 matmul takes %.3f ms" % (1.0 / _G["per_ms"]))
    return _G["per_ms"]


def gate(stream, ms):
    import torch
    n = max(1, int(math.ceil(ms * calibrate())))
    with torch.cuda.stream(stream):
        _chain(n)
    return n


def issued_behind(stream):
    return not stream.query()


def gate_for(name, issue, stream):
    """issue(): the test's call sequence (fresh outputs every time).  Runs it once warm, once timed -> the gate's length in ms"""
    issue()
    stream.synchronize()
    t0 = time.perf_counter()
    issue()
    t = time.perf_counter() - t0
    stream.synchronize()
    print("stream-gate: %-58s issue %8.3f ms  gate %8.3f ms" % (name, 1e3 * t, 4e3 * t))
    assert 4.0 * t <= MAX_GATE_S, "%s: issuing the calls takes %.3f s of host time, 4 x that exceeds %.1f s: split the sequence" % (name, t, MAX_GATE_S)
    return 4e3 * t


def pinned(shape, dtype):
    import torch
    t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name)).pin_memory()
    assert t.is_pinned()
    return t.numpy()


class Window:
    def __init__(self, stream):
        self.stream, self.snaps, self.behind = stream, None, None

    def returned(self, *outs):
        """straight after the call under test: was it issued behind the gate; its outputs as they are at this place in the stream"""
        import torch
        self.behind = issued_behind(self.stream)
        with torch.cuda.stream(self.stream):
            self.snaps = [o.clone() for o in outs]

    def numpy(self):
        return [s.cpu().numpy() for s in self.snaps]


@contextmanager
def window(stream, dst, real, decoy, ms):
    """dst, real, decoy: a device tensor each, or equally long lists of them.  The body makes the call and hands its outputs to w.returned();
    the caller ends the test with stream.synchronize() and reads w.numpy()."""
    import torch
    dst, real, decoy = ([x] if not isinstance(x, (list, tuple)) else list(x) for x in (dst, real, decoy))
    w = Window(stream)
    with torch.cuda.stream(stream):
        for t, v in zip(dst, decoy):
            t.copy_(v)
        stream.synchronize()
        gate(stream, ms)
        for t, v in zip(dst, real):
            t.copy_(v)
    yield w
    assert w.snaps is not None, "the body did not call returned()"
    with torch.cuda.stream(stream):
        for t, v in zip(dst, decoy):
            t.copy_(v)


# ------------------------------------------------------------------------------------------------ the cases, in numpy (inputs, their decoys, both answers)
# Every case is a dict: what the call under test gets (`real`), what stands in its place outside the call's window (`decoy`), the exact answer of
# each (`want`, `want_decoy`: tuples as the call returns them) and the names of its arrays.  check_case is the vacuity condition; a test compares
# what the device returned with case["want"] through same().
_T = {}
SHAPES = {"A": (20_001, 64), "B": (100_000, 128)}


def table(name):
    """'A' 20 001 x 64 (the fp32 forms), 'B' 100 000 x 128 (where a mirror is needed): integers -8..8, made once"""
    if name not in _T:
        n, d = SHAPES[name]
        _T[name] = xr.make(TABLE, n, d, 1, seed=77)[0]
    return _T[name]


def queries(tab, nq, seed):
    n, d = SHAPES[tab]
    return xr.make(TABLE, 8, d, nq, seed=seed)[1]


def search_case(tab, nq, k, seed=1):
    X = table(tab)
    Qr, Qd = queries(tab, nq, seed), queries(tab, nq, seed + 1000)
    fr = first_ids(X, Qr)
    for again in range(1, 9):      # (a thousand queries over 20 001 rows: a few decoys share their first id with the real query - those are drawn again)
        eq = np.flatnonzero(fr == first_ids(X, Qd))
        if len(eq) == 0:
            break
        Qd[eq] = queries(tab, nq, seed + 1000 + again)[eq]
    return dict(name="search %s nq %d k %d" % (tab, nq, k), tab=tab, k=k, real=(Qr,), decoy=(Qd,), want=topk_np(X, Qr, k)[:3], want_decoy=topk_np(X, Qd, k)[:3],
                names=("ids", "dist", "counts"))


def range_case(tab, nq=4, cap=16, seed=3):
    """radii of the REAL queries: query 0 is complete (3 rows or the ties of the third), query 1 has more rows than cap (RANGE_TOPK), the others sit
    midway behind their 5th row.  The decoy: other queries under the same radii - and, for a host radius, radii under the same queries that
    admit no row at all."""
    X = table(tab)
    Qr, Qd = queries(tab, nq, seed), queries(tab, nq, seed + 1000)
    d = np.sort(int_dists(X, Qr), axis=0)
    radius = np.array([0.5 * (d[4, q] + d[5, q]) for q in range(nq)], F)
    radius[0] = F(d[2, 0])
    radius[1] = F(d[4 * cap, 1])
    decoy_radius = (d[0] - 1).astype(F)      # (under the same queries only a radius that admits NO row changes the first id: every answer is empty)
    want = topk_np(X, Qr, cap, radius=radius)
    assert want[3][0] <= cap < want[3][1], "range case: query 0 must be complete and query 1 beyond the cap: totals %s" % want[3]
    return dict(name="search_range %s nq %d cap %d" % (tab, nq, cap), tab=tab, cap=cap, real=(Qr, radius), decoy=(Qd, decoy_radius), want=want,
                want_decoy=topk_np(X, Qd, cap, radius=radius), want_decoy_radius=topk_np(X, Qr, cap, radius=decoy_radius),
                names=("ids", "dist", "counts", "totals"))


def among_case(tab, nq, k, shared, seed=5, longest=400):
    """one list for every query, or one per query (lengths 0 .. longest, the same offsets for the real lists and the decoys).  Decoys: other
    queries under the real lists, and other lists (other rows) under the real queries."""
    X = table(tab)
    n = len(X)
    rng = np.random.default_rng(seed)
    Qr, Qd = queries(tab, nq, seed), queries(tab, nq, seed + 1000)
    if shared:
        lens, off = np.array([longest]), None
    else:
        lens = rng.integers(k + 1, longest + 1, nq)
        lens[0] = longest
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # the decoy lists name rows that NO real list names: whatever a call takes from them, and however it is split, no first id is the real one
    perm = rng.permutation(n)
    pool_r, pool_d = perm[:n // 2], perm[n // 2:]
    Lr, Ld = (np.concatenate([rng.choice(pool, size=m, replace=False) for m in lens]).astype(np.int64) for pool in (pool_r, pool_d))
    split = lambda L: L if shared else [L[off[q]:off[q + 1]] for q in range(nq)]      # noqa: E731
    mr_, md_ = rows_mask(n, split(Lr), nq), rows_mask(n, split(Ld), nq)
    fr = first_ids(X, Qr, mr_)
    for again in range(1, 9):      # (a list of a few hundred rows: a decoy query may share its first id with the real one - drawn again)
        eq = np.flatnonzero(fr == first_ids(X, Qd, mr_))
        if len(eq) == 0:
            break
        Qd[eq] = queries(tab, nq, seed + 1000 + again)[eq]
    return dict(name="search_among %s nq %d k %d %s" % (tab, nq, k, "one list" if shared else "a list per query"), tab=tab, k=k, offsets=off,
                real=(Qr, Lr), decoy=(Qd, Ld), want=topk_np(X, Qr, k, mr_)[:3], want_decoy=topk_np(X, Qd, k, mr_)[:3],
                want_decoy_list=topk_np(X, Qr, k, md_)[:3], want_both_decoys=topk_np(X, Qd, k, md_)[:3], names=("ids", "dist", "counts"))


SELECT_PROG = [("i32", 0), ("const", 5), (">",)]


def select_case(tab="A", skip=3, limit=50, seed=7):
    """select under the program `attribute > 5`: the attribute rows are the input that changes"""
    n = SHAPES[tab][0]
    rng = np.random.default_rng(seed)
    rows_r, rows_d = (rng.integers(0, 10, n).astype(np.int32) for _ in range(2))

    def answer(rows):
        vis = np.flatnonzero(rows > 5)
        ids = np.full(limit, FILL, np.int64)
        w = vis[skip:skip + limit]
        ids[:len(w)] = w
        return ids, np.array([len(w), len(vis)], np.int64)
    return dict(name="select %s skip %d limit %d" % (tab, skip, limit), tab=tab, skip=skip, limit=limit, real=(rows_r,), decoy=(rows_d,),
                want=answer(rows_r), want_decoy=answer(rows_d), names=("ids", "counts"))


def filter_case(tab, nq, k, kind, seed=9):
    """(c): a borrowed bitset ('deleted') or int column ('column', visible iff value == 0).  State 1 hides a few random rows; state 2 hides,
    besides, every query's first id under state 1.  real = (state 1, state 2): the first search must answer for state 1, the second for state 2."""
    X = table(tab)
    n = len(X)
    rng = np.random.default_rng(seed)
    Q = queries(tab, nq, seed)
    hid1 = np.zeros(n, bool)
    hid1[rng.choice(n, size=50, replace=False)] = True
    w1 = topk_np(X, Q, k, ~hid1)[:3]
    hid2 = hid1.copy()
    hid2[w1[0][:, 0]] = True
    w2 = topk_np(X, Q, k, ~hid2)[:3]
    pack = (lambda h: np.packbits(h, bitorder="little")) if kind == "deleted" else (lambda h: h.astype(np.int32))
    return dict(name="filter %s %s nq %d k %d" % (kind, tab, nq, k), tab=tab, k=k, kind=kind, Q=Q, real=(pack(hid1), pack(hid2)), decoy=(pack(hid2), pack(hid1)),
                want=w1, want_decoy=w2, names=("ids", "dist", "counts"))


def merge_case(kind, G=3, nq=5, k=16, seed=11):
    """(e): G sorted lists per query, full, with unique 40-bit ids; the decoy is another draw"""
    import merge_ref as mg

    def draw(rng):
        if kind == "select":
            ids = np.sort(rng.choice(1 << 20, size=(G, k), replace=False).astype(np.int64), axis=1)
            cnt = np.full(G, k, np.int64)
            return ids, cnt, cnt + 5
        dist = np.sort(rng.integers(0, 1000, (G, nq, k)).astype(F), axis=2)
        ids = rng.choice(1 << 40, size=G * nq * k, replace=False).astype(np.int64).reshape(G, nq, k)
        for s in range(G):      # (equal distances inside a list: ids ascending)
            for j in range(nq):
                o = np.lexsort((ids[s, j], dist[s, j]))
                ids[s, j], dist[s, j] = ids[s, j][o], dist[s, j][o]
        if kind == "range":
            return ids, dist, np.full((G, nq), k, np.int32), np.full((G, nq), k + 2, np.int64)
        return dist, ids

    def answer(a):
        if kind == "select":
            w, total = mg.merge_select(a[0], a[1], a[2], 2, k - 2)      # (a shard's list must reach as far as the window: skip + limit = len)
            return w, np.array([len(w), total], np.int64)
        if kind == "range":
            return mg.merge_range(*a)
        i, d, _, _ = mg.merge_range(a[1], a[0], np.full((G, nq), k, np.int32), np.zeros((G, nq), np.int64))
        return d, i
    real, decoy = draw(np.random.default_rng(seed)), draw(np.random.default_rng(seed + 1000))
    names = {"select": ("ids", "counts"), "range": ("ids", "dist", "counts", "totals")}.get(kind, ("dist", "ids"))
    return dict(name="merge %s G %d nq %d k %d" % (kind, G, nq, k), kind=kind, G=G, nq=nq, k=k, real=real, decoy=decoy, want=answer(real), want_decoy=answer(decoy),
                names=names)


def normalize_case(n=5, d=16, seed=13):
    rng = np.random.default_rng(seed)
    real, decoy = (rng.integers(-8, 9, (n, d)).astype(F) for _ in range(2))
    real[2] = 0      # (a zero row stays zero with only_if_nonzero)

    def answer(a):
        nrm = np.sqrt((a.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
        return (np.where(nrm > 0, a / np.where(nrm > 0, nrm, 1), a).astype(F),)
    return dict(name="normalize_rows %d x %d" % (n, d), real=(real,), decoy=(decoy,), want=answer(real), want_decoy=answer(decoy), names=("rows",))


def first_of(case, answer):
    """the column the vacuity condition reads: the ids' first place per query (a select / a merged select: its first id; normalize: the rows' first value)"""
    a = np.asarray(answer[case["names"].index("ids")] if "ids" in case["names"] else answer[0])
    return a.reshape(len(a), -1)[:, 0] if a.ndim > 1 else a[:1]


def check_case(case):
    """before anything is launched: every decoy answer differs from the real one in every query's first id"""
    for key in case:
        if key.startswith("want_"):
            differ_first(first_of(case, case["want"]), first_of(case, case[key]), "%s (%s)" % (case["name"], key))
    return case
