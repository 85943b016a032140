"""What the graph search under eps_search_params::filter_in_traversal = 1 is held to on tables of ties (tests/walk_ref.py): its documented
rule (include/epsilla_gfx950.h, csrc/traverse.hip graph_search_impl), restated in numpy from the ORACLE's evaluation log alone - for
tests/test_filtered_walk_cpu.py (the conditions on the inputs, planted faults on this model) and tests/test_gpu_traverse_filtered_ties.py (fed
with what GpuIndex.search(..., filter_in_traversal=1) returns).  Nothing here is fitted to device output.

The rule.  The walk is the reference's (invisible rows keep their place in the queues).  The answer of a query is
  * among all rows the walk EVALUATED - the SearchQueueSize seeds and every neighbour a distance was computed for, including those the
    `dist > bound` test dropped from the queues when they were evaluated - the VISIBLE ones (not deleted, passing the int-column test and the
    filter program), in stable (distance, id) order;
  * merged by (distance, id) with the visible rows of the un-indexed tail (exact scan; at most min(limit, 8192) of them take part, tail_plan);
  * cut at Kf = min(n_indexed, limit, LocalQueueSize).  Kf does NOT include SearchQueueSize L - unlike the unfiltered path's cap
    min(n_indexed, limit, LocalQueueSize, L): with limit > L a filtered search may return more than L rows;
  * the count is the number of entries that remain, the rest of a result row is -1 / +inf.
On a tie table fp32 computes every distance exactly in any order, and the device's evaluation count is pinned to the oracle's
(tests/test_gpu_traverse_ties.py), so the evaluated SET is the oracle's and the answer can be asked for id by id, value by value.

preconditions() states what a case's inputs have to deliver, from the oracle and fp64 alone, BEFORE a device is asked.  A case that misses
one gets another table or filter, never a weaker condition."""
import numpy as np

import exact_ref as xr
import select_ref as sr
import walk_ref as wr

F = np.float32
TAIL_CAP = 8192          # tail_plan (csrc/graph_host.hpp): keys of a query's tail list = min(limit, 8192)
LOG_FLOOR = 16384        # trv_launch: slots of a query's evaluation log on the first attempt = min(n, max(16384, 64 L))
MAX_K = 1024             # the filtered merge's widest class: 16 keys per lane
VARIANTS = ["queue_only", "no_beyond", "no_seeds", "cap_L", "log_order", "tail_unfiltered", "no_tail", "cut_before_tail"]


def first_log(n, L):
    """slots of the first attempt's evaluation log (checked against the header by tests/native/graph_host_check.cpp `ecap`)"""
    return min(n, max(LOG_FLOOR, 64 * L))


def repeat_log(n, longest):
    """slots of the second attempt's log after a first one whose longest walk evaluated `longest` rows (graph_search_impl)"""
    return min(n, longest + longest // 4 + 1024)


# ------------------------------------------------------------------------------------------------ the cases (one list for both test files)
A_PARAMS = [(1, 100, 4), (2, 500, 15), (4, 500, 3), (8, 300, 15), (17, 500, 15), (32, 500, 15)]
K_CLASSES = [1, 64, 65, 128, 129, 512, 1024]
SELECTIVE_COL = (4, ">=", 94)        # column values are 0..99: 6 % pass, 4 % with every 3rd row deleted as well
A_COL = {10: (4, ">=", 99), 100: (4, ">=", 94)}   # k = 10 needs fewer than 10 visible rows in a queue of 500 of the 2000: 1 % pass, 0.7 % with the deletions
A_FSEED = {10: 1, 100: 0}                         # (the column draw under which every k = 10 case meets conditions 5 to 9: chosen on the CPU, from the oracle)
REPEAT = dict(n=40000, d=16, nq=12, degree=96, T=4, L=180, I=15, k=50)
REPEAT_FIRST_LOG, REPEAT_SECOND_LOG = 16384, 22895   # slots of the two attempts' logs at REPEAT (tests/native/graph_host_check.cpp repeat_log() pins both)
E_TILED = 264          # queries of a group e call: beyond 256 the plan sends queues from 80 KB of LDS on to HBM (trv_launch)
H_TILED = 1100         # queries of the tiled step of group h: more than the 4 x 256 workgroups of a launch, so that workgroups walk a second query
assert set(A_PARAMS) <= set(wr.QUEUE_PARAMS) and {t for t, _, _ in A_PARAMS} == {1, 2, 4, 8, 17, 32}


def _fcase(name, fgroup, walk, selective=False, every=None, col=None, program=False, n_tail=0, visited=("bitmap",), mode="graph", **more):
    c = dict(walk)
    c.update(name=name, fgroup=fgroup, selective=selective, every=every, col=col, program=program, n_tail=n_tail, visited=tuple(visited), mode=mode)
    c.update(more)
    return c


def _w(metric, T, L, k, I=15, n=2000, d=16, nq=24, **kw):
    return wr._case("filtered", n, d, nq, metric, T, L, k, I=I, **kw)


def cases_a():
    """workers and queues, selective: every 3rd row deleted and a column test that leaves a few per cent visible"""
    return [_fcase("a-%s-T%d-L%d-I%d-k%d" % (wr.METRIC_NAMES[m], T, L, I, k), "a", _w(m, T, L, k, I=I), selective=True, every=3, col=A_COL[k], fseed=A_FSEED[k], v=1,
                   visited=("bitmap", "stamps")) for m in (0, 1, 2) for T, L, I in A_PARAMS for k in (10, 100)]


def cases_b():
    """filter kinds on one (T = 4, L = 500) walk per metric"""
    kinds = [("deleted", dict(every=3)), ("col-w1", dict(col=(1, ">=", 70))), ("col-w2", dict(col=(2, "<", 30))), ("col-w4", dict(col=(4, "!=", 7))),
             ("col-w8", dict(col=(8, "<=", 49))), ("program", dict(program=True)), ("program-deleted", dict(program=True, every=3)),
             ("none-visible", dict(col=(4, ">=", 1000))), ("all-visible", dict(col=(4, ">=", 0)))]
    return [_fcase("b-" + nm, "b", _w(i % 3, 4, 500, 50), **kw) for i, (nm, kw) in enumerate(kinds)]


def cases_c():
    """k and the caps: the merge's keys-per-lane classes (both queue sizes raised to k where k is beyond 500, or Kf would cut there), k beyond
    the visible evaluated rows, LocalQueueSize < k, k > L.  k > L needs LocalQueueSize > SearchQueueSize, where the reference defines no
    walk (its AddIntoQueue runs the L-slot master queue with capacity LocalQueueSize and writes past its end); the device's master queue
    holds L keys whatever LocalQueueSize (csrc/traverse2_kernel.hpp, `cap = w == T - 1 ? L : Lq`), which at T = 1 - no worker queues - is
    the walk with LocalQueueSize = L: walk_lq()."""
    out = [_fcase("c-k%d" % k, "c", _w(i % 3, 4, max(500, k), k, n=3000), every=7) for i, k in enumerate(K_CLASSES)]
    out.append(_fcase("c-short", "c", _w(0, 4, 500, 100), every=3, col=SELECTIVE_COL))
    out.append(_fcase("c-Lq60", "c", _w(0, 4, 400, 100, Lq=60, shape="holes"), every=3))
    out.append(_fcase("c-k-beyond-L", "c", _w(2, 1, 64, 128, I=4, Lq=500), every=3))
    return out


def cases_d():
    """adjacency shapes: the CSR form, duplicate entries, isolated nodes"""
    return [_fcase("d-%s-T%d" % (shape, T), "d", _w(m, T, 500, 100, I=I, shape=shape), every=3, col=(2, "<", 40))
            for shape in ("long", "holes") for m, (T, I) in enumerate([(1, 1), (4, 15)])]


def cases_e():
    """queues in HBM, on the graph the device builds (the CPU file stands a random CSR in for it).  The plan (csrc/graph_host.hpp trv_launch)
    keeps the queues of a call of up to 256 queries in LDS while a workgroup needs at most 150 KB - which (4, 2500) and (1, 12000) do, at
    92 to 97 KB and 134 KB - and sends them to HBM from 80 KB on in a larger call: the 6 queries are tiled to E_TILED = 264, every one
    checked, and the GPU test reads the plan's own word (HBM | LDS) from the library's profile line; tests/native/graph_host_check.cpp pins
    both sides of that threshold.  At L = 12000 = n every row is a seed: the log IS the table and the final queue is the table in order, so
    conditions 7 to 9 cannot hold for any table or filter (nothing is evaluated beyond the queue, the reference's post-filter sees every
    visible row): that walk runs under the same selective filter but is no selective CASE.  In its place (1, 9000) is: at T = 1 the queue
    leaves LDS from L = 8193 on (16384 keys), and with 0.7 % of the rows visible the 9000 of the final queue hold fewer than k = 100."""
    return [_fcase("e-T%d-L%d" % (T, L), "e", wr._case("filtered", 12000, 24, 6, 0, T, L, 100, graph="device"), selective=L < 12000, every=3,
                   col=(4, ">=", v), tiled=E_TILED, check_every=1) for T, L, v in [(4, 2500, 97), (1, 12000, 97), (1, 9000, 99)]]


def cases_f():
    """the tail, selective: the SEARCH_CASE shape (3000 indexed + 500 appended rows, every 4th deleted) with a column test that lets 8 % through;
    and once more with LocalQueueSize 60 < limit: the cut comes after the tail merge"""
    s = wr.SEARCH_CASE
    w = lambda T, Lq: wr._case("filtered", s["n"], s["d"], s["nq"], s["metric"], T, s["L"], s["limit"], Lq=Lq, I=s["I"], K=s["K"], graph="search")
    out = [_fcase("f-tail-T%d" % T, "f", w(T, s["Lq"]), selective=True, every=s["every"], col=(4, ">=", 920), n_tail=s["n_tail"], mode="reference") for T in (1, 4)]
    out.append(_fcase("f-tail-T4-Lq60", "f", w(4, 60), every=s["every"], col=(4, ">=", 920), n_tail=s["n_tail"], mode="reference"))
    return out


def cases_g():
    """the log's repeat: a random CSR of out-degree 96 over a 40000 x 16 tie table; L chosen on the CPU so that some walks evaluate more than
    the first attempt's 16384 log slots and some fewer (asserted by the CPU file and pinned in tests/native/graph_host_check.cpp)"""
    r = REPEAT
    return [_fcase("g-repeat", "g", wr._case("filtered", r["n"], r["d"], r["nq"], 0, r["T"], r["L"], r["k"], I=r["I"], graph="random"), every=3, col=(4, ">=", 90),
                   degree=r["degree"])]


def cases_h():
    """state between calls: the filters and k values one index is asked for in turn (the b walk under L2).  The last one tiles the 24 queries
    to H_TILED = 1100: a launch has at most 4 workgroups per CU, 1024 on 256 CUs (tests/native/graph_host_check.cpp pins it; 300 queries
    would get a workgroup each), so 76 workgroups walk a second query on the visited set, the stamps and the log count their first one
    left.  Every query is checked; the GPU test reads the launch's workgroup count from the library's profile line."""
    w = lambda k: _w(0, 4, 500, k)
    return [_fcase("h-deleted", "h", w(50), every=3), _fcase("h-program", "h", w(50), program=True), _fcase("h-k128", "h", w(128), program=True),
            _fcase("h-k10", "h", w(10), program=True), _fcase("h-tiled", "h", w(50), every=3, col=(4, ">=", 80), tiled=H_TILED, check_every=1)]


def cases_i():
    """the prefilter forced on a filtered call"""
    return [_fcase("i-prefilter", "i", _w(0, 4, 500, 50), every=3, col=(4, ">=", 80))]


def all_cases():
    return cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f() + cases_g() + cases_h() + cases_i()


def case_id(c):
    return c["name"]


def by_name(name):
    return [c for c in all_cases() if c["name"] == name][0]


# ------------------------------------------------------------------------------------------------ inputs
def random_csr(n, degree, seed=0):
    """`degree` random out-edges per node, the last one the next row (every node is reachable)"""
    rng = np.random.default_rng([seed, n, degree, 9])
    nb = np.concatenate([rng.integers(0, n, (n, degree - 1)), ((np.arange(n) + 1) % n)[:, None]], axis=1).astype(np.int64)
    return np.arange(n + 1, dtype=np.int64) * degree, nb.reshape(-1), 0


def inputs(c, oracle, graph=None):
    """(X [n + n_tail], Q, off, nbr, nav): the graph covers the first n rows.  graph: the arrays to use where the case's own come from the device"""
    if c["graph"] == "search":
        s = wr.SEARCH_CASE
        assert (c["n"], c["n_tail"], c["d"], c["nq"], c["metric"]) == (s["n"], s["n_tail"], s["d"], s["nq"], s["metric"])
        X, Q, off, nbr, nav, _, _ = wr.search_inputs(oracle)
        return X, Q, off, nbr, nav
    assert c["n_tail"] == 0
    if c["graph"] == "random":
        X, Q = wr.tie_table(c["n"], c["d"], c["nq"], c["metric"], c["seed"])
        return (X, Q) + random_csr(c["n"], c["degree"], c["seed"])
    X, Q = wr.tie_table(c["n"], c["d"], c["nq"], c["metric"], c["seed"], v=c.get("v"))
    if graph is None:
        graph = wr.oracle_graph(oracle, c["n"], c["d"], c["nq"], c["seed"], v=c.get("v"), cols=c["cols"], K=c["K"])
    return (X, Q) + tuple(wr.reshape_adjacency(graph[0], graph[1], graph[2], c["shape"], c["seed"]))


_PROG_FIELDS = [("a", "i32"), ("x", "f32")]
_COL_TYPES = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def filters(c, oracle=None):
    """dict(deleted bitset | None, col (values, op, value) | None, program | None, rows | None, vis bool [n + n_tail]) of a case; the visible
    set is select_ref.visible_rows' - the deleted bit, the int-column test, the program on a stack of doubles"""
    nt = c["n"] + c["n_tail"]
    rng = np.random.default_rng([c["seed"], nt, 55, c.get("fseed", 0)])
    out = dict(deleted=None, col=None, program=None, rows=None)
    if c["graph"] == "search":          # the search case's own deleted set and column (values 0..999)
        _, _, _, _, _, dele, colv = wr.search_inputs(oracle)
        width, op, value = c["col"]
        assert width == colv.dtype.itemsize
        out.update(deleted=dele, col=(colv, op, value))
    else:
        if c["every"]:
            dele = np.zeros((nt + 7) // 8, np.uint8)
            idx = np.arange(0, nt, c["every"])
            np.bitwise_or.at(dele, idx >> 3, (1 << (idx & 7)).astype(np.uint8))
            out["deleted"] = dele
        if c["col"]:
            width, op, value = c["col"]
            out["col"] = (rng.integers(0, 100, nt).astype(_COL_TYPES[width]), op, value)
    if c["program"]:
        dt, offs = sr.row_layout(_PROG_FIELDS)
        rows = np.zeros(nt, dt)
        rows["a"] = rng.integers(0, 100, nt)
        rows["x"] = rng.integers(0, 8, nt) / F(8)
        out["rows"] = rows
        out["program"] = [("i32", offs["a"]), ("const", 60), (">=",), ("f32", offs["x"]), ("const", 0.5), ("<",), ("and",)]   # a >= 60 AND x < 0.5
    out["vis"] = sr.visible_rows(nt, deleted=out["deleted"], int_filter=out["col"], program=out["program"], rows=out["rows"])
    return out


_LOGS = {}


def walk_lq(c):
    """LocalQueueSize as the oracle's walk gets it (cases_c: beyond SearchQueueSize only at T = 1, where it is L)"""
    L, Lq, _ = wr.effective(c)
    if Lq > L:
        assert c["T"] == 1, "LocalQueueSize > SearchQueueSize with worker queues: the reference defines no walk"
        return L
    return Lq


def logged_walks(oracle, c, graph=None, tag=None):
    """per query (queue ids [L], queue distances [L], evaluations, log ids, log distances, log `beyond` flags) of oracle.search_impl under the
    lockstep schedule; once per WALK, whatever filter and k the cases put on it"""
    key = (c["n"], c["n_tail"], c["d"], c["nq"], c["seed"], c["metric"], c["T"], c["L"], c["Lq"], c["I"], c["shape"], c["cols"], c["K"], c["graph"], c.get("degree"), c.get("v"), tag)
    if key not in _LOGS:
        X, Q, off, nbr, nav = inputs(c, oracle, graph)
        L, Lq = wr.effective(c)[0], walk_lq(c)
        init = oracle.prepare_init_ids(off, nbr, nav, L)
        Xg = np.ascontiguousarray(X[:c["n"]])
        _LOGS[key] = (init, [oracle.search_impl(c["metric"], Xg, off, nbr, init, q, T=c["T"], L=L, Lq=Lq, I=c["I"], lockstep=True, log=True) for q in Q])
    return _LOGS[key]


def reference_counts(oracle, c, flt, graph=None):
    """rows per query under the REFERENCE's semantics (oracle.search: post-filter over the final queue) with the case's deleted set and column test"""
    from oracle.pyoracle import make_filter
    assert not c["program"], "the oracle's filter has no program"
    X, Q, off, nbr, nav = inputs(c, oracle, graph)
    L, Lq = wr.effective(c)[0], walk_lq(c)
    kw = {}
    if flt["col"]:
        kw = dict(attr=flt["col"][0], op=flt["col"][1], value=flt["col"][2], width=flt["col"][0].dtype.itemsize)
    f, keep = make_filter(deleted=flt["deleted"], **kw)
    return [len(oracle.search(c["metric"], X, c["n"], off, nbr, nav, q, c["k"], T=c["T"], L=L, Lq=Lq, I=c["I"], flt=f, n_total=len(X), lockstep=True)[0]) for q in Q]


# ------------------------------------------------------------------------------------------------ the rule
def kf(c):
    """Kf = min(n_indexed, limit, LocalQueueSize): no L"""
    return min(c["n"], c["k"], c["Lq"])


def _exact32(X, ids, q, metric):
    d64 = xr.dist64(X[ids], q[None, :], metric)[:, 0] if len(ids) else np.zeros(0, np.float64)
    d32 = d64.astype(F)
    assert (d32.astype(np.float64) == d64).all(), "a distance of the tail is no fp32 value - not a table fp32 computes exactly"
    return d32


def candidates(c, walk, vis, X, q, variant=None):
    """the visible rows a query's answer is cut from, merged and ordered: (ids, distances), uncut.  variant: a planted fault (VARIANTS)"""
    qid, qd, ev, lid, ld, lb = walk
    n, nt, k = c["n"], c["n"] + c["n_tail"], c["k"]
    L = wr.effective(c)[0]
    cid, cd = lid, ld
    if variant == "queue_only":
        cid, cd = np.asarray(qid), np.asarray(qd)
    elif variant == "no_beyond":
        cid, cd = lid[lb == 0], ld[lb == 0]
    elif variant == "no_seeds":
        cid, cd = lid[L:], ld[L:]
    m = vis[cid]
    cid, cd = cid[m], cd[m]
    o = np.argsort(cd, kind="stable") if variant == "log_order" else np.lexsort((cid, cd))
    cid, cd = cid[o], cd[o]
    if variant == "cut_before_tail":
        cid, cd = cid[:kf(c)], cd[:kf(c)]
    if nt > n and variant != "no_tail":
        tid = np.arange(n, nt, dtype=np.int64)
        if variant != "tail_unfiltered":
            tid = tid[vis[n:nt]]
        td = _exact32(X, tid, q, c["metric"])
        o = np.lexsort((tid, td))[:min(k, TAIL_CAP)]
        cid, cd = np.concatenate([cid, tid[o]]), np.concatenate([cd, td[o]])
        o = np.argsort(cd, kind="stable") if variant == "log_order" else np.lexsort((cid, cd))
        cid, cd = cid[o], cd[o]
    return cid.astype(np.int64), cd.astype(F)


def rule(c, walk, vis, X, q, variant=None):
    """(ids, distances) of ONE query's answer; its count is their length"""
    cid, cd = candidates(c, walk, vis, X, q, variant)
    cut = kf(c)
    if variant == "cut_before_tail":
        cut = c["k"]          # (the k slots of the result row, never cut again)
    if variant == "cap_L":
        cut = min(cut, wr.effective(c)[0])
    return cid[:cut], cd[:cut]


def expected(c, walks, vis, X, Q, variant=None):
    return [rule(c, w, vis, X, q, variant) for w, q in zip(walks, Q)]


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def preconditions(c, init, walks, vis, X, Q, ref_counts=None):
    """The nine conditions of a filtered case (module docstring of tests/test_filtered_walk_cpu.py lists them); asserts each one that applies
    and returns {number: True | "n/a"} - "n/a" where the case has nothing the condition speaks about (5: no answer holds two rows; 6: no
    query has more than Kf visible candidates; 7 to 9: asked of selective cases only).  ref_counts: reference_counts() for a selective case."""
    what = c["name"]
    L = wr.effective(c)[0]
    K = kf(c)
    met = {}
    for qi, (qid, qd, ev, lid, ld, lb) in enumerate(walks):
        assert len(lid) == ev, "%s query %d: %d log entries, %d evaluations" % (what, qi, len(lid), ev)                                  # 1
        assert len(np.unique(lid)) == len(lid), "%s query %d: a row is logged twice" % (what, qi)                                        # 2
        assert np.array_equal(lid[:L], init), "%s query %d: the log does not start with the %d seeds" % (what, qi, L)                    # 3
        assert not lb[:L].any(), "%s query %d: a seed is flagged as dropped by the bound" % (what, qi)
        d64 = xr.dist64(X[lid], Q[qi][None, :], c["metric"])[:, 0]
        bad = np.flatnonzero(ld.astype(np.float64) != d64)
        assert len(bad) == 0, "%s query %d: logged distance %r of row %d is not its fp64 distance %r" % (what, qi, ld[bad[0]], lid[bad[0]], d64[bad[0]])   # 4
    met[1] = met[2] = met[3] = met[4] = True
    exp = expected(c, walks, vis, X, Q)
    if sum(max(len(d) - 1, 0) for _, d in exp) > 0:
        share = wr.tie_share([d for _, d in exp])
        assert share >= wr.TIE_FLOOR, "%s: only %.3f of the adjacent positions of the expected answers are ties (floor %.2f) - change the TABLE or the filter" % (what, share, wr.TIE_FLOOR)
        met[5] = True
    else:
        share = 0.0
        met[5] = "n/a"
    longer = boundary = 0
    for w, q in zip(walks, Q):
        cid, cd = candidates(c, w, vis, X, q)
        if len(cid) > K:
            longer += 1
            boundary += int(cd[K - 1] == cd[K])
    if longer:
        assert boundary >= 1, "%s: no query has equal distances at ranks %d and %d of its visible candidates - change the TABLE or the filter" % (what, K, K + 1)
        met[6] = True
    else:
        met[6] = "n/a"
    met[7] = met[8] = met[9] = "n/a"
    if c["selective"]:
        outside = flagged = 0
        for (eid, ed), (qid, qd, ev, lid, ld, lb) in zip(exp, walks):
            gid = eid[eid < c["n"]]          # the INDEXED rows of the answer: a row of the tail is in no queue and no log
            outside += int(len(np.setdiff1d(gid, qid)) > 0)
            flagged += int(len(np.intersect1d(gid, lid[lb != 0])) > 0)
        assert outside >= 1, "%s: no expected answer holds an indexed row outside the oracle's final queue" % what                               # 7
        assert flagged >= 1, "%s: no expected answer holds an indexed row the bound dropped when it was evaluated" % what                        # 8
        assert ref_counts is not None and min(ref_counts) < c["k"], "%s: the reference's semantics returns k rows for every query" % what   # 9
        met[7] = met[8] = met[9] = True
    return met, share, exp


def border_ties(exp, n_indexed):
    return wr.border_ties(exp, n_indexed)


# ------------------------------------------------------------------------------------------------ the comparator
def assert_same_filtered(ids, dist, cnt, exp_ids, exp_dist, what=""):
    """ONE query.  ids / dist: the returned row of the result arrays (k entries), cnt: its count; the expected answer.  The count is the
    expected one, the ids are the expected ones position by position, the distances are the expected ones as VALUES (==: -0 and +0 are one
    distance; a NaN equals nothing), the rest of the row is -1 / +inf.  No tolerance, no set difference."""
    ids, dist = np.asarray(ids), np.asarray(dist)
    eid, ed = np.asarray(exp_ids, np.int64), np.asarray(exp_dist)
    m = len(eid)
    assert len(ids) >= m and len(dist) >= m, "%s: %d ids, %d distances for %d expected results" % (what, len(ids), len(dist), m)
    got_i, got_d = ids[:m].astype(np.int64), np.asarray(dist[:m], np.float64)
    bad = np.flatnonzero((got_i != eid) | ~(got_d == np.asarray(ed, np.float64)))
    if len(bad):
        r = int(bad[0])
        lo, hi = wr._group(ed, r)
        raise AssertionError(
            "%s: first difference at rank %d of %d (%d places differ; count %d, expected %d): returned (id %d, %r), expected (id %d, %r)\n"
            "  tie group of the expected answer around it, ranks [%d, %d) at distance %r: ids %s\n  returned there: ids %s, distances %s" % (
                what, r, m, len(bad), int(cnt), m, got_i[r], dist[r], eid[r], ed[r], lo, hi, ed[r], eid[lo:hi].tolist(), ids[lo:min(hi, len(ids))].tolist(),
                dist[lo:min(hi, len(dist))].tolist()))
    assert int(cnt) == m, "%s: %d results, %d expected" % (what, int(cnt), m)
    assert (ids[m:] == -1).all(), "%s: ids beyond the count are not -1" % what
    assert np.isposinf(np.asarray(dist[m:], np.float64)).all(), "%s: distances beyond the count are not +inf" % what
    assert len(np.unique(got_i)) == m, "%s: a row appears twice" % what
