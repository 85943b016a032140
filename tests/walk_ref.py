"""What the graph WALK (csrc/traverse2_kernel.hpp) is held to on tables of ties: the oracle's SearchImpl under the lockstep schedule, with no
tolerance at all - for tests/test_walk_ties_cpu.py (the conditions on the inputs, planted faults, the oracle against the compiled reference)
and tests/test_gpu_traverse_ties.py (fed with what GpuIndex.search returns).  numpy plus the oracle front-end; nothing here is fitted to
device output.

Tie tables: rows and queries are integers in [-v, v] (divided by 16 under COSINE, as "integers / 16" of exact_ref.py).  Every product and
every partial sum of a distance is then an integer (a multiple of 1/256) far below 2^24: fp32 computes the distance exactly in ANY summation
order, lane split or piece count, so the walk is a pure function of its inputs and the reference's (distance, id) order is total.  The
device must return the oracle's ids, distance values and evaluation count exactly; on such tables a large share of all comparisons the walk
makes are ties (`dist == bound` at the `dist > bound` test, equal keys ordered by id, the duplicate test inside a run of equal distances,
the last-slot overwrite of the queue merge, the 8-bit prefilter at equality).

preconditions() states what a table has to deliver for that to be true, from the oracle and fp64 alone, BEFORE a device is asked.  A case
that misses one gets another table (narrower values, more rows), never a lower floor."""
import numpy as np

import exact_ref as xr

F = np.float32
TIE_FLOOR = 0.25      # share of adjacent positions of the compared queue prefixes that hold equal distances, per case
METRIC_NAMES = {0: "L2", 1: "COSINE", 2: "DOT"}


# ------------------------------------------------------------------------------------------------ tables, graphs, adjacency shapes
_TABLES, _GRAPHS, _WALKS = {}, {}, {}


def default_v(d):
    return 1 if d >= 768 else 2


def int_table(n, d, nq, seed=0, v=None):
    """(rows, queries) as integers in [-v, v], float32; drawn once per (seed, n, d, nq, v)"""
    v = default_v(d) if v is None else v
    key = (n, d, nq, seed, v)
    if key not in _TABLES:
        rng = np.random.default_rng([seed, n, d])
        X = rng.integers(-v, v + 1, (n, d)).astype(F)
        Q = rng.integers(-v, v + 1, (nq, d)).astype(F)
        X.setflags(write=False)
        Q.setflags(write=False)
        _TABLES[key] = (X, Q)
    return _TABLES[key]


def tie_table(n, d, nq, metric, seed=0, v=None):
    """the integer table as the metric sees it: divided by 16 under COSINE (exact: a power of two)"""
    X, Q = int_table(n, d, nq, seed, v)
    if metric == 1:
        X, Q = X / F(16), Q / F(16)
    return X, Q


def oracle_graph(oracle, n, d, nq, seed=0, v=None, cols=None, K=60):
    """oracle.build_graph(0, ., K) over the integer table (its first `cols` columns for the wide tables: any CSR is a valid input of the
    walk, and the CPU build stays at seconds).  L2 over the table / 16 is L2 over the table / 256, exactly: one graph serves every metric."""
    key = (n, d, nq, seed, default_v(d) if v is None else v, cols, K)
    if key not in _GRAPHS:
        X, _ = int_table(n, d, nq, seed, v)
        off, nbr, nav = oracle.build_graph(0, np.ascontiguousarray(X[:, :cols]) if cols else X, K=K)
        _GRAPHS[key] = (np.asarray(off, np.int64), np.asarray(nbr, np.int64), int(nav))
    return _GRAPHS[key]


def reshape_adjacency(off, nbr, nav, shape, seed=0):
    """"plain": as built.  "long": six lists grow beyond 64 entries (the device's CSR form) by random ids, ten lists repeat their first
    entry.  "holes": the same, and five nodes (never the navigation node) lose their list altogether."""
    if shape == "plain":
        return off, nbr, nav
    assert shape in ("long", "holes"), shape
    n = len(off) - 1
    rng = np.random.default_rng([seed, n, 77])
    lists = [list(nbr[off[i]:off[i + 1]]) for i in range(n)]
    for v in rng.choice(n, size=6, replace=False):
        lists[int(v)] += [int(x) for x in rng.integers(0, n, size=int(rng.integers(70, 150)))]
    for v in rng.choice(n, size=10, replace=False):
        if lists[int(v)]:
            lists[int(v)].append(lists[int(v)][0])
    if shape == "holes":
        for v in [int(x) for x in rng.choice(n, size=6, replace=False) if int(x) != nav][:5]:
            lists[v] = []
    off2 = np.zeros(n + 1, np.int64)
    off2[1:] = np.cumsum([len(l) for l in lists])
    nbr2 = np.asarray([x for l in lists for x in l], np.int64)
    return off2, nbr2, nav


# ------------------------------------------------------------------------------------------------ the cases (one list for both test files)
QUEUE_PARAMS = [(1, 100, 4), (1, 500, 1), (2, 500, 15), (3, 64, 2), (4, 100, 15), (4, 500, 1), (4, 500, 3), (8, 300, 15), (16, 500, 15),
                (17, 500, 15), (32, 500, 15)]
WIDTHS = [19, 100, 128, 132, 256, 768, 772, 1030, 1536]
WIDTH_PARAMS = [(1, 100), (2, 200), (4, 300)]
LARGE_PARAMS = [(1, 3000), (4, 2500), (4, 6000), (1, 12000), (2, 12000)]


def _case(group, n, d, nq, metric, T, L, k, Lq=None, I=15, shape="plain", cols=None, K=60, graph="oracle", **more):
    c = dict(group=group, n=n, d=d, nq=nq, metric=metric, T=T, L=L, Lq=L if Lq is None else Lq, I=I, k=k, shape=shape, cols=cols, K=K,
             graph=graph, seed=0)
    c.update(more)
    return c


def width_metrics(d, i):
    """metrics rotate 0 / 1 / 2 over the widths; only two of the widths are no multiple of 4 (19, 1030: the scalar form of the distance
    phases), so those two run under all three metrics - every metric meets both forms"""
    return (0, 1, 2) if d % 4 else (i % 3,)


def queue_cases():
    """1: queue logic on heavy ties"""
    return [_case("queue", 2000, 16, 24, m, T, L, min(L, 500), I=I) for m in (0, 1, 2) for T, L, I in QUEUE_PARAMS]


def width_cases():
    """2: every width of the distance phases; d = 100 once more with 300 queries (the 32 tiled: the 4-wavefront form), every 10th checked"""
    out = []
    for i, d in enumerate(WIDTHS):
        for m in width_metrics(d, i):
            for T, L in WIDTH_PARAMS:
                out.append(_case("width", 3000, d, 32, m, T, L, min(L, 100), cols=16 if d >= 132 else None))
                if d == 100:
                    out.append(_case("width", 3000, d, 32, m, T, L, min(L, 100), tiled=300, check_every=10))
    return out


def large_cases():
    """3: queues beyond LDS, graph built by the device (the CPU file stands an oracle-built graph in for it)"""
    return [_case("large", 12000, 24, 6, 0, T, L, 1000, graph="device") for T, L in LARGE_PARAMS]


def shape_cases():
    """4: shapes of adjacency and queues"""
    out = []
    for shape in ("long", "holes"):
        for m, (T, L, I) in enumerate([(1, 500, 1), (4, 500, 15), (8, 300, 15)]):
            out.append(_case("shape", 2000, 16, 24, m, T, L, min(L, 500), I=I, shape=shape))
    out.append(_case("shape", 2000, 16, 24, 0, 4, 400, 100, Lq=60, shape="holes"))      # Lq < L, k beyond Lq: counts equal Lq
    out.append(_case("shape", 2000, 16, 24, 2, 1, 500, 100, Lq=30, shape="long"))
    for T, I in ((1, 15), (4, 1)):                                                           # L clamped to n: the whole table is the queue
        out.append(_case("shape", 600, 16, 24, 0, T, 5000, 600, I=I, shape="holes", K=30))
    return out


SEARCH_CASE = dict(group="search", n=3000, n_tail=500, d=32, nq=24, metric=0, L=500, Lq=500, I=15, limit=100, K=60, seed=0, every=4, op=">=", value=250)


def all_walk_cases():
    return queue_cases() + width_cases() + large_cases() + shape_cases()


def case_id(c):
    s = "%s-n%d-d%d-%s-T%d-L%d" % (c["group"], c["n"], c["d"], METRIC_NAMES[c["metric"]], c["T"], c["L"])
    if c["Lq"] != c["L"]:
        s += "-Lq%d" % c["Lq"]
    s += "-I%d" % c["I"]
    if c["shape"] != "plain":
        s += "-" + c["shape"]
    if c.get("tiled"):
        s += "-q%d" % c["tiled"]
    return s


def case_inputs(c, oracle, graph=None):
    """(X, Q, off, nbr, nav) of a walk case; graph: the arrays to use where the case's own come from the device"""
    X, Q = tie_table(c["n"], c["d"], c["nq"], c["metric"], c["seed"])
    if graph is None:
        graph = oracle_graph(oracle, c["n"], c["d"], c["nq"], c["seed"], cols=c["cols"], K=c["K"])
    off, nbr, nav = reshape_adjacency(graph[0], graph[1], graph[2], c["shape"], c["seed"])
    return X, Q, off, nbr, nav


def effective(c):
    """(L, Lq, compared entries per query) as the reference clamps them: SearchQueueSize to the graph, results to LocalQueueSize (:872)"""
    L = min(c["L"], c["n"])
    Lq = min(c["Lq"], c["n"])
    return L, Lq, min(c["k"], Lq, L)


def oracle_walks(oracle, c, graph=None, tag=None):
    """per query (ids [L], distances [L], evaluations) of oracle.search_impl under the lockstep schedule; computed once per walk, whatever
    engine switches the device runs it with.  tag: names a device-built graph in the cache key."""
    key = (c["n"], c["d"], c["nq"], c["seed"], c["metric"], c["T"], c["L"], c["Lq"], c["I"], c["shape"], c["cols"], c["K"], c["graph"], tag)
    if key not in _WALKS:
        X, Q, off, nbr, nav = case_inputs(c, oracle, graph)
        L, Lq, _ = effective(c)
        init = oracle.prepare_init_ids(off, nbr, nav, L)
        _WALKS[key] = [oracle.search_impl(c["metric"], X, off, nbr, init, q, T=c["T"], L=L, Lq=Lq, I=c["I"], lockstep=True) for q in Q]
    return _WALKS[key]


def search_inputs(oracle):
    """5: the whole Search path - (X [n + n_tail], Q, off, nbr, nav, deleted bitset, int column) with the graph over the first n rows"""
    c = SEARCH_CASE
    X, Q = tie_table(c["n"] + c["n_tail"], c["d"], c["nq"], c["metric"], c["seed"])
    key = ("search", c["n"], c["d"], c["K"])
    if key not in _GRAPHS:
        off, nbr, nav = oracle.build_graph(0, np.ascontiguousarray(X[:c["n"]]), K=c["K"])
        _GRAPHS[key] = (np.asarray(off, np.int64), np.asarray(nbr, np.int64), int(nav))
    off, nbr, nav = _GRAPHS[key]
    nt = c["n"] + c["n_tail"]
    dele = np.zeros((nt + 7) // 8, np.uint8)
    for i in range(0, nt, c["every"]):
        dele[i >> 3] |= 1 << (i & 7)
    col = np.random.default_rng([c["seed"], nt, 5]).integers(0, 1000, nt).astype(np.int32)
    return X, Q, off, nbr, nav, dele, col


def oracle_searches(oracle, T):
    """per query (ids, distances, evaluations) of oracle.search (graph walk, brute-force tail, merge, post-filter) under the lockstep schedule"""
    from oracle.pyoracle import make_filter
    key = ("search", T)
    if key not in _WALKS:
        c = SEARCH_CASE
        X, Q, off, nbr, nav, dele, col = search_inputs(oracle)
        flt, keep = make_filter(deleted=dele, attr=col, op=c["op"], value=c["value"])
        _WALKS[key] = [oracle.search(c["metric"], X, c["n"], off, nbr, nav, q, c["limit"], T=T, L=c["L"], Lq=c["Lq"], I=c["I"], flt=flt,
                                     n_total=len(X), lockstep=True) for q in Q]
    return _WALKS[key]


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def _dist64_of(X, q, ids, metric):
    return xr.dist64(X[np.asarray(ids, np.int64)], q[None, :], metric)[:, 0]


def tie_share(dists):
    """share of adjacent positions that hold equal distances, over a list of per-query distance arrays"""
    eq = sum(int((np.asarray(d)[1:] == np.asarray(d)[:-1]).sum()) for d in dists)
    tot = sum(max(len(d) - 1, 0) for d in dists)
    return eq / float(max(tot, 1))


def preconditions(case, oracle_results, X, Q, what=""):
    """From the oracle and fp64 alone:  1 every oracle distance equals the fp64 distance of the row it names, exactly;  2 at least TIE_FLOOR
    of the adjacent positions of the compared prefixes hold equal distances;  3 where a k-prefix of a longer queue is compared, at least one
    query has equal distances at ranks k and k + 1.  oracle_results: per query (ids, distances, ...), whole queues.  case: a walk case, or
    {"compared": n} for results compared as a whole.  Returns the tie share."""
    kc = case["compared"] if "compared" in case else effective(case)[2]
    metric = case["metric"]
    prefixes, boundary, longer = [], 0, False
    for qi, res in enumerate(oracle_results):
        oid, od = np.asarray(res[0]), np.asarray(res[1])
        assert not np.isnan(od).any(), "%s query %d: the oracle returns a NaN" % (what, qi)
        d64 = _dist64_of(X, Q[qi], oid, metric)
        bad = np.flatnonzero(od.astype(np.float64) != d64)
        assert len(bad) == 0, "%s query %d rank %d: oracle distance %r of row %d is not its fp64 distance %r - not a table fp32 computes exactly" % (
            what, qi, bad[0], od[bad[0]], oid[bad[0]], d64[bad[0]])
        m = min(kc, len(oid))
        prefixes.append(od[:m])
        if m < len(oid):
            longer = True
            boundary += int(od[m - 1] == od[m])
    share = tie_share(prefixes)
    assert share >= TIE_FLOOR, "%s: only %.3f of the adjacent positions are ties (floor %.2f) - change the TABLE, not the floor" % (what, share, TIE_FLOOR)
    if longer:
        assert boundary >= 1, "%s: no query has equal distances at ranks %d and %d - change the TABLE" % (what, kc, kc + 1)
    return share


def border_ties(oracle_results, n_indexed):
    """adjacent equal-distance pairs of the results with one row in the graph and one in the appended tail"""
    c = 0
    for res in oracle_results:
        oid, od = np.asarray(res[0]), np.asarray(res[1])
        c += int(((od[1:] == od[:-1]) & ((oid[1:] < n_indexed) != (oid[:-1] < n_indexed))).sum())
    return c


# ------------------------------------------------------------------------------------------------ the comparator
def _group(od, r):
    """[lo, hi) of the run of distances equal to od[r]"""
    lo, hi = r, r + 1
    while lo > 0 and od[lo - 1] == od[r]:
        lo -= 1
    while hi < len(od) and od[hi] == od[r]:
        hi += 1
    return lo, hi


def assert_same_walk(ids, dist, cnt, oracle_ids, oracle_dist, k, what=""):
    """ONE query.  ids / dist: the returned row of the result arrays (any length >= k), cnt: its count; the oracle's queue and the number k of
    entries that must come back.  The count is k, the ids are the oracle's position by position, the distances are the oracle's as VALUES (==:
    -0 and +0 are one distance, the kernel's key normalises d + 0.0f; a NaN equals nothing), the rest of the row is -1.  No tolerance, no set
    difference."""
    ids, dist = np.asarray(ids), np.asarray(dist)
    oid, od = np.asarray(oracle_ids)[:k], np.asarray(oracle_dist)[:k]
    assert len(oid) == k, "%s: the oracle holds %d entries, %d are to be compared" % (what, len(oid), k)
    assert int(cnt) == k, "%s: %d results, the oracle has %d" % (what, int(cnt), k)
    assert len(ids) >= k and len(dist) >= k, "%s: %d ids, %d distances for %d results" % (what, len(ids), len(dist), k)
    got_i, got_d = ids[:k].astype(np.int64), dist[:k]
    assert not np.isnan(np.asarray(got_d, np.float64)).any(), "%s: NaN distance at rank %d" % (what, int(np.flatnonzero(np.isnan(np.asarray(got_d, np.float64)))[0]))
    bad = np.flatnonzero((got_i != oid) | ~(np.asarray(got_d, np.float64) == np.asarray(od, np.float64)))
    if len(bad):
        r = int(bad[0])
        lo, hi = _group(np.asarray(oracle_dist), r)
        hi = min(hi, k + 1)
        raise AssertionError(
            "%s: first difference at rank %d of %d (%d places differ): returned (id %d, %r), oracle (id %d, %r)\n"
            "  tie group of the oracle around it, ranks [%d, %d) at distance %r: ids %s\n  returned there: ids %s, distances %s" % (
                what, r, k, len(bad), got_i[r], got_d[r], oid[r], od[r], lo, hi, od[r], np.asarray(oracle_ids)[lo:hi].tolist(),
                ids[lo:min(hi, len(ids))].tolist(), dist[lo:min(hi, len(dist))].tolist()))
    assert (ids[k:] == -1).all(), "%s: ids beyond the count are not -1" % what


def same_evals(device_total, oracle_total, what=""):
    assert int(device_total) == int(oracle_total), "%s: %d distance evaluations on the device, %d in the oracle" % (what, int(device_total), int(oracle_total))
