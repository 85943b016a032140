"""The STAGES of the graph build (csrc/graph_build.hip, csrc/traverse_kernel.hpp) against tests/build_ref.py on tables of ties: every node,
ids position by position, no tolerance.  Small integers, so fp32 computes every distance exactly in any summation order, (distance, id) is a
total order and a large share of all comparisons are ties - what tests/test_gpu_build.py, with its floors on continuous U[0,1) rows under
L2, cannot see: a kernel that is wrong on 1 node in 1000, or only at an equality.  The reference is proved equal to the oracle wherever the
oracle is defined, and is shown to catch the planted faults, by tests/test_build_ref_cpu.py.

  a  the kNN stage's exact path (n < 65 536) under the three metrics, K clamped to n - 1, around the 2048-query pass boundary, runs of rows
     identical to each other;
  b  the kNN stage's matrix path (n >= 65 536: the 128 closest rows by 8-bit approximate key, re-ranked in fp32) under the three metrics on
     clustered integer tables whose mates lead on the device's own 8-bit grid, and the shape of its lists on a table with a forced row;
  c  SelectEdge on pools with repeats, holes, with / without / with several copies of the node, at one distance, with rows identical to the
     node; the same lists from indices opened under COSINE and DOT_PRODUCT (everything after the kNN stage is L2);
  d  InterInsert on Link lists of a tie table, and on a hub that receives more offers than the pool holds: the closest PRUNE_POOL, twice;
  e  the navigation node on tables with an exact centroid;
  f  Link and the whole build: the properties of every list, the same lists under every engine switch and field metric, twice;
  g  wide rows: the launches between 64 and 160 KB of LDS, and the refusal above.

Each case asserts the conditions on its inputs first and prints one line `build-ties: ...` (table, metric, n, d, nodes compared, tie share)."""
import numpy as np
import pytest

import build_ref as br

pytestmark = pytest.mark.gpu

KNN_DIMS = [1, 3, 7, 16, 33, 100, 768]
KNN_NS = [2, 3, 101, 102, 2047, 2048, 2049, 4097]
KNN_FLOOR_FROM = 101       # tables of at least this many rows meet the tie floor each on its own (their lists hold 100 entries)


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd as amd
    from vectordb_amd.build import build
    build()
    return amd


def _line(table, metric, n, d, nodes, share, more=""):
    print("\nbuild-ties: table=%s metric=%s n=%d d=%d nodes_compared=%d tie_share=%.3f%s" % (table, br.METRIC_NAMES[metric], n, d, nodes, share, more))


def _index(amd, X, metric):
    ix = amd.GpuIndex(X.shape[1], metric)
    ix.attach_rows(X)
    return ix


# ------------------------------------------------------------------------------------------------ a. kNN stage, exact path
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("d", KNN_DIMS)
def test_knn_stage_exact_path_equals_the_reference(amd, d, metric):
    """The floor on the tie share is held on EVERY table whose lists have adjacent pairs to speak of (n >= 101: 100 entries a list).  A list
    of one or two entries (n = 2, 3) has no or one adjacent pair of its own: those two tables are exact in fp32 and count into the share of
    the case (all n of one width and metric), which meets the floor as well."""
    cases = []
    for n in KNN_NS:
        X = br.tie_table(n, d, metric, seed=21)
        want, wd = br.knn_lists(X, metric, 100)
        what = "knn n=%d d=%d %s" % (n, d, br.METRIC_NAMES[metric])
        if n >= KNN_FLOOR_FROM:
            share = br.preconditions(X, metric, list(wd), what)
        else:
            assert br.exact_in_fp32(X, metric), what
            share = br.wr.tie_share(list(wd))
        cases.append((n, X, want, wd, share, what))
    pooled = br.preconditions(cases[-1][1], metric, [l for c in cases for l in c[3]], "knn d=%d %s" % (d, br.METRIC_NAMES[metric]))
    for n, X, want, wd, share, what in cases:
        ix = _index(amd, X, metric)
        got = ix.knn_graph()
        ix.close()
        _line("integers", metric, n, d, n, share, " (case %.3f) K=%d" % (pooled, want.shape[1]))
        br.assert_same_lists(got, None, want, None, X, what, metric)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_knn_stage_on_runs_of_identical_rows(amd, metric):
    """runs of 140 identical rows: more than K + 1 keys tie with a row's own, so the row itself is not among its K + 1 best keys - it must
    leave by id, and the list must still hold K entries"""
    n, d = 700, 16
    X = br.runs_table(n, d, metric)
    want, wd = br.knn_lists(X, metric, 100)
    share = br.preconditions(X, metric, list(wd), "knn runs %s" % br.METRIC_NAMES[metric])
    ix = _index(amd, X, metric)
    got = ix.knn_graph()
    ix.close()
    _line("runs of 140", metric, n, d, n, share)
    br.assert_same_lists(got, None, want, None, X, "knn runs %s" % br.METRIC_NAMES[metric], metric)


# ------------------------------------------------------------------------------------------------ b. kNN stage, matrix path
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("centres,per,d", br.CLUSTER_CASES)
def test_knn_stage_matrix_path_on_clusters(amd, metric, centres, per, d):
    """Expected list of a row: its per - 1 mates by exact (distance, id) (knng = per - 1).  Asserted BEFORE knn_graph is called, on the grid
    the device reports: the restated mirror on the device's centre and step is the device's mirror, and on it every mate's accumulator is
    strictly above every outsider's for 200 sampled rows - the 128 rows taken by approximate key then contain all mates.  The floor on the
    tie share is held on every one of the nine tables (the offsets are sparse for that, build_ref.clustered_table)."""
    import test_bound_math as bm
    X, cl = br.clustered_table(centres, per, d, metric)
    n = len(X)
    assert n >= 65536 and n % 2048 != 0 and br.mates_closer(X, cl, metric, 200)
    want, wd = br.clustered_lists(X, cl, metric)
    share = br.preconditions(X, metric, list(wd), "knn matrix path %d x %d %s" % (n, d, br.METRIC_NAMES[metric]))
    ix = _index(amd, X, metric)
    rows = np.random.default_rng(4).choice(n, size=200, replace=False)
    mv = ix.mirror_view(8, X[rows])
    assert mv["usable"] and not mv["rot"] and mv["forced_rows"] == 0, (mv["usable"], mv["rot"], mv["forced_rows"])
    m = bm.mirror(X, metric, mu=mv["mu8"][:d].astype(np.float32), step=np.float32(mv["step"]))
    assert np.array_equal(m["xi"], mv["x8"][:n, :d]) and np.array_equal(m["acc0"], mv["acc0"][:n]), "the restated grid is not the device's"
    qi = np.stack([bm.query(X[r], m, metric)[0] for r in rows])
    assert np.array_equal(qi, mv["q8"][:, :d]), "the restated queries are not the device's"
    gap = br.accumulator_gap(m["xi"], m["acc0"], qi, cl, rows)
    assert gap.min() > 0 and per <= 128, "a mate's accumulator does not lead (worst gap %d) - change the TABLE" % gap.min()
    got = ix.knn_graph(knng=per - 1)
    ix.close()
    _line("clusters of %d" % per, metric, n, d, n, share, " K=%d worst accumulator gap %d" % (per - 1, gap.min()))
    br.assert_same_lists(got, None, want, None, X, "knn matrix path %d x %d %s" % (n, d, br.METRIC_NAMES[metric]), metric)


def test_knn_stage_matrix_path_lists_are_well_formed_with_a_forced_row(amd):
    """the mirror pin's table with a forced row and a clamped value, at 65 536 rows: every list holds K distinct valid ids, not the row itself,
    in distance order - judged in fp64 within the error bound of two fp32 distances (exact_ref.gamma over d + 3 terms), since these rows are
    continuous and an exact order of their fp32 distances is not restated here.  The id half of the order is checked where it is decidable
    without one: 256 rows of the table are copies of 256 others, two copies are at bit-equal distances from any node, and wherever both
    stand next to each other in a list the smaller id comes first.  Membership is not pinned here."""
    import exact_ref as xr
    from test_gpu_mirror_pin import forced_row_table
    n, d, K = 65536, 32, 100
    X = forced_row_table(np.random.default_rng(61), n, d)
    twins = np.random.default_rng(62).permutation(np.setdiff1d(np.arange(n), [n // 3, n // 2]))[:512]
    X[twins[256:]] = X[twins[:256]]
    ix = _index(amd, X, 0)
    got = ix.knn_graph()
    ix.close()
    assert got.shape == (n, K) and (got >= 0).all() and (got < n).all() and not (got == np.arange(n)[:, None]).any()
    srt = np.sort(got, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a repeated id in list %d" % int(np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(1))[0])
    X64 = X.astype(np.float64)
    g = xr.gamma(xr.free_terms(d))
    copies = 0
    for r0 in range(0, n, 4096):
        l = got[r0:r0 + 4096]
        D = ((X64[l] - X64[r0:r0 + 4096, None, :]) ** 2).sum(2)
        bad = np.argwhere(D[:, 1:] < D[:, :-1] - g * (D[:, 1:] + D[:, :-1]))
        assert len(bad) == 0, "list %d is not in distance order at position %d: %r then %r" % (r0 + bad[0][0], bad[0][1], D[bad[0][0], bad[0][1]], D[bad[0][0], bad[0][1] + 1])
        same = (X[l[:, 1:]] == X[l[:, :-1]]).all(2)          # two copies of one row next to each other: equal distances, bit for bit
        bad = np.argwhere(same & (l[:, 1:] < l[:, :-1]))
        assert len(bad) == 0, "list %d holds the copies %d, %d of one row in descending id order at position %d" % (
            r0 + bad[0][0], l[bad[0][0], bad[0][1]], l[bad[0][0], bad[0][1] + 1], bad[0][1])
        copies += int(same.sum())
    assert copies >= 256, "only %d adjacent pairs of copies in the lists: the id order is hardly checked - change the TABLE" % copies
    _line("uniform with a forced row and 256 copied rows", 0, n, d, n, 0.0, " K=%d (shape of the lists only; %d adjacent pairs of copies in id order)" % (K, copies))


# ------------------------------------------------------------------------------------------------ c. SelectEdge
@pytest.mark.parametrize("d", br.SELECT_DIMS)
def test_select_edges_equal_the_reference(amd, d):
    X = br.select_table(d)
    cases = []
    for cpn in br.SELECT_POOLS:
        nodes, cands, shapes = br.select_pools(X, cpn)
        cases.append((cpn, nodes, cands, shapes, [br.Pool(X, int(v), cands[i]) for i, v in enumerate(nodes)]))
    share = br.preconditions(X, 0, [p.dv for c in cases for p in c[4]], "select d=%d" % d)
    ixs = {m: _index(amd, br.select_table(d, m), m) for m in (0, 1, 2)}      # (the table / 16 under COSINE: the same L2 order, exactly)
    compared = 0
    for cpn, nodes, cands, shapes, pools in cases:
        for depth, R in br.select_params():
            want = np.full((len(nodes), R), -1, np.int64)
            wdeg = np.zeros(len(nodes), np.int64)
            for i, p in enumerate(pools):
                sel = br.select_from_pool(p, depth, R)
                want[i, :len(sel)], wdeg[i] = sel, len(sel)
            for m, ix in ixs.items():
                got, gdeg = ix.select_edges(nodes, cands, depth=depth, out_degree=R)
                br.assert_same_lists(got, gdeg, want, wdeg, X, "select d=%d pool=%d depth=%d R=%d index metric %s (pools: %s)" % (
                    d, cpn, depth, R, br.METRIC_NAMES[m], ", ".join(shapes)), 0, nodes)
                compared += len(nodes)
    for ix in ixs.values():
        ix.close()
    _line("integers + twins", 0, br.SELECT_N, d, compared, share, " pools=%s depths=%s R=%s, indices under L2 / COSINE / DOT" % (
        br.SELECT_POOLS, br.SELECT_DEPTHS, br.SELECT_RS))


# ------------------------------------------------------------------------------------------------ d. InterInsert
@pytest.mark.parametrize("R", [12, 50])
def test_inter_insert_equals_the_reference(amd, R):
    X, ids, deg = br.link_lists(R)
    offers = br.offers_of(ids, deg)
    share = br.preconditions(X, 0, [br.Pool(X, v, np.r_[ids[v, :deg[v]], offers[v]]).dv for v in range(len(X))], "inter_insert R=%d" % R)
    want, wdeg = br.inter_insert(X, ids, deg, R)
    ix = _index(amd, X, 0)
    got, gdeg = ix.inter_insert(ids, deg.astype(np.int32), R)
    ix.close()
    _line("integers, Link lists", 0, len(X), X.shape[1], len(X), share, " R=%d, %d pools beyond out_degree" % (R, int((br.pool_sizes(ids, deg) > R).sum())))
    br.assert_same_lists(got, gdeg, want, wdeg, X, "inter_insert R=%d" % R)


def test_inter_insert_gives_a_hub_the_closest_pool_every_time(amd):
    """node 0 receives 5999 offers: more than the PRUNE_POOL = 4096 keys of SelectEdge's pool.  The pool is the 4096 smallest keys by (dist, id)
    - not the first arrivals - so the list is the reference's, and the same on the next call."""
    X, ids, deg = br.hub_lists()
    share = br.preconditions(X, 0, [br.Pool(X, 0, np.r_[ids[0, :1], np.arange(1, br.HUB_N)]).dv], "hub")
    want, wdeg = br.inter_insert(X, ids, deg, br.HUB_R)
    ix = _index(amd, X, 0)
    first = ix.inter_insert(ids, deg.astype(np.int32), br.HUB_R)
    second = ix.inter_insert(ids, deg.astype(np.int32), br.HUB_R)
    ix.close()
    _line("integers, hub of %d offers" % (br.HUB_N - 1), 0, br.HUB_N, br.HUB_D, br.HUB_N, share, " R=%d" % br.HUB_R)
    br.assert_same_lists(first[0], first[1], want, wdeg, X, "hub, first call")
    br.assert_same_lists(second[0], second[1], want, wdeg, X, "hub, second call")


# ------------------------------------------------------------------------------------------------ e. navigation node
def _ring_knn(n, K):
    return (np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(K, dtype=np.int64)[None, :]) % n


@pytest.mark.parametrize("n", [64, 4096, 70_001 + 1])
def test_navigation_node_is_the_smallest_id_among_the_closest_to_an_exact_centroid(amd, n):
    """+- row pairs around an integer centre: every column sum is exact in fp32 in any order of the blocks' atomic adds, and the centroid is
    the centre itself.  (On continuous rows the order of those adds may move the centroid's last bit between runs; nothing is pinned there.)"""
    d = 16
    X, c = br.paired_table(n, d)
    want, dc = br.nav_node(X)
    ties = int((dc == dc.min()).sum())
    assert ties >= 2, "one closest row only - change the TABLE"
    ix = _index(amd, X, 0)
    _, _, nav = ix.link(_ring_knn(n, 8), -1, knng=8)
    ix.close()
    _line("+- pairs", 0, n, d, 1, br.wr.tie_share([np.sort(dc)[:100]]), " rows at the minimal distance: %d" % ties)
    assert nav == want, "navigation node %d (|x - c|^2 = %r), the reference has %d (%r); rows at the minimum: %s" % (
        nav, dc[nav], want, dc[want], np.flatnonzero(dc == dc.min())[:16].tolist())


# ------------------------------------------------------------------------------------------------ f. Link and the whole build
def _same(a, b, X, what):
    assert a[2] == b[2], "%s: navigation node %d vs %d" % (what, a[2], b[2])
    br.assert_same_lists(a[0], a[1], b[0], b[1], X, what)


@pytest.mark.parametrize("d", [16, 132])
def test_link_and_build_on_a_tie_table(amd, monkeypatch, d):
    n, R = 3000, 50
    X = br.tie_table(n, d, 0, seed=31)
    knn, kd = br.knn_lists(X, 0, 100)
    for name in ("EPS_BUILD_PREFILTER", "EPS_BUILD_VISITED"):
        monkeypatch.delenv(name, raising=False)
    ix = _index(amd, X, 0)
    assert ix.mirror_view(8)["usable"], "no 8-bit mirror at %d x %d: the prefilter runs of this case would be vacuous - change the TABLE" % (n, d)
    base = ix.link(knn, -1)
    dists = br.check_link_lists(X, knn, base[0], base[1], R, "link d=%d" % d)
    share = br.preconditions(X, 0, list(kd) + dists, "link d=%d" % d)
    runs = 1
    for pf in ("0", "1"):
        for vis in (None, "bitmap", "lds"):
            monkeypatch.setenv("EPS_BUILD_PREFILTER", pf)
            if vis:
                monkeypatch.setenv("EPS_BUILD_VISITED", vis)
            else:
                monkeypatch.delenv("EPS_BUILD_VISITED", raising=False)
            _same(ix.link(knn, -1), base, X, "link d=%d prefilter=%s visited=%s" % (d, pf, vis))
            runs += 1
    monkeypatch.delenv("EPS_BUILD_VISITED", raising=False)
    graphs = []
    for pf in ("0", "1", "1"):                       # the whole build: prefilter off, on, and on once more
        monkeypatch.setenv("EPS_BUILD_PREFILTER", pf)
        ix.build()
        graphs.append(ix.get_graph())
    ix.close()
    for g in graphs[1:]:
        assert g[2] == graphs[0][2] and np.array_equal(g[0], graphs[0][0]) and np.array_equal(g[1], graphs[0][1]), "two builds of one table differ (d=%d)" % d
    assert br.connected(*graphs[0])
    for metric in (1, 2):                            # everything after the kNN stage is L2 whatever the field's metric
        for pf in ("0", "1"):
            monkeypatch.setenv("EPS_BUILD_PREFILTER", pf)
            im = _index(amd, br.tie_table(n, d, metric, seed=31), metric)
            _same(im.link(knn, -1), base, X, "link d=%d on an index under %s, prefilter=%s" % (d, br.METRIC_NAMES[metric], pf))
            im.close()
            runs += 1
    _line("integers", 0, n, d, n * runs, share, " Link under %d switch / metric settings, 3 builds" % runs)


# ------------------------------------------------------------------------------------------------ g. wide rows
@pytest.mark.parametrize("d", br.WIDE_DIMS)
def test_wide_rows_build(amd, d):
    """SelectEdge's launch needs 20 bytes of LDS per dimension + 33 440 at out_degree 50: 54 080 bytes at d = 1030, 74 400 at 2048, 115 360
    at 4096 - above 65 536 a launch depends on the dynamic-LDS attribute being set - and 163 840 at d = 6520, all a gfx950 workgroup can
    have: the widest row the build accepts"""
    n, R = 600, 50
    X = br.wide_table(n, d, 41)
    Q = br.wide_table(16, d, 42)
    knn, kd = br.knn_lists(X, 0, 100)
    ix = _index(amd, X, 0)
    got = ix.knn_graph()
    br.assert_same_lists(got, None, knn, None, X, "knn wide d=%d" % d)
    ids, deg, nav = ix.link(knn, -1)
    dists = br.check_link_lists(X, knn, ids, deg, R, "link wide d=%d" % d)
    share = br.preconditions(X, 0, list(kd) + dists, "wide d=%d" % d)
    ix.build()
    off, nbr, nav2 = ix.get_graph()
    assert nav2 == nav and br.connected(off, nbr, nav2)
    gi, gd, gc = ix.search(Q, 10, mode=amd.MODE_GRAPH, intra_threads=1, master_queue=n)
    fi, fd, fc = ix.search(Q, 10, mode=amd.MODE_FLAT)
    ix.close()
    D = br.pair_dist(np.concatenate([X, Q]), np.arange(n, n + 16), np.arange(n))
    for qi in range(16):
        o = np.lexsort((np.arange(n), D[qi]))[:10]
        assert fi[qi].tolist() == o.tolist() and np.array_equal(fd[qi].astype(np.float64), D[qi][o]), (d, qi, "flat", fi[qi], o)
        assert gi[qi].tolist() == fi[qi].tolist() and np.array_equal(gd[qi], fd[qi]) and gc[qi] == fc[qi] == 10, (d, qi, gi[qi], fi[qi])
    _line("integers, wide", 0, n, d, 2 * n + 16, share, " LDS of SelectEdge %d bytes" % (20 * ((d + 3) // 4 * 4) + 32768 + 8 * R + 272))


@pytest.mark.parametrize("d", [6524, 8192])
def test_the_widest_rows_are_built_or_refused_by_name(amd, d):
    """d = 8192 needs 197 280 bytes of LDS per workgroup and d = 6524, the first width past the limit, 163 920; a gfx950 workgroup has
    163 840: the build is refused with EPS_DB_UNSUPPORTED_ERROR and the width limit in words before anything is launched - never a HIP error
    string"""
    from vectordb_amd._lib import EPS_DB_UNSUPPORTED_ERROR, EpsillaError
    n = 600
    X = br.tie_table(n, d, 0, seed=43)
    ix = _index(amd, X, 0)
    try:
        ix.build()
    except EpsillaError as e:
        msg = str(e)
        assert e.code == EPS_DB_UNSUPPORTED_ERROR, msg
        assert "width limit" in msg and str(d) in msg and "LDS" in msg, msg
        assert "hip" not in msg.lower(), msg
        for call in (lambda: ix.link(br.knn_lists(X[:, :64], 0, 100)[0], -1), lambda: ix.select_edges(np.arange(4), np.arange(8).reshape(4, 2) + 10),
                     lambda: ix.inter_insert(np.full((n, 50), -1, np.int64), np.zeros(n, np.int32), 50)):
            with pytest.raises(EpsillaError) as ei:
                call()
            assert ei.value.code == EPS_DB_UNSUPPORTED_ERROR and "width limit" in str(ei.value) and "hip" not in str(ei.value).lower(), str(ei.value)
        _line("integers, widest", 0, n, d, 0, 0.0, " refused: %s" % msg)
    else:
        off, nbr, nav = ix.get_graph()
        assert br.connected(off, nbr, nav)
        _line("integers, widest", 0, n, d, n, 0.0, " built")
    ix.close()
