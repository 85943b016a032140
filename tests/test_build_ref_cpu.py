"""tests/build_ref.py before a device is asked (no GPU):  1 the restatement equals the oracle - eo_knn_exact, eo_select_edge, eo_inter_insert,
each pinned to the reference's own code by test_oracle_vs_ref.py - on continuous tables (build_ref.fine_table: a grid fine enough that equal
distances are ruled out list by list, coarse enough that the oracle's fp32 is exact), where the oracle is defined; pools WITH and WITHOUT the
node itself at depths 0 / 1 / 40 / 300, which is what decides how `depth` counts;  2 every planted
fault changes an answer on the tie tables tests/test_gpu_build_ties.py compares on - a comparison that cannot see one of them is not a pin;
3 the conditions on those tables."""
import numpy as np
import pytest

import build_ref as br


# ------------------------------------------------------------------------------------------------ 1. the restatement against the oracle
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_knn_lists_equal_the_oracles_exact_knn(oracle, metric):
    for n, d, K in ((700, 7, 100), (90, 24, 100), (2, 5, 100), (3, 16, 100)):
        X = br.fine_table(n, d, 100 + d)
        assert not br.on_grid(X)
        got, _ = br.knn_lists(X, metric, K)                    # (the oracle orders its lists by (distance, id) too: equal distances may stay)
        want = oracle.knn_exact(metric, X, min(K, n - 1))
        assert got.shape == want.shape and np.array_equal(got, want), (metric, n, d)


def _continuous_pools(X, cpn, m, rng, with_node):
    """m pools of cpn candidates at DISTINCT distances from their node (redrawn until they are); every fourth is ragged"""
    n = len(X)
    nodes = rng.choice(n, size=m, replace=False).astype(np.int64)
    cands = np.empty((m, cpn), np.int64)
    for i, v in enumerate(nodes):
        while True:
            c = rng.choice(np.setdiff1d(np.arange(n), [v]), size=cpn, replace=False)
            if br.distinct(br.pair_dist(X, [v], c)[0]):
                break
        cands[i] = c
    if with_node:
        cands[np.arange(m), rng.integers(cpn, size=m)] = nodes
    if cpn > 4:
        cands[::4, -2:] = -1
    return nodes, cands


@pytest.mark.parametrize("with_node", [True, False])
def test_select_edge_equals_the_oracle_with_and_without_the_node(oracle, with_node):
    """depth counts pool POSITIONS 0 .. depth in the reference: `depth` candidates when the node sorts first and is skipped, depth + 1 when it
    is not in its pool.  The restatement must follow the oracle in both.  One stated exception: unlimited (depth 0) over candidates that fit
    into out_degree keeps them ALL - InterInsert's rule when nothing overflows (nsg.cpp:640-650), which is the only caller of the unlimited
    form; the oracle's eo_select_edge prunes there, so those calls are held to the sorted candidates instead."""
    n, d = 3000, 16
    X = br.fine_table(n, d, 7)
    rng = np.random.default_rng(8)
    checked = fits = 0
    for cpn in (1, 2, 5, 64, 420):
        nodes, cands = _continuous_pools(X, cpn, 24, rng, with_node)
        for depth in (0, 1, 40, 300):
            for R in (1, 4, 8, 50):
                for i, v in enumerate(nodes):
                    got = br.select_edge(X, int(v), cands[i], depth, R)
                    c = cands[i][(cands[i] >= 0) & (cands[i] != v)]
                    if depth == 0 and len(c) <= R:
                        want = c[np.argsort(br.pair_dist(X, [v], c)[0])]
                        fits += 1
                    else:
                        want = oracle.select_edge(X, int(v), cands[i], depth, R)
                    assert list(got) == list(want), (with_node, cpn, depth, R, int(v), list(got), list(want))
                    checked += 1
    assert checked == 5 * 4 * 4 * 24 and 0 < fits < checked // 4


def test_depth_counts_one_more_candidate_when_the_node_is_absent(oracle):
    """the same pool with and without the node, at a depth that binds: the oracle's list over the pool without the node may reach one
    candidate further - stated once in the open, so that the rule is not only implied by list equality"""
    n, d = 2000, 8
    X = br.fine_table(n, d, 9)
    rng = np.random.default_rng(10)
    longer = 0
    for v in range(40):
        c = _continuous_pools(X, 60, 1, rng, False)[1][0]
        c = c[(c != v) & (c >= 0)]
        order = c[np.argsort(br.pair_dist(X, [v], c)[0])]
        for depth in (1, 5, 40):
            without = list(oracle.select_edge(X, v, c, depth, 50))
            withv = list(oracle.select_edge(X, v, np.r_[c, v], depth, 50))
            assert set(withv) <= set(order[:depth].tolist()) and set(without) <= set(order[:depth + 1].tolist())
            assert withv == list(br.select_edge(X, v, np.r_[c, v], depth, 50)) and without == list(br.select_edge(X, v, c, depth, 50))
            longer += int(order[depth]) in without
    assert longer > 0


def test_inter_insert_equals_the_oracle_where_the_oracle_is_defined(oracle):
    """a node whose candidates fit into out_degree keeps (own edges U offers) on both sides - the reference appends, the device's rule sorts:
    same set; a node whose candidates overflow gets ONE SelectEdge(unlimited) over all of them by the stated rule, the oracle's SelectEdge on
    that set (the reference's incremental result there is order dependent by design)."""
    n, d = 1500, 16
    X = br.fine_table(n, d, 19)
    knn = oracle.knn_exact(0, X, 30)
    for R in (12, 50):
        ids0 = np.full((n, R), -1, np.int64)
        deg0 = np.zeros(n, np.int64)
        for v in range(n):
            sel = oracle.select_edge(X, v, knn[v], 300, R)
            ids0[v, :len(sel)], deg0[v] = sel, len(sel)
        got, gdeg = br.inter_insert(X, ids0, deg0, R)
        want, wdeg = oracle.inter_insert(X, ids0, deg0, R)
        offers = br.offers_of(ids0, deg0)
        fit = over = 0
        for v in range(n):
            cand = np.unique(np.r_[ids0[v, :deg0[v]], offers[v]])
            if not br.distinct(br.pair_dist(X, [v], cand)[0]):     # (the oracle's stable sort leaves equal distances in input order)
                continue
            mine = got[v, :gdeg[v]].tolist()
            if len(cand) <= R:
                fit += 1
                assert sorted(mine) == sorted(cand.tolist()) == sorted(want[v, :wdeg[v]].tolist()), (R, v)
            else:
                over += 1
                assert mine == list(oracle.select_edge(X, v, cand, 0, R)), (R, v)
        assert fit > 0 and (R == 50 or over > 0)


# ------------------------------------------------------------------------------------------------ 2. planted faults
def _select_answers(d, **fault):
    """every list of the SelectEdge pin at width d, as a tuple - with a fault planted into the rule, or none"""
    pool_kw = {k: v for k, v in fault.items() if k in ("descending_ids", "keep_repeats")}
    walk_kw = {k: v for k, v in fault.items() if k in ("strict", "keep_self", "depth_shift")}
    X = br.select_table(d)
    out = []
    for cpn in br.SELECT_POOLS:
        nodes, cands, _ = br.select_pools(X, cpn)
        for i, v in enumerate(nodes):
            pool = br.Pool(X, int(v), cands[i], **pool_kw)
            out += [tuple(br.select_from_pool(pool, depth, R, **walk_kw).tolist()) for depth, R in br.select_params()]
    return out


@pytest.fixture(scope="module")
def select_truth():
    return _select_answers(16)


@pytest.mark.parametrize("name,fault", [("<= for < in the MRNG test", dict(strict=False)), ("ties by descending id", dict(descending_ids=True)),
                                        ("self kept", dict(keep_self=True)), ("a repeated candidate kept twice", dict(keep_repeats=True)),
                                        ("depth one too many", dict(depth_shift=1)), ("depth one too few", dict(depth_shift=-1))])
def test_a_planted_fault_in_select_edge_changes_an_answer(select_truth, name, fault):
    wrong = _select_answers(16, **fault)
    differ = sum(a != b for a, b in zip(select_truth, wrong))
    print("\nplanted fault '%s': %d of %d lists differ" % (name, differ, len(wrong)))
    assert differ > 0, name


def test_first_arrivals_instead_of_the_closest_changes_the_hub():
    X, ids, deg = br.hub_lists()
    assert br.pool_sizes(ids, deg)[0] == br.HUB_N and br.HUB_N > br.PRUNE_POOL
    want, wd = br.inter_insert(X, ids, deg, br.HUB_R, nodes=[0])
    wrong, xd = br.inter_insert(X, ids, deg, br.HUB_R, nodes=[0], first_arrivals=True)
    assert want[0].tolist() != wrong[0].tolist()
    # and the rule is a function of the SET of offers: any arrival order gives the same list
    perm = np.random.default_rng(3).permutation(np.arange(1, br.HUB_N))
    pool = br.Pool(X, 0, np.r_[ids[0, :1], perm])
    assert br.select_from_pool(pool, 0, br.HUB_R).tolist() == want[0, :wd[0]].tolist()


def test_planted_faults_in_the_knn_rule_change_a_list():
    """ties by descending id; self excluded by distance instead of by id (the runs table: a row's twins sit at its own distance)"""
    X = br.runs_table(700, 16, 0)
    ids, dist = br.knn_lists(X, 0, 100)
    D = br.pair_dist(X, np.arange(700), np.arange(700), 0)
    by_desc = np.stack([np.lexsort((-np.arange(700), D[i]))[:101] for i in range(700)])
    assert any(ids[i].tolist() != [x for x in by_desc[i] if x != i][:100] for i in range(700))
    first_dropped = np.stack([np.lexsort((np.arange(700), D[i]))[1:101] for i in range(700)])      # "the closest key is the row itself"
    assert (first_dropped != ids).any()
    assert not (ids == np.arange(700)[:, None]).any()


# ------------------------------------------------------------------------------------------------ 3. the conditions on the tables
@pytest.mark.parametrize("d", br.SELECT_DIMS)
def test_select_tables_are_exact_and_full_of_ties(d):
    X = br.select_table(d)
    for metric in (0, 1, 2):
        assert br.exact_in_fp32(br.select_table(d, metric), metric)
    lists = []
    for cpn in br.SELECT_POOLS:
        nodes, cands, shapes = br.select_pools(X, cpn)
        assert shapes == br.POOL_SHAPES
        for i, v in enumerate(nodes):
            has = int((cands[i] == v).sum())
            if shapes[i] == "node x3":
                assert has >= 1 and (cpn < 64 or has >= 2)
            else:
                assert has == {"node": 1, "holes+node": 1, "twins": 1 if cpn > 1 else 0}.get(shapes[i], 0), (shapes[i], cpn, has)
            lists.append(br.Pool(X, int(v), cands[i]).dv)
            if shapes[i] == "one distance":
                assert len(np.unique(lists[-1])) == 1
            if shapes[i] == "twins" and cpn > 1:
                assert (lists[-1] == 0).sum() >= 2             # the node and rows identical to it
    share = br.preconditions(X, 0, lists, "select d=%d" % d)
    print("\nselect tables d=%d: tie share of the sorted pools %.3f" % (d, share))


def test_inter_insert_tables_are_exact_and_full_of_ties():
    for R in (12, 50):
        X, ids, deg = br.link_lists(R)
        offers = br.offers_of(ids, deg)
        lists = [br.Pool(X, v, np.r_[ids[v, :deg[v]], offers[v]]).dv for v in range(len(X))]
        share = br.preconditions(X, 0, lists, "inter_insert R=%d" % R)
        over = int((br.pool_sizes(ids, deg) > R).sum())
        print("\ninter_insert R=%d: tie share %.3f, %d pools beyond out_degree" % (R, share, over))
        assert R == 50 or over > 0
    X, ids, deg = br.hub_lists()
    br.preconditions(X, 0, [br.Pool(X, 0, np.r_[ids[0, :1], np.arange(1, br.HUB_N)]).dv], "hub")


def test_grid_distances_are_the_fp64_reference():
    """pair_dist's Gram form on a grid table is exact_ref.dist64, value for value"""
    import exact_ref as xr
    for metric in (0, 1, 2):
        X = br.tie_table(300, 33, metric, seed=2)
        a, b = np.arange(0, 300, 7), np.arange(300)
        assert np.array_equal(br.pair_dist(X, a, b, metric), xr.dist64(X[b], X[a], metric).T)
        Xc, cl = br.clustered_table(40, 24, 72, metric)
        assert np.array_equal(br.pair_dist(Xc, a, np.arange(len(Xc)), metric), xr.dist64(Xc, Xc[a], metric).T)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_a_clusters_mates_in_order_are_its_rows_knn_lists(metric):
    """clustered_lists (the expected lists of the matrix path's case, cluster by cluster) is knn_lists over the whole table where every mate
    is closer than every outsider - on a table small enough to ask knn_lists for every row"""
    for centres, per, d in ((40, 24, 72), (12, 101, 16)):
        X, cl = br.clustered_table(centres, per, d, metric)
        assert br.mates_closer(X, cl, metric, len(X))
        ids, dist = br.clustered_lists(X, cl, metric)
        want, wd = br.knn_lists(X, metric, per - 1)
        assert np.array_equal(ids, want) and np.array_equal(dist, wd)
        assert br.wr.tie_share(list(dist)) >= br.TIE_FLOOR


def test_nav_and_link_checks_catch_what_they_name():
    X, c = br.paired_table(64, 16)
    nav, d = br.nav_node(X)
    assert np.array_equal(X.astype(np.float64).mean(0), c) and d[nav] == d.min() and not (d[:nav] == d.min()).any()
    Xl, ids, deg = br.link_lists(12)
    knn = br.knn_lists(Xl, 0, br.LINK_K)[0]
    br.check_link_lists(Xl, knn, ids, deg, 12)
    for spoil in ("self", "repeat", "order", "hole", "mrng"):
        bad, bdeg = ids.copy(), deg.copy()
        v = int(np.flatnonzero(deg >= 3)[0])
        if spoil == "self":
            bad[v, 1] = v
        elif spoil == "repeat":
            bad[v, 2] = bad[v, 1]
        elif spoil == "order":
            bad[v, [0, 1]] = bad[v, [1, 0]]
        elif spoil == "hole":
            bad[v, 1] = -1
        else:                                                   # a pruned kNN entry put back behind the kept ones
            pruned = [int(x) for x in knn[v] if x not in ids[v, :deg[v]]]
            far = max(pruned, key=lambda x: (br.pair_dist(Xl, [v], [x])[0, 0], x))
            bad[v, deg[v]] = far
            bdeg[v] += 1
        with pytest.raises(AssertionError):
            br.check_link_lists(Xl, knn, bad, bdeg, 12)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_cluster_mates_lead_on_the_restated_8bit_grid(metric):
    """the condition of the matrix path's case on the grid test_bound_math.mirror restates (identity frame, the table's own centre): on the
    24-rows-per-cluster table every mate's accumulator is strictly above every outsider's, for 200 sampled rows and without a forced row -
    the 128 rows the kNN stage takes by approximate key then contain the 23 mates, and the exact re-rank decides their order"""
    import test_bound_math as bm
    centres, per, d = br.CLUSTER_CASES[2]
    X, cl = br.clustered_table(centres, per, d, metric)
    assert br.exact_in_fp32(X, metric) and br.mates_closer(X, cl, metric, 200)
    m = bm.mirror(X, metric)
    assert not m["forced"].any()
    rows = np.random.default_rng(4).choice(len(X), size=200, replace=False)
    qi = np.stack([bm.query(X[r], m, metric)[0] for r in rows])
    gap = br.accumulator_gap(m["xi"], m["acc0"], qi, cl, rows)
    print("\ncluster condition, metric %s: worst gap %d accumulator units" % (br.METRIC_NAMES[metric], gap.min()))
    assert gap.min() > 0


@pytest.mark.parametrize("d", [1, 3, 7, 16, 33, 100, 768])
def test_knn_tables_are_exact_and_full_of_ties(d):
    """the tables of the kNN pin's exact path, as test_gpu_build_ties.py draws them: exact in fp32 under each metric; every table of 101 rows
    or more meets the floor on its own, and the lists of a case (all n of one width and metric, the tables of 2 and 3 rows among them) do"""
    import test_gpu_build_ties as gt
    assert d in gt.KNN_DIMS and len(gt.KNN_DIMS) == 7 and gt.KNN_FLOOR_FROM == 101 and sorted(n for n in gt.KNN_NS if n < 101) == [2, 3]
    for metric in (0, 1, 2):
        lists = []
        for n in gt.KNN_NS:
            X = br.tie_table(n, d, metric, seed=21)
            assert br.exact_in_fp32(X, metric)
            mine = list(br.knn_lists(X, metric, 100)[1])
            if n >= gt.KNN_FLOOR_FROM:
                br.preconditions(X, metric, mine, "knn n=%d d=%d %s" % (n, d, br.METRIC_NAMES[metric]))
            lists += mine
        br.preconditions(X, metric, lists, "knn d=%d %s" % (d, br.METRIC_NAMES[metric]))


def test_the_other_tables_of_the_gpu_pins_meet_their_conditions():
    for metric in (0, 1, 2):                                     # runs of identical rows
        X = br.runs_table(700, 16, metric)
        br.preconditions(X, metric, list(br.knn_lists(X, metric, 100)[1]), "runs")
    for n, d, seed in ((3000, 16, 31), (3000, 132, 31), (600, 1030, 41), (600, 2048, 41), (600, 4096, 41), (600, 6520, 41)):      # Link / build, wide rows
        for metric in (0, 1, 2) if n == 3000 else ():
            assert br.exact_in_fp32(br.tie_table(n, d, metric, seed=seed), metric)
        X = br.tie_table(n, d, 0, seed=seed) if n == 3000 else br.wide_table(n, d, seed)
        assert X.shape == (n, d) and (n == 3000 or (d in br.WIDE_DIMS and (X != 0).any(0).all()))
        br.preconditions(X, 0, list(br.knn_lists(X, 0, 100)[1]), "link / wide %d x %d" % (n, d))
    for n in (64, 4096, 70002):                                  # navigation node: an exact centroid, more than one closest row
        X, c = br.paired_table(n, 16)
        nav, dc = br.nav_node(X)
        assert (dc == dc.min()).sum() >= 2 and br.exact_in_fp32(X, 0)
    for centres, per, d in br.CLUSTER_CASES:                     # matrix path: exact, full of ties, every mate closer than every outsider
        for metric in (0, 1, 2):
            X, cl = br.clustered_table(centres, per, d, metric)
            assert len(X) >= 65536 and len(X) % 2048 and br.mates_closer(X, cl, metric, 200)
            assert np.abs(X[:, :16]).min() * (16 if metric == 1 else 1) >= 99 and set(np.unique(X[:, 16:] * (16 if metric == 1 else 1))) <= {-1.0, 0.0, 1.0}
            share = br.preconditions(X, metric, list(br.clustered_lists(X, cl, metric)[1]), "clusters of %d, d=%d, %s" % (per, d, br.METRIC_NAMES[metric]))
            print("\nclusters of %d, d=%d, %s: tie share of the mates' lists %.3f" % (per, d, br.METRIC_NAMES[metric], share))
