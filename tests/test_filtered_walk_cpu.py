"""tests/filtered_walk_ref.py on the CPU: the oracle's evaluation log moves nothing, the conditions on the inputs hold for every case
tests/test_gpu_traverse_filtered_ties.py runs (one case list, defined in filtered_walk_ref.py), every planted fault of the MODEL - a variant of the
numpy rule, never of project code - gives a different answer on these inputs, and the comparator can fail.

The nine conditions of a filtered case, from the oracle and fp64 alone:
  1 the log's length is the oracle's evaluation count;  2 its ids are distinct;  3 its first L ids are prepare_init_ids;  4 every logged
  distance equals its fp64 distance exactly;  5 the tie share of the expected answers is at least walk_ref.TIE_FLOOR (where an answer holds
  two rows at all);  6 at least one query has equal distances at ranks Kf and Kf + 1 of its visible candidates (where more than Kf exist);
  and in every SELECTIVE case at least one query's  7 expected answer holds an indexed row that is not in the oracle's final queue,  8 expected
  answer holds an indexed row the bound dropped when it was evaluated (a row of the tail is in no queue and no log: it does not count),  9 answer under the reference's semantics (oracle.search, same filter) is shorter than k."""
import numpy as np
import pytest

import filtered_walk_ref as fr
import walk_ref as wr

GROUPS = "abcdefghi"


def _stand_in_graph(n):
    """group e walks a graph the device builds; here a random CSR stands in for it, as in tests/test_walk_ties_cpu.py"""
    return fr.random_csr(n, 25, 3)


def _case(oracle, c):
    graph = _stand_in_graph(c["n"]) if c["graph"] == "device" else None
    X, Q, off, nbr, nav = fr.inputs(c, oracle, graph)
    init, walks = fr.logged_walks(oracle, c, graph, "stand-in" if graph else None)
    flt = fr.filters(c, oracle)
    ref = fr.reference_counts(oracle, c, flt, graph) if c["selective"] else None
    return X, Q, init, walks, flt, ref


_MET = {}


def _met(oracle, c):
    if c["name"] not in _MET:
        X, Q, init, walks, flt, ref = _case(oracle, c)
        met, share, exp = fr.preconditions(c, init, walks, flt["vis"], X, Q, ref)
        print("\nfiltered-pre: %s visible=%.3f rows/query=%.1f reference rows/query=%s tie_share=%.3f evals/query=%.1f met=%s" % (
            c["name"], flt["vis"].mean(), np.mean([len(e[0]) for e in exp]), "-" if ref is None else "%.1f" % np.mean(ref), share,
            np.mean([w[2] for w in walks]), ",".join(str(i) for i in sorted(met) if met[i] is True)))
        _MET[c["name"]] = met
    return _MET[c["name"]]


# ------------------------------------------------------------------------------------------------ the hook moved nothing
@pytest.mark.parametrize("T", [1, 4])
def test_the_evaluation_log_moves_nothing(oracle, T):
    """search_impl with and without the log: the same queue, distances (as bits) and evaluation count; the log is off again afterwards"""
    c = [c for c in wr.queue_cases() if c["metric"] == 0 and c["T"] == T][0]
    X, Q, off, nbr, nav = wr.case_inputs(c, oracle)
    init = oracle.prepare_init_ids(off, nbr, nav, c["L"])
    for q in Q[:6]:
        kw = dict(T=T, L=c["L"], Lq=c["Lq"], I=c["I"], lockstep=True)
        a = oracle.search_impl(0, X, off, nbr, init, q, **kw)
        b = oracle.search_impl(0, X, off, nbr, init, q, log=True, **kw)
        assert len(a) == 3 and len(b) == 6
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2] == len(b[3])
        assert oracle.L.eo_eval_log_count() == 0
        a2 = oracle.search_impl(0, X, off, nbr, init, q, **kw)
        assert np.array_equal(a[0], a2[0]) and a[2] == a2[2] and oracle.L.eo_eval_log_count() == 0


# ------------------------------------------------------------------------------------------------ the conditions
@pytest.mark.parametrize("group", list(GROUPS))
def test_preconditions_hold_for_every_gpu_case(oracle, group):
    cases = [c for c in fr.all_cases() if c["fgroup"] == group]
    assert cases
    for c in cases:
        met = _met(oracle, c)
        assert all(met[i] is True for i in (1, 2, 3, 4)), (c["name"], met)
        if c["selective"]:
            assert all(met[i] is True for i in (7, 8, 9)), (c["name"], met)


def test_every_condition_is_met_by_a_named_case(oracle):
    """each of the nine is reported as met - not merely not applicable - by at least one case; 7 to 9 by every selective case, and the
    selective cases are the groups that claim it: a (all of it), e at (4, 2500), e at (4, 2500) and (1, 9000), f at T = 1 and 4"""
    first = {}
    for c in fr.all_cases():
        for i, v in _met(oracle, c).items():
            if v is True:
                first.setdefault(i, c["name"])
    print("\nfiltered-pre: conditions first met by " + ", ".join("%d: %s" % (i, first.get(i)) for i in range(1, 10)))
    assert sorted(first) == list(range(1, 10)), first
    sel = [c for c in fr.all_cases() if c["selective"]]
    assert {c["fgroup"] for c in sel} == {"a", "e", "f"} and all(c["selective"] for c in fr.cases_a())
    assert [c["name"] for c in fr.cases_e() if c["selective"]] == ["e-T4-L2500", "e-T1-L9000"] and len([c for c in fr.cases_f() if c["selective"]]) == 2


def test_whole_table_as_seeds_leaves_nothing_beyond_the_queue(oracle):
    """why e at L = 12000 = n is no selective CASE under its selective filter: the log is the seed list and the queue is the table"""
    c = fr.by_name("e-T1-L12000")
    X, Q, init, walks, flt, ref = _case(oracle, c)
    for qid, qd, ev, lid, ld, lb in walks:
        assert ev == c["n"] and np.array_equal(lid, init) and not lb.any() and np.array_equal(np.sort(qid), np.arange(c["n"]))


def test_ties_cross_the_border_between_graph_and_tail(oracle):
    for c in fr.cases_f():
        X, Q, init, walks, flt, ref = _case(oracle, c)
        exp = fr.expected(c, walks, flt["vis"], X, Q)
        assert fr.border_ties(exp, c["n"]) >= 1, c["name"]
        assert any((e[0] >= c["n"]).any() for e in exp) and any((e[0] < c["n"]).any() for e in exp)


def test_repeat_case_straddles_the_first_log(oracle):
    """some walks of the repeat case evaluate more rows than the first attempt's log holds, some fewer; the second attempt's log holds them all"""
    c = fr.cases_g()[0]
    init, walks = fr.logged_walks(oracle, c)
    ev = np.array([w[2] for w in walks])
    first = fr.first_log(c["n"], c["L"])
    assert c["n"] > fr.LOG_FLOOR and first == fr.REPEAT_FIRST_LOG and c["T"] * c["degree"] <= 2048
    assert (ev > first).any() and (ev < first).any(), ev
    second = fr.repeat_log(c["n"], int(ev.max()))
    assert second == fr.REPEAT_SECOND_LOG and ev.max() <= second < c["n"]
    # a first attempt that answered from its truncated log would be wrong: the rows it loses are the late, close ones
    flt = fr.filters(c, oracle)
    X, Q, off, nbr, nav = fr.inputs(c, oracle)
    differ = 0
    for w, q in zip(walks, Q):
        cut = (w[0], w[1], w[2], w[3][:first], w[4][:first], w[5][:first])
        differ += int(not np.array_equal(fr.rule(c, cut, flt["vis"], X, q)[0], fr.rule(c, w, flt["vis"], X, q)[0]))
    assert differ >= 1


def test_case_list_covers_what_it_claims():
    cs = fr.all_cases()
    assert len({c["name"] for c in cs}) == len(cs) and {c["fgroup"] for c in cs} == set(GROUPS)
    a = fr.cases_a()
    assert {c["T"] for c in a} == {1, 2, 4, 8, 17, 32} and {c["metric"] for c in a} == {0, 1, 2} and {c["k"] for c in a} == {10, 100}
    assert all(c["visited"] == ("bitmap", "stamps") and c["every"] == 3 and c["col"] for c in a)
    b = fr.cases_b()
    assert {c["col"][0] for c in b if c["col"]} >= {1, 2, 4, 8} and any(c["program"] and c["every"] for c in b) and any(c["program"] and not c["every"] for c in b)
    assert fr.filters(fr.by_name("b-none-visible"))["vis"].sum() == 0 and fr.filters(fr.by_name("b-all-visible"))["vis"].all()
    assert all((c["T"], c["L"]) == (4, 500) for c in b)
    c_ = fr.cases_c()
    assert [c["k"] for c in c_[:len(fr.K_CLASSES)]] == [1, 64, 65, 128, 129, 512, 1024] and max(fr.K_CLASSES) == fr.MAX_K
    assert fr.kf(fr.by_name("c-Lq60")) == 60 and fr.by_name("c-k-beyond-L")["k"] > fr.by_name("c-k-beyond-L")["L"]
    assert {c["shape"] for c in fr.cases_d()} == {"long", "holes"}
    assert [(c["T"], c["L"], c["graph"]) for c in fr.cases_e()] == [(4, 2500, "device"), (1, 12000, "device"), (1, 9000, "device")]
    s = wr.SEARCH_CASE
    assert all((c["n"], c["n_tail"], c["k"], c["mode"]) == (s["n"], s["n_tail"], s["limit"], "reference") for c in fr.cases_f()) and {c["T"] for c in fr.cases_f()} == {1, 4}
    assert [c.get("tiled") for c in fr.cases_h()] == [None] * 4 + [fr.H_TILED] and fr.H_TILED > 4 * 256 and fr.cases_h()[-1]["check_every"] == 1
    assert all(c["tiled"] == fr.E_TILED and c["check_every"] == 1 for c in fr.cases_e()) and fr.E_TILED > 256 and fr.E_TILED % 6 == 0


# ------------------------------------------------------------------------------------------------ planted faults on the model
@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_planted_variant_is_told_apart(oracle, variant):
    """a variant of the numpy rule gives a different answer from the true rule for at least one query of at least one case: these inputs can
    tell it apart, and the comparator says so"""
    told = []
    for c in fr.all_cases():
        if c["graph"] == "device" or c.get("tiled"):
            continue
        X, Q, init, walks, flt, ref = _case(oracle, c)
        n = 0
        for qi, (w, q) in enumerate(zip(walks, Q)):
            eid, ed = fr.rule(c, w, flt["vis"], X, q)
            vid, vd = fr.rule(c, w, flt["vis"], X, q, variant)
            if len(eid) == len(vid) and np.array_equal(eid, vid) and np.array_equal(ed, vd):
                continue
            n += 1
            k = max(c["k"], len(vid))
            row_i, row_d = np.full(k, -1, np.int64), np.full(k, np.inf, np.float32)
            row_i[:len(vid)], row_d[:len(vid)] = vid, vd
            with pytest.raises(AssertionError):
                fr.assert_same_filtered(row_i, row_d, len(vid), eid, ed, "%s %s q%d" % (variant, c["name"], qi))
        if n:
            told.append("%s (%d of %d queries)" % (c["name"], n, len(Q)))
    print("\nfiltered-pre: variant %s told apart by %d cases: %s" % (variant, len(told), "; ".join(told[:6])))
    assert told, "no case can tell the variant %s from the rule" % variant


# ------------------------------------------------------------------------------------------------ the comparator can fail
def test_comparator_rejects_near_misses(oracle):
    c = fr.by_name("b-deleted")
    X, Q, init, walks, flt, ref = _case(oracle, c)
    k = c["k"]
    swaps = 0
    for qi, (w, q) in enumerate(zip(walks, Q)):
        eid, ed = fr.rule(c, w, flt["vis"], X, q)
        assert len(eid) == k
        fr.assert_same_filtered(eid, ed, k, eid, ed, "clean q%d" % qi)
        pos = np.flatnonzero(ed[1:] == ed[:-1])
        if len(pos):
            p = int(pos[len(pos) // 2])
            m = eid.copy()
            m[p], m[p + 1] = m[p + 1], m[p]
            with pytest.raises(AssertionError, match="tie group"):
                fr.assert_same_filtered(m, ed, k, eid, ed)
            swaps += 1
        m = ed.copy()
        m[k // 2] = np.nextafter(m[k // 2], np.float32(np.inf))
        with pytest.raises(AssertionError):
            fr.assert_same_filtered(eid, m, k, eid, ed)
        with pytest.raises(AssertionError):
            fr.assert_same_filtered(eid, ed, k - 1, eid, ed)
        with pytest.raises(AssertionError):
            fr.assert_same_filtered(np.append(eid, 7), np.append(ed, np.float32(np.inf)), k, eid, ed)
        with pytest.raises(AssertionError):
            fr.assert_same_filtered(np.append(eid, -1), np.append(ed, np.float32(3.0)), k, eid, ed)
        fr.assert_same_filtered(np.append(eid, -1), np.append(ed, np.float32(np.inf)), k, eid, ed)
        short_i, short_d = eid.copy(), ed.copy()
        short_i[-1], short_d[-1] = -1, np.inf
        with pytest.raises(AssertionError):
            fr.assert_same_filtered(short_i, short_d, k - 1, eid, ed)
    assert swaps >= len(Q) // 2
    # an empty answer: count 0, the whole row padding
    fr.assert_same_filtered(np.full(5, -1), np.full(5, np.inf, np.float32), 0, np.zeros(0, np.int64), np.zeros(0, np.float32))
    with pytest.raises(AssertionError):
        fr.assert_same_filtered(np.array([3, -1]), np.array([1.0, np.inf], np.float32), 1, np.zeros(0, np.int64), np.zeros(0, np.float32))


def test_zero_signs_are_one_distance():
    eid, ed = np.arange(3), np.array([0.0, 0.0, 1.0], np.float32)
    fr.assert_same_filtered(eid, np.array([-0.0, 0.0, 1.0], np.float32), 3, eid, ed)
