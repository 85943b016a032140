"""The graph search under filter_in_traversal = 1 (csrc/traverse.hip graph_search_impl, the evaluation log of csrc/traverse2_kernel.hpp, the
filtered merge_lists_kernel, cap_keys_kernel) against its documented rule restated in numpy from the ORACLE's evaluation log
(tests/filtered_walk_ref.py), on tables of ties: every id, every distance value, every count and the padding must be the rule's - no
tolerance, no set comparison - and the evaluation count must be the oracle's and the unfiltered call's (the walk itself is unchanged).
tests/test_gpu_traverse.py keeps the continuous table, where only properties can be asked.

Each case asserts the conditions on its inputs first (filtered_walk_ref.preconditions; tests/test_filtered_walk_cpu.py runs them without a
device) and prints one line `filtered-ties: ...` (group h: one per step).  Where a case is about the launch's form - queues in HBM, workgroups
that walk a second query - the test reads that form from the library's own profile line (EPS_TRV_PROF), not from a belief about the plan."""
import re
import sys

import numpy as np
import pytest

import filtered_walk_ref as fr
import walk_ref as wr
from test_gpu_build import check_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd as amd
    from vectordb_amd.build import build
    build()
    return amd


def _prepare(oracle, c, graph=None, tag=None):
    """inputs, the oracle's logged walks, the filter, the conditions on them and the expected answers of a case"""
    X, Q, off, nbr, nav = fr.inputs(c, oracle, graph)
    init, walks = fr.logged_walks(oracle, c, graph, tag)
    flt = fr.filters(c, oracle)
    ref = fr.reference_counts(oracle, c, flt, graph) if c["selective"] else None
    met, share, exp = fr.preconditions(c, init, walks, flt["vis"], X, Q, ref)
    return dict(X=X, Q=Q, graph=(off, nbr, nav), walks=walks, flt=flt, share=share, exp=exp, met=met)


def _install(ix, flt):
    ix.set_deleted(flt["deleted"])
    if flt["col"] is not None:
        ix.set_int_filter(flt["col"][0], flt["col"][1], flt["col"][2])
    else:
        ix.set_int_filter(None, None, 0)
    ix.set_filter_program(flt["program"], flt["rows"])


def _index(amd, c, p):
    ix = amd.GpuIndex(c["d"], c["metric"])
    ix.attach_rows(p["X"][:c["n"]])
    ix.set_graph(*p["graph"])
    if c["n_tail"]:
        ix.append_rows(p["X"][c["n"]:])
    _install(ix, p["flt"])
    return ix


def _kw(amd, c):
    return dict(mode=amd.MODE_REFERENCE if c["mode"] == "reference" else amd.MODE_GRAPH, intra_threads=c["T"], master_queue=c["L"], local_queue=c["Lq"],
                sync_interval=c["I"])


def _queries(c, Q):
    return np.tile(Q, (c["tiled"] // len(Q) + 1, 1))[:c["tiled"]] if c.get("tiled") else Q


def _ask(amd, ix, c, p, what, extra="", say=True):
    """the case's search, unfiltered then filtered, on an index that holds its filter: every checked query is the rule's answer, the
    evaluation count is the oracle's and the unfiltered call's.  Returns (ids, dist, counts, stats, unfiltered stats) of the filtered call;
    say=False: the case's line is left in p["line"] for the caller to print."""
    Q = _queries(c, p["Q"])
    nq0 = len(p["Q"])
    kw = _kw(amd, c)
    rid, rdist, rcnt = ix.search(Q, c["k"], filter_in_traversal=0, **kw)
    st0 = ix.stats()
    ids, dist, cnt = ix.search(Q, c["k"], filter_in_traversal=1, **kw)
    st = ix.stats()
    want = sum(p["walks"][qi % nq0][2] for qi in range(len(Q))) + len(Q) * c["n_tail"]
    p["line"] = "visible=%.3f rows/query filtered=%.1f reference=%.1f tie_share=%.3f evals/query=%.1f attempts=%d" % (
        p["flt"]["vis"].mean(), cnt.mean(), rcnt.mean(), p["share"], st["dist_evals"] / float(len(Q)),
        st["main_kernel_launches"] // max(st0["main_kernel_launches"], 1))
    if say:
        print("\nfiltered-ties: %s%s %s" % (what, extra, p["line"]))
    assert ids.shape == (len(Q), c["k"]) and dist.shape == ids.shape
    for qi in range(0, len(Q), c.get("check_every", 1)):
        eid, ed = p["exp"][qi % nq0]
        fr.assert_same_filtered(ids[qi], dist[qi], cnt[qi], eid, ed, "%s q%d" % (what, qi))
    wr.same_evals(st["dist_evals"], want, what)
    wr.same_evals(st0["dist_evals"], st["dist_evals"], what + " (unfiltered against filtered)")
    return ids, dist, cnt, st, st0


def _run(amd, oracle, monkeypatch, c, graph=None, tag=None):
    """a case under each of its visited-set kinds, on one index; one line for the case (the kinds agree on every figure of it: each is
    held to the same expected answers and the same evaluation count)"""
    p = _prepare(oracle, c, graph, tag)
    ix = _index(amd, c, p)
    out, lines = None, []
    for visited in c["visited"]:
        monkeypatch.setenv("EPS_TRV_VISITED", visited)
        out = _ask(amd, ix, c, p, c["name"], say=False)
        lines.append(p["line"])
    ix.close()
    assert len(set(lines)) == 1, lines
    print("\nfiltered-ties: %s visited=%s %s" % (c["name"], "+".join(c["visited"]), lines[0]))
    return p, out


_PLAN = re.compile(r"\[eps trv\] nq=(\d+) T=(\d+) L=(\d+) I=\d+ (HBM|LDS) queues, (\d+) wavefronts/query, (\d+) slots")


def _launch_forms(capfd):
    """[(queries, T, L, "HBM" | "LDS", wavefronts per query, workgroups of a launch)] of the traversals since the last look, from the lines the
    library writes under EPS_TRV_PROF (csrc/traverse.hip print_profile); what was captured goes on to the test's own output"""
    out, err = capfd.readouterr()
    forms = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5)), int(m.group(6))) for m in _PLAN.finditer(err)]
    with capfd.disabled():
        sys.stdout.write(out)
        sys.stderr.write("".join(l + "\n" for l in err.splitlines() if "[eps trv]" not in l))
    return forms


# ------------------------------------------------------------------------------------------------ a: workers and queues
@pytest.mark.parametrize("c", fr.cases_a(), ids=fr.case_id)
def test_workers_and_queues_selective(amd, oracle, monkeypatch, c):
    """2000 x 16 (values -1..1), 24 queries, T = 1, 2, 4, 8, 17, 32 under the three metrics, every 3rd row deleted and a column test that
    leaves 0.7 % (k = 10) or 4 % (k = 100) visible: the reference's semantics starves, the answer reaches beyond the final queue and into the
    evaluations the bound dropped (conditions 7 to 9).  Visited set as bitmap and as generation stamps, on one index."""
    p, _ = _run(amd, oracle, monkeypatch, c)
    assert all(p["met"][i] is True for i in (7, 8, 9))


# ------------------------------------------------------------------------------------------------ b: filter kinds
@pytest.mark.parametrize("c", fr.cases_b(), ids=fr.case_id)
def test_filter_kinds(amd, oracle, monkeypatch, c):
    """one (T = 4, L = 500) walk: the deleted bitset alone, a column test at widths 1, 2, 4 and 8 bytes, a compiled program with an integer
    and a float leaf, program + deleted, no visible row (counts 0, ids -1), every row visible (the k best evaluated rows)"""
    p, (ids, dist, cnt, st, st0) = _run(amd, oracle, monkeypatch, c)
    if c["name"] == "b-none-visible":
        assert (cnt == 0).all() and (ids == -1).all() and np.isposinf(dist).all()
    if c["name"] == "b-all-visible":
        assert (cnt == c["k"]).all()


def test_no_filter_set_is_the_plain_search(amd, oracle, monkeypatch):
    """filter_in_traversal = 1 with no filter installed: bit for bit the plain search - ids, distances, counts, evaluations, one launch"""
    c = dict(fr.by_name("b-all-visible"), col=None, name="b-no-filter")
    X, Q, off, nbr, nav = fr.inputs(c, oracle)
    init, walks = fr.logged_walks(oracle, c)
    ix = amd.GpuIndex(c["d"], c["metric"])
    ix.attach_rows(X)
    ix.set_graph(off, nbr, nav)
    kw = _kw(amd, c)
    a = ix.search(Q, c["k"], filter_in_traversal=0, **kw)
    sa = ix.stats()
    b = ix.search(Q, c["k"], filter_in_traversal=1, **kw)
    sb = ix.stats()
    ix.close()
    print("\nfiltered-ties: b-no-filter visible=1.000 rows/query filtered=%.1f reference=%.1f tie_share=%.3f evals/query=%.1f attempts=1" % (
        b[2].mean(), a[2].mean(), wr.tie_share([w[1][:c["k"]] for w in walks]), sb["dist_evals"] / float(len(Q))))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    for key in ("dist_evals", "expansions", "main_kernel_launches", "rerank_rows"):
        assert sa[key] == sb[key], key
    for qi, (qid, qd, ev, lid, ld, lb) in enumerate(walks):
        wr.assert_same_walk(b[0][qi], b[1][qi], b[2][qi], qid, qd, c["k"], "b-no-filter q%d" % qi)
    wr.same_evals(sb["dist_evals"], sum(w[2] for w in walks), "b-no-filter")


# ------------------------------------------------------------------------------------------------ c: k and the caps
@pytest.mark.parametrize("c", fr.cases_c(), ids=fr.case_id)
def test_k_and_the_caps(amd, oracle, monkeypatch, c):
    """k = 1, 64, 65, 128, 129, 512, 1024 (the merge's keys-per-lane classes, full rows); k beyond the visible evaluated rows (count below k,
    padding); LocalQueueSize 60 < k (count 60); k = 128 > L = 64 (128 rows: Kf has no L)"""
    p, (ids, dist, cnt, st, st0) = _run(amd, oracle, monkeypatch, c)
    if c["name"].startswith("c-k") and c["name"] != "c-k-beyond-L":
        assert (cnt == c["k"]).all()
    if c["name"] == "c-short":
        assert (cnt < c["k"]).all() and (cnt > 0).all()
    if c["name"] == "c-Lq60":
        assert (cnt == 60).all()
    if c["name"] == "c-k-beyond-L":
        assert (cnt == c["k"]).all() and c["k"] > c["L"]


def test_k_beyond_1024_is_refused(amd, oracle):
    c = fr.by_name("c-k1024")
    p = _prepare(oracle, c)
    ix = _index(amd, c, p)
    with pytest.raises(amd.EpsillaError) as e:
        ix.search(p["Q"], 1025, filter_in_traversal=1, **dict(_kw(amd, c), master_queue=1025, local_queue=1025))
    assert e.value.code == 50002 and "1024" in str(e.value) and ix.L.eps_index_last_error_class(ix.h) == 1      # EPS_DB_UNSUPPORTED_ERROR, EPS_ERRCLASS_DEVICE_RANGE
    ids, dist, cnt = ix.search(p["Q"], 1025, filter_in_traversal=0, **dict(_kw(amd, c), master_queue=1025, local_queue=1025))   # (the plain search takes it)
    assert (cnt > 0).all()
    ix.close()
    print("\nfiltered-ties: c-k1025 refused: %s" % e.value)


# ------------------------------------------------------------------------------------------------ d: adjacency shapes
@pytest.mark.parametrize("c", fr.cases_d(), ids=fr.case_id)
def test_adjacency_shapes(amd, oracle, monkeypatch, c):
    """lists beyond 64 entries (the CSR form), duplicate entries, isolated nodes: no row appears twice in an answer (the comparator asks)"""
    p, (ids, dist, cnt, st, st0) = _run(amd, oracle, monkeypatch, c)
    for qi in range(len(ids)):
        got = ids[qi][:cnt[qi]]
        assert len(np.unique(got)) == len(got)


# ------------------------------------------------------------------------------------------------ e: queues in HBM
@pytest.fixture(scope="module")
def device_graph(amd):
    """the 12000 x 24 tie table's graph, built by the device (tests/test_gpu_traverse_ties.py holds two builds to one another)"""
    c = fr.cases_e()[0]
    X, Q = wr.tie_table(c["n"], c["d"], c["nq"], c["metric"], c["seed"])
    ix = amd.GpuIndex(c["d"], c["metric"])
    ix.attach_rows(X)
    ix.build(c["n"])
    off, nbr, nav = ix.get_graph()
    ix.close()
    check_graph(off, nbr, nav, c["n"])
    return off.astype(np.int64), nbr.astype(np.int64), int(nav)


@pytest.mark.parametrize("c", fr.cases_e(), ids=fr.case_id)
def test_queues_in_hbm(amd, oracle, monkeypatch, capfd, device_graph, c):
    """12000 x 24 on the device-built graph, (T, L) = (4, 2500), (1, 12000) and (1, 9000), the 6 queries tiled to 264 (in a call of up to
    256 queries all three would keep their queues in LDS), every one checked; 2 % of the rows visible, 0.7 % at (1, 9000).  The library's
    profile line must say that the queues of both calls, unfiltered and filtered, were in HBM.  At L = n every row is a seed and nothing
    lies beyond the queue: conditions 7 to 9 are asked of (4, 2500) and (1, 9000) (filtered_walk_ref.cases_e)."""
    monkeypatch.setenv("EPS_TRV_PROF", "1")
    capfd.readouterr()
    p, _ = _run(amd, oracle, monkeypatch, c, graph=device_graph, tag="device")
    forms = _launch_forms(capfd)
    assert len(forms) == 2 and all(f[:4] == (c["tiled"], c["T"], c["L"], "HBM") for f in forms), forms
    if c["selective"]:
        assert all(p["met"][i] is True for i in (7, 8, 9))


# ------------------------------------------------------------------------------------------------ f: the tail
@pytest.mark.parametrize("c", fr.cases_f(), ids=fr.case_id)
def test_tail(amd, oracle, monkeypatch, c):
    """MODE_REFERENCE: 3000 indexed + 500 appended rows, every 4th row deleted, `column >= 920`, limit 100, T = 1 and 4 - and LocalQueueSize 60:
    the cut at Kf comes after the tail merge.  Ties cross the border between graph and tail among the expected rows (asserted on the inputs)."""
    p = _prepare(oracle, c)
    assert fr.border_ties(p["exp"], c["n"]) >= 1
    ix = _index(amd, c, p)
    ids, dist, cnt, st, st0 = _ask(amd, ix, c, p, c["name"])
    ix.close()
    assert (ids[cnt > 0] >= c["n"]).any() and (cnt == fr.kf(c)).all()


# ------------------------------------------------------------------------------------------------ g: the log's repeat
def test_log_overflow_repeats_the_search(amd, oracle, monkeypatch):
    """40000 x 16, a random CSR of out-degree 96, T = 4, L = 180: the oracle evaluates more than the first attempt's 16384 log slots for some
    queries and fewer for others (tests/test_filtered_walk_cpu.py; the plan of both attempts: tests/native/graph_host_check.cpp).  The
    answers are the rule's, the evaluations are counted once, and the launch count shows the second attempt."""
    c = fr.cases_g()[0]
    p = _prepare(oracle, c)
    ev = np.array([w[2] for w in p["walks"]])
    first = fr.first_log(c["n"], c["L"])
    assert (ev > first).any() and (ev < first).any()
    ix = _index(amd, c, p)
    ids, dist, cnt, st, st0 = _ask(amd, ix, c, p, c["name"], " log=%d->%d" % (first, fr.repeat_log(c["n"], int(ev.max()))))
    assert st0["main_kernel_launches"] == 1 and st["main_kernel_launches"] == 2, (st0["main_kernel_launches"], st["main_kernel_launches"])
    ids2, dist2, cnt2, st2, _ = _ask(amd, ix, c, p, c["name"], say=False)                   # the same call once more: again two attempts, the same answer
    assert st2["main_kernel_launches"] == 2 and np.array_equal(ids, ids2) and np.array_equal(cnt, cnt2)
    ix.close()


# ------------------------------------------------------------------------------------------------ h: state between calls
def test_state_between_calls(amd, oracle, monkeypatch, capfd):
    """one index: filtered / unfiltered / filtered with another filter, a larger k, a smaller k, then the 24 queries tiled to 1100, every one
    checked - every answer is still the rule's (a stale evaluation count or log of an earlier call would show).  The tiled call is one
    launch of fewer workgroups than queries (read from the library's profile line: 1024 on 256 CUs), so some workgroups walk a second
    query on the visited set, the stamps and the log count their first one left; under both kinds of visited set.  One line per step."""
    cs = {c["name"]: c for c in fr.cases_h()}
    ps = {nm: _prepare(oracle, c) for nm, c in cs.items()}
    first = cs["h-deleted"]
    ix = _index(amd, first, ps["h-deleted"])
    monkeypatch.setenv("EPS_TRV_PROF", "1")
    steps = [("h-deleted", "bitmap"), ("h-program", "bitmap"), ("h-k128", "bitmap"), ("h-k10", "bitmap"), ("h-deleted", "bitmap"), ("h-tiled", "bitmap"),
             ("h-k10", "bitmap"), ("h-tiled", "stamps"), ("h-k10", "stamps")]
    for step, (nm, visited) in enumerate(steps):    # (_ask: an unfiltered call sits between any two filtered ones)
        monkeypatch.setenv("EPS_TRV_VISITED", visited)
        _install(ix, ps[nm]["flt"])
        capfd.readouterr()
        _ask(amd, ix, cs[nm], ps[nm], nm, " step=%d visited=%s" % (step + 1, visited))
        forms = _launch_forms(capfd)
        nq = cs[nm].get("tiled", cs[nm]["nq"])
        assert len(forms) == 2 and all(f[0] == nq for f in forms), forms
        if nm == "h-tiled":
            assert all(f[5] < nq for f in forms), "every query of the tiled step had a workgroup of its own: %r" % (forms,)
        else:
            assert all(f[5] == nq for f in forms), forms
    ix.close()


# ------------------------------------------------------------------------------------------------ i: the prefilter
def test_forced_prefilter_stays_off_on_a_filtered_call(amd, oracle, monkeypatch):
    """EPS_TRV_PREFILTER=1 on a filtered call: the same answer, and no row went through the 8-bit prefilter (rerank_rows == 0): the evaluation
    log needs the distance of every evaluated row, which the prefilter exists to avoid"""
    c = fr.cases_i()[0]
    p = _prepare(oracle, c)
    ix = _index(amd, c, p)
    monkeypatch.setenv("EPS_TRV_PREFILTER", "0")
    a = _ask(amd, ix, c, p, c["name"], say=False)
    monkeypatch.setenv("EPS_TRV_PREFILTER", "1")
    b = _ask(amd, ix, c, p, c["name"], " prefilter=1")
    ix.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    assert b[3]["rerank_rows"] == 0 and a[3]["rerank_rows"] == 0
    assert b[4]["rerank_rows"] > 0          # (the unfiltered call of the same pair did run it)
