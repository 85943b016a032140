"""The traversal kernel (csrc/traverse2_kernel.hpp) against the oracle's SearchImpl under the lockstep schedule, BIT FOR BIT, on tables of
ties (tests/walk_ref.py): small integers, so that fp32 computes every distance exactly in any summation order and the walk is a pure
function of its inputs.  Every id, every distance value and the evaluation count must be the oracle's - no tolerance, no set difference, no
slack on the count.  A large share of all comparisons on such tables are ties: `dist == bound` at the `dist > bound` test, equal distances
ordered by id, the duplicate test inside a run of equal keys, the last-slot overwrite of the queue merge, the rank sort + in-place merge of a
whole expansion, the 8-bit prefilter at equality.  The wide tables hold every form of the distance phases (lane groups, the scalar form, the
fused one-wavefront-per-row phase, more than three pieces per lane) to the same exact reference.  tests/test_gpu_traverse.py and
tests/test_gpu_fuzz.py keep the continuous tables, where a tolerance is justified.

Each case asserts the conditions on its inputs first (walk_ref.preconditions) and prints one line `walk-ties: ...`."""
import numpy as np
import pytest

import walk_ref as wr
from test_gpu_build import check_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd as amd
    from vectordb_amd.build import build
    build()
    return amd


def _report(c, Lq, pf, share, nq, st):
    print("\nwalk-ties: n=%d d=%d metric=%s T=%d L=%d Lq=%d I=%d prefilter=%s tie_share=%.3f evals/query=%.1f rerank_rows/dist_evals=%d/%d (%.3f)" % (
        c["n"], c["d"], wr.METRIC_NAMES[c["metric"]], c["T"], c["L"], Lq, c["I"], pf, share, st["dist_evals"] / float(nq), st["rerank_rows"],
        st["dist_evals"], st["rerank_rows"] / float(max(st["dist_evals"], 1))))


def _prefilter_worked(st, unfiltered, what):
    """With the prefilter forced on: 0 < rerank_rows <= dist_evals.  rerank_rows counts the fp32 rows the neighbour phase still read; the
    seeds (SearchQueueSize rows per query) and an appended tail are evaluated without the prefilter and are not in it, so the bound that is
    held is the tighter rerank_rows <= dist_evals - unfiltered, and `0 <` is asked wherever the walk evaluated a neighbour at all: with
    SearchQueueSize = the table every row is a seed, no neighbour is ever evaluated, and 0 of 0 is the only value there is."""
    nbr_evals = st["dist_evals"] - unfiltered
    assert 0 <= st["rerank_rows"] <= nbr_evals <= st["dist_evals"], (what, st["rerank_rows"], nbr_evals, st["dist_evals"])
    assert (st["rerank_rows"] > 0) == (nbr_evals > 0), (what, st["rerank_rows"], nbr_evals, st["dist_evals"])


def _run(amd, oracle, monkeypatch, c, pf, graph=None, tag=None):
    """one walk case on the device with the prefilter forced off ("0"), on ("1") or on over generation stamps ("1+stamps")"""
    X, Q, off, nbr, nav = wr.case_inputs(c, oracle, graph)
    res = wr.oracle_walks(oracle, c, graph, tag)
    what = wr.case_id(c) + " prefilter " + pf
    share = wr.preconditions(c, res, X, Q, what)
    L, Lq, kc = wr.effective(c)
    Qrun = np.tile(Q, (c["tiled"] // len(Q) + 1, 1))[:c["tiled"]] if c.get("tiled") else Q
    ix = amd.GpuIndex(c["d"], c["metric"])
    ix.attach_rows(X)
    ix.set_graph(off, nbr, nav)
    kw = dict(mode=amd.MODE_GRAPH, intra_threads=c["T"], master_queue=c["L"], local_queue=c["Lq"], sync_interval=c["I"])
    monkeypatch.setenv("EPS_TRV_VISITED", "stamps" if "stamps" in pf else "bitmap")
    want_evals = sum(res[qi % len(Q)][2] for qi in range(len(Qrun)))
    ev_off = None
    if pf[0] == "1":      # the same walk with the prefilter off, on the same index: the count must not move
        monkeypatch.setenv("EPS_TRV_PREFILTER", "0")
        ix.search(Qrun, c["k"], **kw)
        ev_off = ix.stats()["dist_evals"]
    monkeypatch.setenv("EPS_TRV_PREFILTER", pf[0])
    ids, dist, cnt = ix.search(Qrun, c["k"], **kw)
    st = ix.stats()
    ix.close()
    _report(c, Lq, pf, share, len(Qrun), st)
    for qi in range(0, len(Qrun), c.get("check_every", 1)):
        oid, od, _ = res[qi % len(Q)]
        wr.assert_same_walk(ids[qi], dist[qi], cnt[qi], oid, od, kc, "%s q%d" % (what, qi))
    wr.same_evals(st["dist_evals"], want_evals, what)
    if pf[0] == "1":
        _prefilter_worked(st, len(Qrun) * L, what)
        wr.same_evals(ev_off, st["dist_evals"], what + " (prefilter off against on)")


# ------------------------------------------------------------------------------------------------ 1: queue logic on heavy ties
@pytest.mark.parametrize("pf", ["0", "1", "1+stamps"])
@pytest.mark.parametrize("c", wr.queue_cases(), ids=wr.case_id)
def test_queue_logic_on_heavy_ties(amd, oracle, monkeypatch, c, pf):
    """2000 x 16, values -2..2, 24 queries, the whole returned queue: worker counts 1..32 (T = 17: past one scratch stride; T = 32: the most
    the build's out-degree allows), LDS queues of 64 to 500 keys, sync intervals 1 to 15, the three metrics; prefilter off, on, and on with
    the visited set as generation stamps."""
    _run(amd, oracle, monkeypatch, c, pf)


# ------------------------------------------------------------------------------------------------ 2: every width of the distance phases
@pytest.mark.parametrize("pf", ["0", "1"])
@pytest.mark.parametrize("c", wr.width_cases(), ids=wr.case_id)
def test_every_width_of_the_distance_phases(amd, oracle, monkeypatch, c, pf):
    """3000 rows, 32 queries, d = 19 .. 1536 (values -1..1 from d = 768): lane groups (d <= 128), the scalar form (d % 4 != 0: 19, 1030 -
    under all three metrics), the fused one-wavefront-per-row phase (d > 128, d % 4 == 0), more than three 16-byte pieces per lane (d >= 772);
    graphs over the first 16 columns from d = 132.  d = 100 also as 300 queries (the 32 tiled): the 4-wavefront form, every 10th checked."""
    _run(amd, oracle, monkeypatch, c, pf)


# ------------------------------------------------------------------------------------------------ 3: queues beyond LDS
@pytest.fixture(scope="module")
def device_graph(amd):
    """the 12000 x 24 tie table's graph, built by the device - twice, to the same arrays.  No parity with the reference's build is claimed on
    ties (its std::sort on Neighbor is unstable there, oracle/epsilla_oracle.c); the graph has to be a graph: check_graph of test_gpu_build.py."""
    c = wr.large_cases()[0]
    X, Q = wr.tie_table(c["n"], c["d"], c["nq"], c["metric"], c["seed"])
    graphs = []
    for _ in range(2):
        ix = amd.GpuIndex(c["d"], c["metric"])
        ix.attach_rows(X)
        ix.build(c["n"])
        graphs.append(ix.get_graph())
        ix.close()
    (o1, n1, v1), (o2, n2, v2) = graphs
    assert v1 == v2 and np.array_equal(o1, o2) and np.array_equal(n1, n2), "two builds of the tie table differ"
    check_graph(o1, n1, v1, c["n"])
    return o1.astype(np.int64), n1.astype(np.int64), int(v1)


@pytest.mark.parametrize("pf", ["0", "1"])
@pytest.mark.parametrize("c", wr.large_cases(), ids=wr.case_id)
def test_queues_beyond_lds(amd, oracle, monkeypatch, device_graph, c, pf):
    """12000 x 24, 6 queries, the first 1000 entries of SearchQueueSize 2500 .. 12000 (the whole table): queues in HBM, the bitonic sort
    staged through LDS, chunked in-place merges - on a graph the device built on the tie table."""
    _run(amd, oracle, monkeypatch, c, pf, graph=device_graph, tag="device")


# ------------------------------------------------------------------------------------------------ 4: shapes of adjacency and queues
@pytest.mark.parametrize("pf", ["0", "1"])
@pytest.mark.parametrize("c", wr.shape_cases(), ids=wr.case_id)
def test_shapes_of_adjacency_and_queues(amd, oracle, monkeypatch, c, pf):
    """The case 1 table with lists beyond 64 entries (the CSR form), duplicate entries and isolated nodes; LocalQueueSize below
    SearchQueueSize with k beyond it (counts equal LocalQueueSize); SearchQueueSize 5000 on 600 rows (clamped: the queue is the table)."""
    _run(amd, oracle, monkeypatch, c, pf)


# ------------------------------------------------------------------------------------------------ 5: the whole Search path
@pytest.mark.parametrize("pf", ["0", "1"])
@pytest.mark.parametrize("T", [1, 4])
def test_whole_search_path_on_ties(amd, oracle, monkeypatch, T, pf):
    """MODE_REFERENCE: graph over 3000 rows, 500 appended rows, every 4th row deleted, `column >= 250`: the walk, the brute-force tail, the
    merge into the first K slots and the post-filter against oracle.search - ids, distance values, counts, evaluations.  Ties cross the
    border between graph and tail (asserted on the inputs)."""
    c = wr.SEARCH_CASE
    X, Q, off, nbr, nav, dele, col = wr.search_inputs(oracle)
    res = wr.oracle_searches(oracle, T)
    share = wr.preconditions(dict(compared=c["limit"], metric=c["metric"]), res, X, Q, "search T%d" % T)
    assert wr.border_ties(res, c["n"]) >= 1
    monkeypatch.setenv("EPS_TRV_PREFILTER", pf)
    ix = amd.GpuIndex(c["d"], c["metric"])
    ix.attach_rows(X[:c["n"]])
    ix.set_graph(off, nbr, nav)
    ix.append_rows(X[c["n"]:])
    ix.set_deleted(dele)
    ix.set_int_filter(col, c["op"], c["value"])
    ids, dist, cnt = ix.search(Q, c["limit"], mode=amd.MODE_REFERENCE, intra_threads=T, master_queue=c["L"], local_queue=c["Lq"], sync_interval=c["I"])
    st = ix.stats()
    ix.close()
    _report(dict(c, n=c["n"] + c["n_tail"], T=T), c["Lq"], pf, share, len(Q), st)
    for qi, (oid, od, ev) in enumerate(res):
        wr.assert_same_walk(ids[qi], dist[qi], cnt[qi], oid, od, len(oid), "search T%d q%d" % (T, qi))
    wr.same_evals(st["dist_evals"], sum(r[2] for r in res), "search T%d" % T)
    if pf == "1":
        _prefilter_worked(st, len(Q) * (c["L"] + c["n_tail"]), "search T%d" % T)
