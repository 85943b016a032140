"""GpuIndex.search_multi / eps_index_search_multi on the MI355X: the k closest groups per BAG of vectors, by the sum over the bag of each vector's
distance to the group's closest visible row; over every group (the scan's table, multi_sum_topk_kernel) or over the groups the caller names
(multi_gather_kernel), the same bits (csrc/multi.hip).

Every comparison is for equality of group keys, score bits, counts, match ids and match distance bits.  Tables of ties (every fp32 sum exact in any
order: assert_ties_bags) are held to tests/multi_ref.py, which is checked on the CPU in tests/test_multi_ref_cpu.py.  Continuous tables are held to
the same model fed with the device's own flat search with k = n: the rule is defined on those bits, and it is there that a reassociated sum fails."""
import numpy as np
import pytest

import exact_ref as er
import groups_ref as gr
import multi_ref as mr
import select_ref as sr
import stream_gate as sg
import vectordb_amd as amd
from vectordb_amd._lib import EpsillaError

pytestmark = pytest.mark.gpu

F = np.float32
METRIC = {0: "EUCLIDEAN", 1: "COSINE", 2: "DOT_PRODUCT"}
SIZES = [1, 3, 0, 4, 5, 9]   # a quad of 4 vectors, its remainders 1 and 3 (5 = 4 + 1, 9 = 4 + 4 + 1) and an empty bag in one batch
OFF = mr.bag_offsets(SIZES)
T = int(OFF[-1])


def index(X, metric, keys=None):
    ix = amd.GpuIndex(X.shape[1], METRIC[metric], device=0)
    ix.attach_rows(X)
    if keys is not None:
        ix.set_groups(keys)
    return ix


def reset(ix):
    ix.set_deleted(None)
    ix.set_int_filter(None, None, 0)
    ix.set_filter_program(None)
    ix.set_id_map(0, 1)


def packbits(hidden):
    return np.packbits(np.concatenate([hidden, np.zeros(-len(hidden) % 8, bool)]), bitorder="little")


def both_forms(ix, Q, off, k, d, vis, keys, what, best=None, **kw):
    """the whole-table form against the model; the candidate form with every key named (shared, and per bag) against the same answer"""
    want = mr.numpy_multi(d, vis, keys, off, k, best=best)
    mr.same(ix.search_multi((Q, off), k, **kw), want, what + " whole table")
    every = np.unique(keys)[::-1].copy()   # (descending: nothing relies on the list's order)
    mr.same(ix.search_multi((Q, off), k, cand_keys=every, **kw), want, what + " every key named, one list")
    nq = len(off) - 1
    mr.same(ix.search_multi((Q, off), k, cand_keys=np.tile(every, nq), cand_offsets=np.arange(nq + 1) * len(every), **kw), want, what + " every key named, per bag")
    return want


def subset_lists(keys, nq, seed):
    """per-bag lists: a random part of the keys, some twice, some unknown; one bag with an empty list, one with unknown keys only"""
    rng = np.random.default_rng(seed)
    u = np.unique(keys)
    unknown = np.setdiff1d(np.array([u.min() - 1 if u.min() > gr.I64_MIN else 5, 123456789, u.max() + 1 if u.max() < gr.I64_MAX else 7], np.int64), u)
    lists = []
    for j in range(nq):
        part = rng.choice(u, size=max(1, len(u) // 2), replace=False)
        part = np.concatenate([part, part[:3], unknown])
        lists.append(rng.permutation(part) if j != 1 else (unknown if len(unknown) else part[:0]))
    lists[-1] = lists[-1][:0]
    off = mr.bag_offsets([len(x) for x in lists])
    return np.concatenate(lists).astype(np.int64), off


# ---- 1. tables of ties against the model: every metric, width, size, layout and k, both forms
@pytest.mark.parametrize("d", [8, 20, 96])   # 16-byte form G = 2 | G = 8 (20 = 5 pieces: three lanes idle in the last) | G = 32
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3000])   # one row | a wavefront of rows less one, exactly, plus one | a chunk of 256 plus one | many blocks
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ties_tables_equal_the_model(metric, n, d):
    X, Q, d32 = gr.ties_table(metric, n, d, T, seed=metric)
    dT = np.ascontiguousarray(d32.T)
    mr.assert_ties_bags(dT, OFF, grid=1 / 256 if metric == 1 else 1)
    ix = index(X, metric)
    for name, keys in gr.layouts(n, seed=metric).items():
        ix.set_groups(keys)
        G = len(np.unique(keys))
        best = mr.minima_all(dT, np.ones(dT.shape, bool), keys)
        cand, coff = subset_lists(keys, len(SIZES), seed=n + d)
        for k in sorted({1, 10, min(G, 1024), min(G + 3, 1024)}):   # (k <= 1024 is the call's limit)
            what = "%s metric %d n %d d %d k %d" % (name, metric, n, d, k)
            want = both_forms(ix, Q, OFF, k, dT, None, keys, what, best=best)
            assert want[2][2] == 0 and (want[2][[0, 1, 3, 4, 5]] == min(k, G)).all()
            mr.check_multi(ix.search_multi((Q, OFF), k, cand_keys=cand, cand_offsets=coff), dT, None, keys, OFF, k, cand, coff, what=what + " subsets per bag", best=best)
            mr.check_multi(ix.search_multi((Q, OFF), k, cand_keys=cand[:coff[1]]), dT, None, keys, OFF, k, cand[:coff[1]], what=what + " a subset, one list", best=best)
    ix.close()


# ---- 2. continuous tables: the model fed with the device's own flat search, k = n.  A sum taken in another order fails here
@pytest.mark.parametrize("name,metric", [("gaussian", 0), ("embedding-like", 1), ("gaussian x 3 queries", 2)])
def test_continuous_tables_equal_the_model_on_the_flat_searchs_bits(name, metric):
    n, d = 3000, 64
    X, Q = er.make(name, n, d, T, seed=5)
    ix = index(X, metric)
    ids, dist, cnt = ix.search(Q, n, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    assert (cnt == n).all()
    dT = np.empty((T, n), F)
    np.put_along_axis(dT, ids, dist, axis=1)
    for lname, keys in gr.layouts(n, seed=5).items():
        if lname == "every row its own":
            keys = keys // 3000017   # (about a third of the rows share a key with a neighbour: sums over real minima, not single rows)
        ix.set_groups(keys)
        best = mr.minima_all(dT, np.ones(dT.shape, bool), keys)
        cand, coff = subset_lists(keys, len(SIZES), seed=3)
        for k in (1, 10, 100):
            both_forms(ix, Q, OFF, k, dT, None, keys, "%s %s k %d" % (name, lname, k), best=best)
            mr.check_multi(ix.search_multi((Q, OFF), k, cand_keys=cand, cand_offsets=coff), dT, None, keys, OFF, k, cand, coff, what="%s %s subsets" % (name, lname),
                           best=best)
    # the sum's order can be told on this table: the pairwise sum of the same terms differs somewhere
    keys = gr.layouts(n, seed=5)["n / 8 groups"]

    def pairwise(terms):
        t = [F(x) for x in terms]
        while len(t) > 1:
            t = [F(t[i] + t[i + 1]) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return F(F(0) + t[0])
    a, b = mr.numpy_multi(dT, None, keys, OFF, 100), mr.numpy_multi(dT, None, keys, OFF, 100, summed=pairwise)
    assert not np.array_equal(a[1], b[1], equal_nan=True), "VACUOUS: a pairwise sum gives the same scores on this table"
    ix.close()


# ---- 3. the chunk boundary of the gather, one group holding the table, unknown keys only
@pytest.fixture(scope="module")
def table4():
    n, d = 3000, 20
    X, Q, d32 = gr.ties_table(0, n, d, T, seed=4)
    keys = gr.layouts(n, seed=4)["n / 8 groups"] * 11 - 2000
    ix = index(X, 0, keys)
    yield ix, X, Q, np.ascontiguousarray(d32.T), keys
    ix.close()


def test_candidate_groups_around_the_chunk_of_256_rows(table4):
    ix, X, Q, dT, _ = table4
    reset(ix)
    sizes = [255, 256, 257, 513, 1, 2]   # one chunk less a row | exactly one | one and a row | two and a row
    keys = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 9, sizes)
    keys = np.concatenate([keys, np.arange(3000 - len(keys), dtype=np.int64) + 1000])
    keys = keys[np.random.default_rng(1).permutation(3000)]
    ix.set_groups(keys)
    named = np.arange(len(sizes), dtype=np.int64) * 7 - 9
    for k in (1, 6, 7):
        mr.check_multi(ix.search_multi((Q, OFF), k, cand_keys=named), dT, None, keys, OFF, k, named, what="chunk boundary k %d" % k)
    st = ix.stats()
    assert st["dist_evals"] == sum(sizes) * T and st["main_kernel_bits"] == 32 and st["main_kernel_ms"] > 0 and st["main_kernel_launches"] == 1, st
    both_forms(ix, Q, OFF, 10, dT, None, keys, "chunk boundary table")
    ix.set_groups(np.full(3000, -3, np.int64))   # one group holds the whole table: 12 chunks per quad of vectors
    want = both_forms(ix, Q, OFF, 4, dT, None, np.full(3000, -3, np.int64), "one group")
    assert (want[2] == [1, 1, 0, 1, 1, 1]).all()
    got = ix.search_multi((Q, OFF), 3, cand_keys=np.array([5, 6, -4], np.int64))   # unknown keys only
    assert (got[0] == 0).all() and np.isposinf(got[1]).all() and (got[2] == 0).all() and (got[3] == -1).all() and np.isposinf(got[4]).all()
    assert ix.stats()["dist_evals"] == 0
    got = ix.search_multi((Q, OFF), 3, cand_keys=np.zeros(0, np.int64))   # an empty list is a list: no group
    assert (got[2] == 0).all() and (got[3] == -1).all()
    ix.set_groups(table4[4])


# ---- 4. scratch_bytes: three passes in each form, and the refusal one byte below a bag's table
def test_scratch_bytes_forces_passes_and_refuses_a_bag_that_does_not_fit(table4):
    ix, X, Q, dT, keys = table4
    reset(ix)
    G = len(np.unique(keys))
    want = mr.numpy_multi(dT, None, keys, OFF, 10)
    # 9 x G x 8 holds 9 vectors' rows of the table: the bags of 1, 3, 0 and 4, then the bag of 5, then the bag of 9 - three passes
    mr.same(ix.search_multi((Q, OFF), 10, scratch_bytes=9 * G * 8), want, "three passes, whole table")
    st = ix.stats()
    assert st["dist_evals"] == T * len(X) and st["main_kernel_queries"] == T, st
    every = np.unique(keys)
    mr.same(ix.search_multi((Q, OFF), 10, cand_keys=every, scratch_bytes=9 * G * 8), want, "three passes, candidates")
    for kw in (dict(), dict(cand_keys=every)):
        with pytest.raises(EpsillaError) as e:
            ix.search_multi((Q, OFF), 10, scratch_bytes=9 * G * 8 - 1, **kw)
        assert e.value.code == 50002 and str(9 * G * 8) in str(e.value), str(e.value)
        mr.same(ix.search_multi((Q, OFF), 10, **kw), want, "after the refusal")
    assert ix.search_multi((Q[:4], mr.bag_offsets([1, 3])), 10, scratch_bytes=3 * G * 8)[2].tolist() == [10, 10]   # (the cap binds the largest bag only)


# ---- 5. visibility
ROW8 = np.dtype([("a", np.int32), ("x", np.float32)])


def test_deleted_minimum_rows_and_an_invisible_group(table4):
    ix, X, Q, dT, keys = table4
    reset(ix)
    free = mr.numpy_multi(dT, None, keys, OFF, 10)
    hidden = np.zeros(len(X), bool)
    hidden[free[3][free[3] >= 0]] = True          # every row that matched a vector in the free answer: the groups' next rows take over
    hidden[keys == free[0][5, 0]] = True          # ... and the best group of the last bag altogether
    ix.set_deleted(packbits(hidden))
    vis = np.broadcast_to(~hidden, dT.shape)
    want = both_forms(ix, Q, OFF, 10, dT, vis, keys, "deleted")
    assert not (want[0] == free[0][5, 0]).any() and not np.isin(want[3], np.flatnonzero(hidden)).any()
    reset(ix)


def test_int_column_program_on_distance_and_id_map(table4):
    ix, X, Q, dT, keys = table4
    reset(ix)
    n = len(X)
    rng = np.random.default_rng(3)
    col = rng.integers(-100, 100, n).astype(np.int32)
    ix.set_int_filter(col, "<", 13)
    vis = np.broadcast_to(sr.visible_rows(n, int_filter=(col, "<", 13)), dT.shape)
    both_forms(ix, Q, OFF, 10, dT, vis, keys, "int column")
    rows = np.zeros(n, ROW8)
    rows["a"] = rng.integers(-100, 100, n)
    rows["x"] = rng.random(n, dtype=F)
    t = float(np.sort(dT, axis=1)[:, 600].min())   # an integer some row's distance EQUALS: `<=` keeps it
    assert (dT == F(t)).any()
    prog = [("dist",), ("const", t), ("<=",), ("i32", 0), ("const", 60), ("<",), ("and",)]
    ix.set_filter_program(prog, rows)
    vis = np.stack([sr.visible_rows(n, program=prog, rows=rows, dist=dT[u].astype(np.float64)) for u in range(T)])
    ix.set_id_map(3, 8)
    G = len(np.unique(keys))
    want = mr.numpy_multi(dT, vis, keys, OFF, 1024)
    got = ix.search_multi((Q, OFF), 1024)
    mr.same(got, want[:3] + (np.where(want[3] >= 0, want[3] * 8 + 3, -1), want[4]), "program on @distance, id map")
    every = np.unique(keys)
    mr.same(ix.search_multi((Q, OFF), 1024, cand_keys=every), got, "program on @distance, id map, candidates")
    q = want[2][[0, 1, 3, 4, 5]]
    assert len(set(q.tolist())) > 1 and (q > 0).all() and (q < G).all(), q   # groups qualify for one bag and not for another
    assert (want[4][np.isfinite(want[4])] <= F(t)).all()
    reset(ix)


def test_nan_rows_and_equal_scores():
    n, d = 300, 8
    X, Q, d32 = gr.ties_table(0, n, d, T, seed=8)
    X, dT = X.copy(), np.ascontiguousarray(d32.T).copy()
    keys = (np.arange(n, dtype=np.int64) // 6) * 5 - 100
    nan_rows = [0, 1, 2, 3, 4, 5, 17, 40]   # group -100 entirely NaN, rows of two other groups
    X[nan_rows, 0] = np.nan
    dT[:, nan_rows] = np.nan
    ix = index(X, 0, keys)
    for k in (7, 50, 64):
        want = both_forms(ix, Q, OFF, k, dT, None, keys, "NaN rows k %d" % k)
    assert (want[2][[0, 1, 3, 4, 5]] == 50).all() and (want[0][[0, 1, 3, 4, 5], 49] == -100).all() and np.isnan(want[1][[0, 1, 3, 4, 5], 49]).all()
    ix.close()
    # equal scores across groups: four distances, many identical rows; the smaller key goes first
    X = np.zeros((512, d), F)
    X[:, 0] = np.arange(512) % 4
    Qz = np.zeros((T, d), F)
    Qz[::2, 0] = 3
    keys = np.random.default_rng(2).integers(0, 40, 512).astype(np.int64) * -3
    dT = np.ascontiguousarray(gr.assert_ties_table(X, Qz, 0).T)
    ix = index(X, 0, keys)
    for k in (1, 7, 40):
        want = both_forms(ix, Qz, OFF, k, dT, None, keys, "equal scores k %d" % k)
    tied = np.flatnonzero(np.diff(want[1][5]) == 0)
    assert len(tied) > 10 and (np.diff(want[0][5])[tied] > 0).all()   # many groups share a score: inside a run the keys ascend
    ix.close()


# ---- 6. buffers and stream order
def shapes(nq, k, t_all):
    return (((nq, k), np.int64), ((nq, k), F), ((nq,), np.int32), ((k * t_all,), np.int64), ((k * t_all,), F))


def test_device_and_host_buffers(table4):
    import torch
    ix, X, Q, dT, keys = table4
    reset(ix)
    nq, k = len(SIZES), 10
    want = mr.numpy_multi(dT, None, keys, OFF, k)
    cand = np.unique(keys)[:40]
    want_c = mr.numpy_multi(dT, None, keys, OFF, k, cand)
    bags = [Q[OFF[j]:OFF[j + 1]] for j in range(nq)]
    mr.same(ix.search_multi(bags, k), want, "a sequence of bags")
    for kw, w in ((dict(), want), (dict(cand_keys=cand), want_c)):
        got = ix.search_multi((Q, OFF), k, **kw)
        assert all(isinstance(a, np.ndarray) for a in got)
        dq = torch.from_numpy(Q).cuda()
        dkw = {name: torch.from_numpy(v).cuda() for name, v in kw.items()}
        torch.cuda.synchronize()
        out = ix.search_multi((dq, OFF), k, **dkw)
        assert all(hasattr(t, "data_ptr") for t in out)
        ix.synchronize()
        mr.same([t.cpu().numpy() for t in out], w, "device")
        mine = tuple(np.full(s, -7, t) for s, t in shapes(nq, k, T))
        out = ix.search_multi((Q, OFF), k, out=mine, **kw)
        assert out[0] is mine[0]
        mr.same(out, w, "out= host")
        dmine = tuple(torch.full(s, -7, dtype=getattr(torch, np.dtype(t).name), device="cuda") for s, t in shapes(nq, k, T))
        torch.cuda.synchronize()
        out = ix.search_multi((Q, OFF), k, out=dmine, **kw)   # host vectors, device results
        ix.synchronize()
        mr.same([t.cpu().numpy() for t in out], w, "host in, device out")
        for j in range(nq):
            assert np.array_equal(amd.index.multi_matches(got[3], OFF, k, j), mr.matches(w[3], OFF, k, j))
    p = lambda a: a.ctypes.data   # noqa: E731
    mine = tuple(np.full(s, -7, t) for s, t in shapes(nq, k, T))
    assert ix.L.eps_index_search_multi(ix.h, p(Q), p(OFF), nq, None, None, 0, k, 0, p(mine[0]), p(mine[1]), None, None, None) == 0   # counts, matches: NULL
    mr.same(mine[:2] + want[2:], want, "no counts, no matches")
    assert all((mine[i] == -7).all() for i in (2, 3, 4))
    dmine = tuple(torch.full(s, -7, dtype=getattr(torch, np.dtype(t).name), device="cuda") for s, t in shapes(nq, k, T))
    torch.cuda.synchronize()
    assert ix.L.eps_index_search_multi(ix.h, p(Q), p(OFF), nq, p(cand), None, len(cand), k, 0, dmine[0].data_ptr(), dmine[1].data_ptr(), None, None, None) == 0
    ix.synchronize()
    mr.same([t.cpu().numpy() for t in dmine[:2]] + list(want_c[2:]), want_c, "device, no counts, no matches")
    assert all((dmine[i] == -7).all().item() for i in (2, 3, 4))


def decoys(X, keys, k, cand):
    decoy = er.make(gr.TIES[0], len(X), X.shape[1], T, seed=404)[1]
    want_decoy = mr.numpy_multi(np.ascontiguousarray(gr.assert_ties_table(X, decoy, 0).T), None, keys, OFF, k, cand)
    return decoy, want_decoy


@pytest.mark.parametrize("form", ["whole table", "candidates"])
def test_host_arrays_are_consumed_when_the_call_returns(table4, form):
    """device outputs, a gate in front; straight after the call returns the page-locked vectors, bag offsets and candidate keys are overwritten from
    the host: a copy still pending then would take the decoys"""
    import torch
    ix, X, Q, dT, keys = table4
    reset(ix)
    nq, k = len(SIZES), 10
    cand = np.unique(keys)[::2].copy() if form == "candidates" else None
    decoy, want_decoy = decoys(X, keys, k, cand)
    want = mr.numpy_multi(dT, None, keys, OFF, k, cand)
    bags = [j for j in range(nq) if SIZES[j]]
    sg.differ_first(want[3][k * OFF[bags]], want_decoy[3][k * OFF[bags]], "search_multi host vectors")
    make_outs = lambda: tuple(torch.full(s, sg.FILL, dtype=getattr(torch, np.dtype(t).name), device="cuda") for s, t in shapes(nq, k, T))   # noqa: E731
    s = torch.cuda.Stream()
    sg.calibrate()
    ix.search_multi((Q, OFF), k, cand_keys=cand)   # (the rows by group are built: a set-up step, with its sync)
    ix.set_stream(s.cuda_stream)
    try:
        host, hoff = sg.pinned(Q.shape, Q.dtype), sg.pinned(OFF.shape, OFF.dtype)
        hcand = sg.pinned(cand.shape, cand.dtype) if cand is not None else None

        def issue(outs=None):
            host[...], hoff[...] = Q, OFF
            if hcand is not None:
                hcand[...] = cand
            ix.search_multi((host, hoff), k, cand_keys=hcand, out=outs or make_outs())
            host[...] = decoy
            hoff[...] = np.arange(nq + 1)   # (other bags)
            if hcand is not None:
                hcand[...] = 123456789      # (no group)
        ms = sg.gate_for("search_multi %s, page-locked host arrays" % form, issue, s)
        outs = make_outs()
        torch.cuda.synchronize()
        sg.gate(s, ms)
        issue(outs)
        s.synchronize()
        mr.same([t.cpu().numpy() for t in outs], want, "a host array was read after the call returned")
    finally:
        ix.set_stream(None)


@pytest.mark.parametrize("form", ["whole table", "candidates"])
def test_device_inputs_on_a_callers_stream_keep_their_place(table4, form):
    """the vectors (and the candidate keys) are valid only at the call's place in the stream: decoys before the gate, the real ones behind it, decoys
    again after the call.  Neither form waits for the device, so the call returns while the gate is still running"""
    import torch
    ix, X, Q, dT, keys = table4
    reset(ix)
    nq, k = len(SIZES), 10
    cand = np.unique(keys)[::2].copy() if form == "candidates" else None
    decoy, want_decoy = decoys(X, keys, k, cand)
    want = mr.numpy_multi(dT, None, keys, OFF, k, cand)
    bags = [j for j in range(nq) if SIZES[j]]
    sg.differ_first(want[3][k * OFF[bags]], want_decoy[3][k * OFF[bags]], "search_multi device vectors")
    make_outs = lambda: tuple(torch.full(s, sg.FILL, dtype=getattr(torch, np.dtype(t).name), device="cuda") for s, t in shapes(nq, k, T))   # noqa: E731
    s = torch.cuda.Stream()
    sg.calibrate()
    ix.search_multi((Q, OFF), k, cand_keys=cand)   # (the rows by group are built)
    ix.set_stream(s.cuda_stream)
    try:
        dq, real, dec = (torch.from_numpy(a).cuda() for a in (decoy, Q, decoy))
        dst, reals, decs = [dq], [real], [dec]
        dc = None
        if cand is not None:
            dc, rc, xc = (torch.from_numpy(a).cuda() for a in (np.full_like(cand, 123456789), cand, np.full_like(cand, 123456789)))
            dst, reals, decs = [dq, dc], [real, rc], [dec, xc]
        torch.cuda.synchronize()
        ms = sg.gate_for("search_multi %s, device inputs" % form, lambda: ix.search_multi((dq, OFF), k, cand_keys=dc, out=make_outs()), s)
        outs = make_outs()
        torch.cuda.synchronize()
        with sg.window(s, dst, reals, decs, ms) as w:
            ix.search_multi((dq, OFF), k, cand_keys=dc, out=outs)
            w.returned(*outs)
        s.synchronize()
        assert w.behind, "the call returned only after the gate (%.1f ms) had run: it waited for the device" % ms
        mr.same(w.numpy(), want, "the call read an input outside its place in the stream")
    finally:
        ix.set_stream(None)


# ---- 7. no trace
def test_search_multi_leaves_no_trace(table4):
    ix, X, Q, dT, keys = table4
    reset(ix)
    cand = np.arange(0, len(X), 3, dtype=np.int64)
    calls = (lambda: ix.search(Q[:5], 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM), lambda: ix.search_groups(Q[:5], 10),
             lambda: ix.search_groups(Q[:5], 130, engine="scan"), lambda: ix.search_group_rows(Q[:5], 10, 4), lambda: ix.search_among(Q[:5], cand, 10))
    before = [c() for c in calls]
    info = ix.groups_info()
    ix.search_multi((Q, OFF), 10)
    ix.search_multi((Q, OFF), 200, cand_keys=np.unique(keys)[:100])
    assert ix.groups_info() == info
    for b, c in zip(before, calls):
        for x, y in zip(b, c()):
            assert np.array_equal(x, y, equal_nan=True)
    assert ix.groups_info() == info
    keys2 = gr.layouts(len(X), seed=9)["zipf"]   # new keys: the rows by group follow them
    ix.set_groups(keys2)
    both_forms(ix, Q, OFF, 10, dT, None, keys2, "new keys")
    ix.set_groups(keys)


# ---- 8. refusals: each gives its error code and leaves the handle usable
def test_refusals(table4):
    import torch
    ix, X, Q, dT, keys = table4
    reset(ix)
    nq, k = len(SIZES), 10
    want = mr.numpy_multi(dT, None, keys, OFF, k)
    p = lambda a: a.ctypes.data   # noqa: E731
    h = [np.empty(s, t) for s, t in shapes(nq, k, T)]
    cand = np.unique(keys)[:5].copy()

    def call(vectors=p(Q), off=p(OFF), n=nq, ck=None, co=None, nc=0, kk=k, scratch=0, outs=None):
        o = [p(a) for a in h] if outs is None else outs
        return ix.L.eps_index_search_multi(ix.h, vectors, off, n, ck, co, nc, kk, scratch, *o), ix.L.eps_index_last_error(ix.h).decode()

    assert call()[0] == 0
    bad = [np.array(v, np.int64) for v in ([1, 1, 1, 1, 1, 1, 1], [0, 5, 4, 9, 9, 9, 22], [0, 1025, 1025, 1025, 1025, 1025, 1025], [0, 1, 2, 3, 4, 5, 4],
                                          [0, 1, 2, 3, 4, 5, 6])]   # (kept alive: the calls below read them through raw pointers)
    for kw, text in ((dict(kk=0), "k must be"), (dict(kk=1025), "k must be"), (dict(n=-1), "nq"), (dict(scratch=-1), "scratch_bytes"),
                     (dict(ck=p(cand), nc=-1), "n_cand"), (dict(vectors=None), "null buffer"), (dict(off=None), "null buffer"),
                     (dict(outs=[None] + [p(a) for a in h[1:]]), "null buffer"), (dict(outs=[p(h[0]), None] + [p(a) for a in h[2:]]), "null buffer"),
                     (dict(outs=[p(a) for a in h[:3]] + [p(h[3]), None]), "null buffer"),   # one match array without the other
                     (dict(co=p(OFF)), "null buffer"),                                      # offsets of a list without its keys
                     (dict(off=p(bad[0])), "q_offsets[0]"),
                     (dict(off=p(bad[1])), "non-decreasing"),
                     (dict(off=p(bad[2])), "1024 vectors"),
                     (dict(ck=p(cand), nc=5, co=p(bad[3])), "cand_offsets"),
                     (dict(ck=p(cand), nc=5, co=p(bad[4])), "cand_offsets")):
        rc, msg = call(**kw)
        assert rc == 30000 and text in msg, (kw, rc, msg)
    dev = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    doff = torch.from_numpy(OFF).cuda()
    rc, msg = call(outs=[dev.data_ptr()] + [p(a) for a in h[1:]])
    assert rc == 30000 and "host or all be device" in msg
    assert call(off=doff.data_ptr())[0] == 30000 and call(ck=p(cand), nc=5, co=doff.data_ptr())[0] == 30000   # offsets are host arrays
    with pytest.raises(ValueError):
        ix.search_multi((Q, OFF), k, out=(dev,) + tuple(h[1:]))
    assert ix.L.eps_index_search_multi(ix.h, None, None, 0, None, None, 0, k, 0, None, None, None, None, None) == 0   # nq = 0
    mr.same(ix.search_multi((Q, OFF), k), want, "after the refusals")
    ix.set_groups(None)   # no groups set
    with pytest.raises(EpsillaError) as e:
        ix.search_multi((Q, OFF), k)
    assert e.value.code == 30000 and "no groups" in str(e.value)
    ix.set_groups(keys)
    # stale labels after an append; stale filters
    ix2 = index(X[:100], 0, keys[:100])
    assert ix2.search_multi((Q, OFF), 3)[2].tolist() == [3, 3, 0, 3, 3, 3]
    ix2.set_deleted(packbits(np.arange(100) == 7))   # (a bitset with a bit set: an empty one is no filter)
    ix2.append_rows(np.zeros((8, X.shape[1]), F))
    for kw in (dict(), dict(cand_keys=cand)):
        with pytest.raises(EpsillaError) as e:
            ix2.search_multi((Q, OFF), 3, **kw)
        assert e.value.code == 30000 and "set_groups" in str(e.value)
    ix2.set_groups(np.concatenate([keys[:100], keys[:8]]))
    with pytest.raises(EpsillaError) as e:
        ix2.search_multi((Q, OFF), 3)
    assert e.value.code == 30000 and "set_deleted" in str(e.value)
    ix2.close()
    # a sharded handle
    sh = amd.GpuIndex(X.shape[1], "EUCLIDEAN", devices=[0, 0])
    sh.attach_rows(np.zeros((300, X.shape[1]), F))
    with pytest.raises(EpsillaError) as e:
        sh.search_multi((Q, OFF), k)
    assert e.value.code == 50002 and "shard" in str(e.value)
    sh.search(Q[:3], 3, mode=amd.MODE_FLAT)
    sh.close()
    # an index without rows: no group
    empty = amd.GpuIndex(X.shape[1], "EUCLIDEAN", device=0)
    empty.set_groups(np.zeros(0, np.int64))
    for kw in (dict(), dict(cand_keys=cand)):
        got = empty.search_multi((Q, OFF), 4, **kw)
        assert (got[0] == 0).all() and np.isposinf(got[1]).all() and (got[2] == 0).all() and (got[3] == -1).all() and np.isposinf(got[4]).all()
    empty.close()
