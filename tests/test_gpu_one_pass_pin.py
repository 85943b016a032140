"""What ONE pass of the one-pass search leaves behind on the DEVICE - every wavefront's list, the table, the threshold the re-rank's selection
reads from it - held to the integer reference of tests/one_pass_ref.py, form by form (GpuIndex.one_pass_probe: eps_index_one_pass_probe, and
GpuIndex.mirror_view of the same index and batch).  Nothing here compares the final answer with another engine: (a) every entry carries the
accumulator its operands give, (b) every slot of the table holds the offer of a visible, unforced row of that slot and kth is the slot of rank
k - 1, (e) T_final is the restated threshold of kth, (c) every row at or above T_final is listed, (d) so is every row that is certainly among the k
closest in fp64.  Every property holds for any interleaving of the wavefronts: one probe per case.

65 573 rows: the smallest table the entry rule admits (>= 65 536), not a multiple of 16 (the r < n clamps, the start values' vector load into the
padding, a partial last block), and every wavefront sees its start-up chunk and at least one chunk under refreshed thresholds.  On the U[0,1)
tables no list may overflow (the suite asserts one_pass == 1 on such tables elsewhere): a case that meets an overflow there fails - but for the one
query whose threshold admits the whole table, where the counts are held to an equality instead (no_overflow_but_the_unavoidable).

The log has one line per case: the instantiation, wavefronts, raw entries, rows at or above T_final, slots filled, the device's T_final against the
restated one.  Seen on the MI355X: one_pass_ref.OBSERVED."""
import numpy as np
import pytest

import exact_ref as er
import one_pass_ref as opr
import select_ref as sr
from test_gpu_mirror_pin import forced_row_table, make_queries, open_index

pytestmark = pytest.mark.gpu
F = np.float32
N = 65_573
PIECES = {100: 2, 520: 3, 1000: 4}


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


_TABLES = {}


@pytest.fixture(scope="module")
def tables(amd):
    """one table per (row width, metric), 32 queries and their fp64 reference: built on first use, shared by every case"""
    def get(d, metric):
        if (d, metric) not in _TABLES:
            rng = np.random.default_rng(1000 * metric + d)
            X = rng.random((N, d), dtype=F)
            if metric == 1:
                X = er.unit(X)
            Q = make_queries(rng, X, 32, metric)
            _TABLES[d, metric] = (open_index(amd, X, metric), X, Q, er.Ref(X, Q, metric))
        return _TABLES[d, metric]
    yield get
    for ix, _, _, _ in _TABLES.values():
        ix.close()
    _TABLES.clear()


def expected_form(d_pad, nq, k, clean=False):
    """the instantiation a call of this shape must run (one_pass.hip launch_pass), restated"""
    slots = 64 if k <= 16 else 128
    matrix = nq > 4 or (slots == 128 and nq > 2)
    return dict(pieces=d_pad // 256, matrix=int(matrix), width=(2 if nq > 16 else 1) if matrix else (4 if nq > 2 else nq), wide=int(slots == 128 and nq <= 2),
                prep_in_kernel=int(clean), slots=slots)


def kernel_name(f):
    return ("stream8m_kernel", f["pieces"], f["width"]) if f["matrix"] else ("stream8_kernel", f["pieces"], f["width"], bool(f["prep_in_kernel"]), bool(f["wide"]))


def pinned(amd, ix, Q, k, visible=None, ref=None, uniform=True, **expect):
    """one probe, one view, (a)-(e), one line in the log; returns (view, probe, figures)"""
    probe = ix.one_pass_probe(Q, k)
    v = ix.mirror_view(8, Q)
    v["Q"] = Q
    form = probe["form"]
    want = dict(expected_form(v["d_pad"], len(Q), k, expect.pop("clean", False)), fold=v["fold"], rot=v["rot"], **expect)
    got = {name: form[name] for name in want}
    assert got == want, (got, want)
    assert form["wave_cap"] == 32 and form["chunk"] == (8 if form["pieces"] == 4 and not form["matrix"] else 16) and 0 < form["waves"] <= 8192, form
    # the queries' constants: the prep launch's in both - or, in the clean form, workgroup 0's of the pass against the prep launch's, bit for bit
    assert np.array_equal(probe["qstat"].view(np.uint32), v["qstat"].view(np.uint32)), "qstat as the pass used it differs from query_prep8_kernel's: %s vs %s" % (
        probe["qstat"].tolist(), v["qstat"].tolist())
    acc = opr.accumulators(v, probe)
    fig = opr.check_all(v, probe, visible, ref, acc=acc)
    print(opr.describe(probe, fig))
    if uniform:
        no_overflow_but_the_unavoidable(v, probe, acc)
    return v, probe, fig


def no_overflow_but_the_unavoidable(v, probe, acc):
    """The condition on the U[0,1) tables: no (query, wavefront) list overflows.  One query of make_queries cannot meet it as stated: the one far
    outside the grid (40 x - 7: every code clamped, a residual norm of ~150 in the margin) gets a threshold some 67 000 000 units below every
    accumulator of the table, EVERY row reaches T_final, and at 65 573 rows the wavefronts 0-2 own a third chunk - 48, 48 and 37 rows for a
    list of 32 (a search of such a batch reports the overflow and the staged chain answers it: the form's design, not a fault of the pass).
    So the condition is held exactly where it can hold and replaced by an equality where it cannot:
      a query whose T_final leaves any row out     no list of it overflows (the issue's condition, unchanged);
      a query whose T_final admits every row       whatever the timing, every wavefront counts exactly the rows it owns, and exactly the
                                                   wavefronts that own more than 32 rows overflow."""
    form, n = probe["form"], v["n"]
    ovf = opr.overflowed(probe)
    owned = np.bincount(opr.wave_of(np.arange(n), form), minlength=form["waves"])
    for q in range(acc.shape[1]):
        if (acc[:, q] >= int(probe["T_final"][q])).all():
            assert np.array_equal(probe["raw_cnt"][q], owned), "query %d: every row reaches T_final %d, wavefront %d counts %d of its %d rows" % (
                q, probe["T_final"][q], np.flatnonzero(probe["raw_cnt"][q] != owned)[0], probe["raw_cnt"][q][probe["raw_cnt"][q] != owned][0], owned[probe["raw_cnt"][q] != owned][0])
            assert np.array_equal(ovf[q], owned > form["wave_cap"])
        else:
            assert not ovf[q].any(), "query %d: %d lists overflowed on a U[0,1) table (T_final %d, %d rows reach it): wavefronts %s count %s" % (
                q, ovf[q].sum(), probe["T_final"][q], (acc[:, q] >= int(probe["T_final"][q])).sum(), np.flatnonzero(ovf[q])[:4].tolist(), probe["raw_cnt"][q][ovf[q]][:4].tolist())


def one_pass_search(amd, ix, Q, k):
    r = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_MFMA_I8)
    st = ix.stats()
    assert st["one_pass"] == 1 and st["main_kernel_bits"] == 8, st
    return r, st


# ------------------------------------------------------------------------------------------------ every instantiation
# (nq, k, clean): 1-2 queries behind the prep launch and - right after a one-pass search - quantised by the pass; 3-4 queries; the 128-slot table
# on v_dot4; one 16-query column block on the matrix cores; two blocks (4 pieces: both blocks' operands in LDS)
SHAPES = ([(1, 10, False), (2, 10, False), (1, 10, True), (2, 10, True), (3, 16, False), (4, 16, False)] +
          [(nq, k, False) for nq in (1, 2) for k in (17, 64)] + [(3, 17, False)] + [(nq, k, False) for nq in (5, 9, 16) for k in (1, 16, 64)] +
          [(nq, k, False) for nq in (17, 32) for k in (10, 64)])
# COSINE and DOT_PRODUCT on the 3-piece table: every kernel family once
# (the clean form: DOT_PRODUCT only - on unit rows of U[0,1), all within a narrow cone, the bound passes every row, a SEARCH overflows and leaves no clean state)
OTHER_METRICS = [(1, 10, False), (2, 10, None), (4, 16, False), (1, 64, False), (2, 17, False), (3, 17, False), (9, 16, False), (16, 64, False), (17, 10, False), (32, 64, False)]
CASES = ([(d, 0, nq, k, clean) for d in sorted(PIECES) for nq, k, clean in SHAPES] +
         [(520, metric, nq, k, metric == 2 if clean is None else clean) for metric in (1, 2) for nq, k, clean in OTHER_METRICS])


def test_the_cases_cover_all_27_instantiations():
    for metric in (0, 1, 2):
        seen = {kernel_name(expected_form(256 * PIECES[d], nq, k, clean)) for d, m, nq, k, clean in CASES if m == metric}
        dot4 = {s for s in seen if s[0] == "stream8_kernel"}
        matrix = {s for s in seen if s[0] == "stream8m_kernel"}
        if metric == 0:
            # stream8_kernel<P, 1|2, PREP>, <P, 1|2, false>, <P, 4, false>, <P, 1|2, false, WIDE>; stream8m_kernel<P, 1>, <P, 2>; P = 2, 3, 4
            assert len(dot4) == 21 and len(matrix) == 6 and {s[1] for s in seen} == {2, 3, 4}, sorted(seen)
        else:
            assert len(dot4) >= 5 and len(matrix) == 2, sorted(seen)


@pytest.mark.parametrize("d,metric,nq,k,clean", CASES)
def test_the_pass_form_by_form(amd, tables, d, metric, nq, k, clean):
    ix, X, Q, ref = tables(d, metric)
    if clean:   # the state a one-pass search of 1-2 queries leaves - of two queries near rows: a batch with the one far outside the grid overflows and is
        one_pass_search(amd, ix, Q[[0, 3][:nq]], k)   # answered by the staged chain -: the next call's pass quantises its queries itself
    pinned(amd, ix, Q[:nq], k, ref=ref.take(slice(0, nq)), uniform=metric != 1, clean=clean, masked=0)   # (unit rows are not U[0,1): see OTHER_METRICS)


# ------------------------------------------------------------------------------------------------ filters
def test_filters(amd, tables):
    ix, X, Q, ref = tables(100, 0)
    rng = np.random.default_rng(3)
    k = 10
    try:
        for nq in (2, 5):
            r4 = ref.take(slice(0, nq))
            for hide in (0.5, 0.9):
                hidden = rng.random(N) < hide
                ix.set_deleted(np.packbits(hidden, bitorder="little"))
                pinned(amd, ix, Q[:nq], k, visible=~hidden, ref=r4, masked=0)
            ix.set_deleted(None)
            col = (np.arange(N) % 7).astype(np.int32)
            ix.set_int_filter(col, "<", 3)
            pinned(amd, ix, Q[:nq], k, visible=sr.visible_rows(N, int_filter=(col, "<", 3)), ref=r4, masked=0)
            ix.set_int_filter(None, None, 0)
            # a compiled program through the mask launch, under a deleted bitset
            rows = ((np.arange(N) * 7919) % 1000).astype(np.int32).reshape(N, 1)
            program = [("i32", 0), ("const", 3), ("%",), ("const", 0), ("=",)]
            hidden = rng.random(N) < 0.3
            bits = np.packbits(hidden, bitorder="little")
            ix.set_deleted(bits)
            ix.set_filter_program(program, rows.view(np.uint8).reshape(N, 4))
            vis = sr.visible_rows(N, deleted=bits, program=program, rows=rows.view(np.uint8).reshape(N, 4))
            assert 0.2 < vis.mean() < 0.3
            pinned(amd, ix, Q[:nq], k, visible=vis, ref=r4, masked=1)
            # ... one that reads @distance: such a search runs the exact stream engine
            ix.set_filter_program([("dist",), ("const", 5.0), ("<",)], rows.view(np.uint8).reshape(N, 4))
            with pytest.raises(amd.EpsillaError) as e:
                ix.one_pass_probe(Q[:nq], k)
            assert e.value.code == 50002
            ix.set_filter_program(None)
            # fewer than k rows visible: the k-th slot stays empty, everything passes - and must be listed (32 rows per wavefront fit its list)
            few = np.zeros(N, bool)
            few[rng.choice(N, 5, replace=False)] = True
            ix.set_deleted(np.packbits(~few, bitorder="little"))
            v, probe, fig = pinned(amd, ix, Q[:nq], k, visible=few, ref=r4, uniform=False, masked=0)
            assert (probe["kth"] == opr.S8_EMPTY).all() and (probe["T_final"] == opr.T_EVERYTHING).all() and fig["filled"] == 5 * nq
            fit = ~opr.overflowed(probe)
            assert fit.any() and fig["entries"] >= int(probe["raw_cnt"][fit].sum()) and fig["at_or_above_T"] == N * nq
            ix.set_deleted(None)
    finally:
        ix.set_deleted(None)
        ix.set_int_filter(None, None, 0)
        ix.set_filter_program(None)


# ------------------------------------------------------------------------------------------------ other tables
def test_a_forced_row_and_a_folding_table(amd):
    rng = np.random.default_rng(21)
    X = forced_row_table(rng, N, 100)
    Q = make_queries(rng, X, 17, 0)
    ix = open_index(amd, X, 0)
    ref = er.Ref(X, Q[:5], 0)
    for nq, k in ((1, 10), (3, 16), (2, 17), (5, 10)):
        v, probe, fig = pinned(amd, ix, Q[:nq], k, ref=ref.take(slice(0, nq)), uniform=False, masked=0)
        assert v["fold"] == 1 and v["forced_rows"] == 1 and probe["form"]["fold"] == 1
        assert opr.listed_mask(probe, N)[N // 3].all(), "the forced row is not in every query's list"
    with pytest.raises(amd.EpsillaError) as e:   # more than 16 queries on a folding table: the staged chain
        ix.one_pass_probe(Q, 10)
    assert e.value.code == 50002
    ix.close()


def test_the_rotated_frame(amd, monkeypatch):
    monkeypatch.setenv("EPS_MIRROR_ROTATE", "1")
    rng = np.random.default_rng(22)
    d = 768
    X = er.embedding_like(rng, N, d)
    Q = er.embedding_like(rng, 5, d)
    ix = open_index(amd, X, 1)
    ref = er.Ref(X, Q, 1)
    ix.search(Q[:1], 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_MFMA_I8)
    for nq, k in ((1, 10), (2, 10), (5, 16)):   # (1-2 queries after a search: the prep launch stays - the transform is its work)
        v, probe, fig = pinned(amd, ix, Q[:nq], k, ref=ref.take(slice(0, nq)), uniform=False, masked=0, clean=False)
        assert v["rot"] == 1 and probe["form"]["rot"] == 1
    ix.close()


def test_a_run_of_identical_rows_in_one_wavefront(amd, tables):
    """40 identical rows in the chunks of ONE wavefront and the query equal to them: ties at the threshold, and that wavefront's list overflows -
    its first 32 entries obey (a), its count is the true one, and no other list overflows"""
    form = tables(100, 0)[0].one_pass_probe(tables(100, 0)[2][:1], 10)["form"]
    W, CH = form["waves"], form["chunk"]
    mine = np.concatenate([np.arange(c * CH, min(N, c * CH + CH)) for c in range(1, (N + CH - 1) // CH, W)])   # the rows of wavefront 1
    assert len(mine) >= 40, (W, CH, len(mine))
    rng = np.random.default_rng(23)
    X = rng.random((N, 100), dtype=F)
    X[mine[:40]] = X[mine[0]]
    Q = X[mine[:1]].copy()
    ix = open_index(amd, X, 0)
    v, probe, fig = pinned(amd, ix, Q, 10, ref=er.Ref(X, Q, 0), uniform=False, masked=0)
    assert probe["form"]["waves"] == W and probe["form"]["chunk"] == CH
    ovf = np.argwhere(opr.overflowed(probe)).tolist()
    assert ovf == [[0, 1]], ovf
    acc = opr.accumulators(v, probe)[:, 0]
    assert (acc[mine[:40]] == acc.max()).all()
    assert 40 <= probe["raw_cnt"][0, 1] <= len(mine), probe["raw_cnt"][0, 1]
    ix.close()


def test_appended_rows(amd):
    rng = np.random.default_rng(24)
    X = rng.random((70_001, 100), dtype=F)
    Q = make_queries(rng, X, 5, 0)
    ix = open_index(amd, X[:N], 0)
    assert ix.mirror_view(8)["n"] == N     # the mirror exists: the append below extends it
    ix.append_rows(X[N:])
    ref = er.Ref(X, Q, 0)
    for nq, k in ((2, 10), (5, 16)):
        v, probe, fig = pinned(amd, ix, Q[:nq], k, ref=ref.take(slice(0, nq)), masked=0)
        assert v["n"] == 70_001 and v["extended_rows"] == 70_001 - N
    ix.close()


# ------------------------------------------------------------------------------------------------ the probe itself
def test_the_probe_leaves_nothing_behind(amd, tables):
    ix, X, Q, ref = tables(520, 0)
    q1 = Q[:1]
    first, _ = one_pass_search(amd, ix, q1, 10)
    again, st0 = one_pass_search(amd, ix, q1, 10)      # (the clean form)
    assert ix.stats() == st0
    probe = ix.one_pass_probe(q1, 10)
    assert probe["form"]["prep_in_kernel"] == 1
    ix.one_pass_probe(Q[:9], 64)
    assert ix.stats() == st0, "a probe changed the statistics of the last search"
    stream = ix.search(q1, 10, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    after = [one_pass_search(amd, ix, q1, 10) for _ in range(2)]     # behind the probe: the prep launch, then the clean form again
    assert ix.one_pass_probe(q1, 10)["form"]["prep_in_kernel"] == 1
    between = one_pass_search(amd, ix, q1, 10)                         # a probe between two clean-form searches
    for r, st in after + [between]:
        assert all(np.array_equal(x, y) for x, y in zip(r, first)) and all(np.array_equal(x, y) for x, y in zip(r, stream))
        assert {key: st[key] for key in ("one_pass", "main_kernel_bits", "rerank_rows", "dist_evals", "overflow_queries", "i8_declined")} == {
            key: st0[key] for key in ("one_pass", "main_kernel_bits", "rerank_rows", "dist_evals", "overflow_queries", "i8_declined")}, (st, st0)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))


def test_the_probe_refuses_what_the_form_does_not_serve(amd, tables):
    ix, X, Q, ref = tables(100, 0)

    def refused(index, q, k):
        with pytest.raises(amd.EpsillaError) as e:
            index.one_pass_probe(q, k)
        assert e.value.code == 50002, e.value
    refused(ix, Q[:1], 65)
    refused(ix, np.concatenate([Q, Q[:1]]), 10)          # 33 queries
    small = open_index(amd, X[:65_535], 0)               # one row short of the entry rule
    refused(small, Q[:1], 10)
    small.close()
    wide = open_index(amd, np.random.default_rng(1).random((65_536, 1025), dtype=F), 0)
    refused(wide, np.zeros((1, 1025), F), 10)
    wide.close()
    grp = amd.GpuIndex(100, 0, devices=[0, 0])
    for s in range(2):
        grp.attach_shard_rows(s, X[s::2])
    refused(grp, Q[:1], 10)
    assert grp.L.eps_index_last_error_class(grp.h) == 0
    grp.close()
    with pytest.raises(amd.EpsillaError) as e:
        ix.one_pass_probe(Q[:1], 0)
    assert e.value.code == 30000
    pinned(amd, ix, Q[:1], 10, ref=ref.take(slice(0, 1)), masked=0)   # ... and the index serves the next probe as before
