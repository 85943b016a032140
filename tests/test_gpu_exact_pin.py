"""The EXACT half of the library - row_dists, make_key / f2ord, WaveTopK + offer, flat_scan_kernel, merge_lists_kernel, rerank_kernel,
s8_rerank_kernel, finalize_kernel, the result pages beyond 1024 - held to the fp64 reference and the contract of tests/exact_ref.py, through
GpuIndex.search alone.  Nothing here compares one engine of the library with another: the stream scan, which every `same(engine, FLAT_STREAM)`
test of the suite measures against, is itself the first thing measured, and every other engine meets the same contract directly.

No tolerance is chosen here.  A distance may differ from its fp64 value by the ORDER-FREE bound (any engine, any rewrite) and, where it comes
from row_dists, by the bound of the DOCUMENTED summation tree; which rows may differ from the true top-k follows from those bounds, and how many
rows that may be is capped from the reference alone BEFORE the device is asked (exact_ref.assert_cap).  Tables of small integers have no band
at all: every distance bit and every id, position by position, with the k-th place inside a group of equal distances.

Every case prints one line (`exact-pin: ...`): the largest observed |d32 - d64| / B for both bounds, the undecided rows, what stats() reported."""
import os

import numpy as np
import pytest

import exact_ref as xr
from helpers import bitset

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


def engines(amd):
    return {"stream": amd.FLAT_STREAM, "mfma": amd.FLAT_MFMA, "mfma_i8": amd.FLAT_MFMA_I8, "auto": amd.FLAT_AUTO}


def held(amd, ix, X, Q, metric, k, ref, name, four=True, exact=False, engine="stream", visible=None, vec4=None, idmap=None, sample=None, tree=True, what="", **kw):
    """one search under the contract.  sample: the queries `ref` was made of (all queries are searched, those are checked)."""
    kw.setdefault("mode", amd.MODE_FLAT)
    if kw["mode"] == amd.MODE_FLAT:
        kw.setdefault("flat_engine", engines(amd)[engine])
    # four: True - check 4 under both bounds; "tree" - under the tree bound only (FREE_BAND_EXEMPT); False - checks 1-3.  The band's cap is a
    # condition on the inputs, asserted before the device is asked
    if four == "tree":
        u = xr.undecided(ref, k, visible, bound="tree", vec4=vec4)
        assert u <= xr.CAP * k * ref.nq, "%s %s k %d: the TREE band leaves %d rows open: change the table" % (name, what, k, u)
    elif four and not exact:
        xr.assert_cap(ref, k, visible, what="%s %s" % (name, what))
    ids, dist, cnt = ix.search(Q, k, **kw)
    st = ix.stats()
    if idmap:
        base, stride = idmap
        live = ids >= 0
        assert ((ids[live] - base) % stride == 0).all(), "%s %s: an id is not base + row x stride" % (name, what)
        ids = np.where(live, (ids - base) // stride, -1)
    if sample is not None:
        ids, dist, cnt = ids[sample], dist[sample], cnt[sample]
    tag = "%s m%d %s %s" % (name, metric, engine, what)
    if exact:
        xr.check_exact(ids, dist, cnt, X, None, metric, k, visible=visible, ref=ref, what=tag)
    und = xr.check_topk(ids, dist, cnt, X, None, metric, k, visible=visible, bound="free", ref=ref, membership=four is True, what=tag)
    if tree:      # (distances that come from row_dists: the documented tree)
        ut = xr.check_topk(ids, dist, cnt, X, None, metric, k, visible=visible, bound="tree", vec4=vec4, ref=ref, membership=bool(four), what=tag)
        und = ut if four == "tree" else und
    rf, rt = xr.error_ratios(ids, dist, cnt, ref, vec4)
    print("exact-pin: %-28s m%d %-7s n %6d d %5d nq %4d k %4d %-22s err/B free %.4f tree %.3f undecided %d of %d  bits %d one_pass %d overflow %d" % (
        name, metric, engine, ref.n, ref.d, len(Q), k, what, rf, rt, und, k * ref.nq, st["main_kernel_bits"], st["one_pass"], st["overflow_queries"]))
    return st


def table(amd, name, metric, n, d, nq, seed):
    X, Q = xr.make(name, n, d, nq, seed=seed)
    ix = amd.GpuIndex(d, metric)
    ix.attach_rows(X)
    return X, Q, ix


# ------------------------------------------------------------------------------------------------ the yardstick itself: FLAT_STREAM
WIDTH_CASES = [("gaussian", 0), ("uniform", 2), ("gaussian x 3 queries", 2), ("embedding-like", 1), ("rows near 100", 0), ("rows near 100", 2),
               ("integers -8..8", 0), ("integers -8..8", 2), ("integers / 16", 1)]


# (table, metric, d) whose ORDER-FREE band cannot be capped: the band grows as d^2 (d terms of a sum of magnitude ~d), the spread of the distances as
# sqrt(d); from d = 4096 on it leaves more than 5 % of k x queries open for every table of continuous values at every row count of the ladder below
# (asserted where it is used, so that the exemption cannot outlive its reason).  These keep check 2 under BOTH bounds and are held to check 4 under the
# TREE bound, whose own band is capped at the same 5 % first.  Exempt by name, as "rows near 100" under DOT_PRODUCT is in exact_ref.TABLES.
FREE_BAND_EXEMPT = {(name, metric, d) for d in (4096, 4100, 8192)
                    for name, metric in (("gaussian", 0), ("uniform", 2), ("gaussian x 3 queries", 2), ("embedding-like", 1), ("rows near 100", 0))}
ROW_LADDER = (None, 2001, 501)      # a table that misses the cap is changed - fewer rows - never the cap (None: the width's full row count)


def capped_table(name, metric, d, n_full, nq, seed):
    """the largest table of the ladder whose order-free band meets the cap at k = 10 and 100, computed from the reference alone -> (X, Q, ref, True);
    none does -> the full table, (X, Q, ref, False)"""
    first = None
    for n in ROW_LADDER:
        X, Q = xr.make(name, n or n_full, d, nq, seed=seed)
        ref = xr.Ref(X, Q, metric)
        first = first or (X, Q, ref)
        if all(xr.undecided(ref, k) <= xr.CAP * k * nq for k in (10, 100)):
            return X, Q, ref, True
    return first + (False,)


@pytest.mark.parametrize("d", [1, 3, 7, 33, 64, 100, 333, 768, 1000, 1536, 4096, 4100, 8192])
def test_stream_scan_at_every_width(amd, d):
    """G = 1 .. 64 lanes per row, the scalar form (d % 4 != 0) and the 16-byte form, one to 32 pieces per lane; d = 4096 is exactly 64 KB of
    staged queries with NQ = 4, d = 4100 and 8192 step pick_nq down (NQ = 4 would not fit).  Every table is held to the whole contract wherever
    its order-free band meets the cap - computed, with fewer rows where the full table misses it; FREE_BAND_EXEMPT says what remains."""
    n = 20_001 if d <= 1536 else (6_001 if d <= 4100 else 3_001)
    nq = 16 if d <= 1536 else 5
    for name, metric in WIDTH_CASES:
        rows, queries, metrics, four, exact = xr.TABLES[name]
        if d == 1 and metric == 1 and not exact:
            continue          # (unit rows of one column are +-1: two distinct cosines, ties everywhere, without being an exact table)
        if exact or metric not in four:
            X, Q = xr.make(name, n, d, nq, seed=100 + d)
            ref, mode = xr.Ref(X, Q, metric), (True if exact else False)
        else:
            X, Q, ref, capped = capped_table(name, metric, d, n, nq, seed=100 + d)
            assert capped != ((name, metric, d) in FREE_BAND_EXEMPT), "%s m%d d %d: FREE_BAND_EXEMPT and the computed cap disagree" % (name, metric, d)
            mode = True if capped else "tree"
        ix = amd.GpuIndex(d, metric)
        ix.attach_rows(X)
        for k in (10, 100):
            held(amd, ix, X, Q, metric, k, ref, name, four=mode, exact=exact)
        ix.close()


def test_widths_the_library_refuses(amd):
    """one query must fit in LDS next to the queues: d > 8192 is refused when the index is made, as a user error"""
    with pytest.raises(amd.EpsillaError) as e:
        amd.GpuIndex(16384, 0)
    assert e.value.code == 30000
    amd.GpuIndex(8192, 0).close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4097, 70_001, 200_003])
def test_stream_scan_at_every_row_count(amd, n):
    """fewer rows than a wavefront's chunk, a last chunk that is not full, more than one block per query group"""
    d = 128
    for name, metric in (("gaussian", 0), ("uniform", 2), ("embedding-like", 1), ("integers -8..8", 0), ("integers / 16", 1)):
        exact = xr.TABLES[name][4]
        X, Q, ix = table(amd, name, metric, n, d, 4, seed=200)
        ref = xr.Ref(X, Q, metric)
        for k in (1, 10, 100):
            held(amd, ix, X, Q, metric, k, ref, name, exact=exact)
        ix.close()


def test_stream_scan_at_every_query_count(amd):
    """NQ = 1, 2, 4 with padded last groups; 2500 queries: the gx_cap regime of flat_scan_waves (4 wavefronts walk the whole table)"""
    n, d = 70_001, 128
    for name, metric in (("gaussian", 0), ("gaussian x 3 queries", 2), ("integers -8..8", 0)):
        exact = xr.TABLES[name][4]
        X, Q, ix = table(amd, name, metric, n, d, 2500, seed=300)
        ref33 = xr.Ref(X, Q[:33], metric)
        for nq in (1, 2, 3, 4, 5, 33):
            ref = ref33.take(slice(0, nq))
            held(amd, ix, X, Q[:nq], metric, 10, ref, name, exact=exact)
        sample = np.arange(0, 2500, 97)
        ref = xr.Ref(X, Q[sample], metric)
        held(amd, ix, X, Q, metric, 10, ref, name, exact=exact, sample=sample, what="(26 of 2500 checked)")
        ix.close()


@pytest.mark.parametrize("nq", [1, 5])
def test_stream_scan_at_every_list_length(amd, nq):
    """KPL = 1, 2, 4, 8, 16 on both sides of each step, with one query and with five (k > 128: one query per group), both widths of
    merge_lists_kernel"""
    n, d = 30_001, 64
    for name, metric in (("uniform", 0), ("gaussian x 3 queries", 2), ("integers -8..8", 0), ("integers / 16", 1)):
        exact = xr.TABLES[name][4]
        X, Q, ix = table(amd, name, metric, n, d, nq, seed=400)
        ref = xr.Ref(X, Q, metric)
        for k in (1, 10, 64, 65, 128, 129, 256, 257, 512, 513, 1024):
            held(amd, ix, X, Q, metric, k, ref, name, exact=exact)
        ix.close()


@pytest.mark.parametrize("metric,name", [(0, "integers -8..8"), (2, "integers -8..8"), (1, "integers / 16")])
def test_result_pages_on_a_table_of_ties(amd, metric, name):
    """beyond 1024 results the scan pages: page p = the best keys ordered after page p - 1's last.  On a table of a few hundred distinct
    distances every page boundary lies inside a group of equal distances: the low word of the key decides"""
    n, d = 5000, 4
    X, Q, ix = table(amd, name, metric, n, d, 3, seed=500)
    ref = xr.Ref(X, Q, metric)
    s = np.sort(ref.d64, axis=0)
    assert all(len(np.unique(ref.d64[:, q])) < 600 for q in range(3)) and (s[1023] == s[1024]).all() and (s[2047] == s[2048]).all()
    for k in (1024, 1025, 2048, 2049, 3000, n + 7):
        for engine in ("stream", "auto"):
            held(amd, ix, X, Q, metric, k, ref, name, exact=True, engine=engine)
    vis = np.ones(n, bool)
    vis[::7] = False
    ix.set_deleted(bitset(n, range(0, n, 7)))
    held(amd, ix, X, Q, metric, 3000, ref, name, exact=True, visible=vis, what="deleted")
    ix.close()


@pytest.mark.parametrize("d", [768, 64])
@pytest.mark.parametrize("metric,name", [(0, "gaussian"), (2, "gaussian x 3 queries"), (0, "integers -8..8")])
def test_rows_attached_4_bytes_off_a_16_byte_boundary(amd, metric, name, d):
    """rows attached from a device tensor whose data pointer is 4 bytes off a 16-byte boundary, d % 4 == 0: a 16-byte load there is misaligned, so
    the library takes the scalar form by alignment.  What this proves: the answers from such a pointer are right - bit for bit on the integer
    table - and every distance is within the tree bound OF THE SCALAR FORM (d = 64: 1 + 6 + 3 roundings against the 16-byte form's 4 + 4 + 3; at
    d = 768 both forms have 21).  Which form ran is not visible through the ABI: that is launch_flat_scan's `vec4` line, not this test."""
    import torch
    n = 40_001
    X, Q = xr.make(name, n, d, 5, seed=600)
    buf = torch.empty(n * d + 4, dtype=torch.float32, device="cuda")
    off = 1 + (-(buf.data_ptr() // 4) % 4)          # first element that is 4 bytes past a 16-byte boundary
    rows = buf[off:off + n * d].view(n, d)
    assert rows.data_ptr() % 16 == 4
    rows.copy_(torch.from_numpy(X))
    ix = amd.GpuIndex(d, metric)
    ix.attach_rows(rows)
    ref = xr.Ref(X, Q, metric)
    for k in (10, 100):
        held(amd, ix, X, Q, metric, k, ref, name, exact=xr.TABLES[name][4], vec4=False, what="misaligned")
    ix.close()


def test_visible_sets_and_id_maps(amd):
    """a deleted bitset (every 11th row; all but 5 rows), an int-column filter, set_id_map with a stride beyond 32 bits"""
    n, d = 50_000, 128
    for name, metric in (("gaussian", 0), ("integers -8..8", 2)):
        exact = xr.TABLES[name][4]
        X, Q, ix = table(amd, name, metric, n, d, 4, seed=700)
        ref = xr.Ref(X, Q, metric)
        ix.set_id_map(3, 2 ** 33)
        held(amd, ix, X, Q, metric, 10, ref, name, exact=exact, idmap=(3, 2 ** 33), what="id map")
        vis = np.ones(n, bool)
        vis[3::11] = False
        ix.set_deleted(bitset(n, range(3, n, 11)))
        for k in (10, 200):
            held(amd, ix, X, Q, metric, k, ref, name, exact=exact, visible=vis, idmap=(3, 2 ** 33), what="deleted")
        col = np.arange(n, dtype=np.int32)[::-1].copy()
        ix.set_int_filter(col, "<", 30_000)
        vis2 = vis & (col < 30_000)
        held(amd, ix, X, Q, metric, 10, ref, name, exact=exact, visible=vis2, idmap=(3, 2 ** 33), what="deleted + filter")
        ix.set_int_filter(None, None, 0)
        keep = np.array([5, 4097, 20_000, 33_333, n - 1])
        vis3 = np.zeros(n, bool)
        vis3[keep] = True
        ix.set_deleted(bitset(n, np.flatnonzero(~vis3)))
        held(amd, ix, X, Q, metric, 10, ref, name, exact=exact, visible=vis3, idmap=(3, 2 ** 33), what="all but 5 deleted")
        ix.close()


@pytest.mark.parametrize("metric,name", [(0, "integers -8..8"), (1, "integers / 16")])
def test_two_row_ranges(amd, metric, name):
    """append_rows after attach_rows on a table of ties: the ids of the second range continue the first, ties across the ranges are in id order"""
    n, d = 30_000, 128
    X, Q = xr.make(name, n, d, 4, seed=800)
    ix = amd.GpuIndex(d, metric)
    ix.attach_rows(X[:17_001])
    ix.append_rows(X[17_001:])
    ref = xr.Ref(X, Q, metric)
    for k in (10, 300):
        held(amd, ix, X, Q, metric, k, ref, name, exact=True, what="two ranges")
    ix.close()


# ------------------------------------------------------------------------------------------------ every other flat engine, directly
ENGINE_CASES = [("uniform", 0), ("gaussian", 0), ("gaussian x 3 queries", 2), ("embedding-like", 1), ("integers -8..8", 0), ("integers / 16", 1)]


@pytest.mark.parametrize("n,d", [(70_001, 768), (100_000, 128)])
@pytest.mark.parametrize("name,metric", ENGINE_CASES)
def test_matrix_engines_meet_the_contract(amd, name, metric, n, d):
    """FLAT_MFMA, FLAT_MFMA_I8, FLAT_AUTO with 40 and 300 queries: their distances come from rerank_kernel (row_dists): both bounds.  On U[0,1)
    and gaussian rows the form that was asked for must have run (as tests/test_gpu_mfma_i8.py requires there); elsewhere the library may
    hand over, and the contract holds whatever ran."""
    exact = xr.TABLES[name][4]
    X, Q, ix = table(amd, name, metric, n, d, 300, seed=900)
    for nq in (40, 300):
        sample = np.arange(0, nq, max(1, nq // 20))[:20]
        ref = xr.Ref(X, Q[sample], metric)
        for k in (10, 100):
            for engine in ("mfma", "mfma_i8", "auto"):
                st = held(amd, ix, X, Q[:nq], metric, k, ref, name, exact=exact, engine=engine, sample=sample, what="(%d checked)" % len(sample))
                if name == "uniform":
                    assert engine != "mfma" or st["main_kernel_bits"] == 16, st
                    assert engine != "mfma_i8" or (st["main_kernel_bits"], st["overflow_queries"]) == (8, 0), st
    ix.close()


@pytest.mark.parametrize("d", [768, 333])
@pytest.mark.parametrize("name,metric", [("uniform", 0), ("gaussian", 0), ("embedding-like", 1), ("integers -8..8", 0), ("integers / 16", 1)])
def test_one_pass_form_meets_the_contract(amd, name, metric, d):
    """up to 32 queries, k <= 64: one pass over the 8-bit mirror, then s8_rerank_kernel (d = 333: its scalar form) - or, with EPS_S8_RERANK=0,
    rerank_kernel behind the selection prologue.  On U[0,1) rows under L2 the one-pass form must have run (tests/test_gpu_mfma_i8.py)."""
    exact = xr.TABLES[name][4]
    n = 70_001
    X, Q, ix = table(amd, name, metric, n, d, 32, seed=1000)
    ref32 = xr.Ref(X, Q, metric)
    for nq in (1, 4, 5, 16, 32):
        ref = ref32.take(slice(0, nq))
        for k in (10, 40, 64):
            for switch in (None, "0"):
                if switch is not None:
                    os.environ["EPS_S8_RERANK"] = switch
                try:
                    st = held(amd, ix, X, Q[:nq], metric, k, ref, name, exact=exact, engine="mfma_i8", what="rerank_kernel" if switch else "s8_rerank_kernel")
                finally:
                    os.environ.pop("EPS_S8_RERANK", None)
                if name == "uniform":
                    assert st["one_pass"] == 1 and (st["main_kernel_bits"], st["overflow_queries"]) == (8, 0), (nq, k, st)
    ix.close()


# ------------------------------------------------------------------------------------------------ graph and sharded results
def test_reference_mode_results_meet_checks_1_to_3(amd):
    """MODE_REFERENCE on the golden graph and on a device-built graph (T = 1 and 4): which rows a traversal reaches is the oracle's business
    (tests/test_gpu_traverse.py); that what comes back is unique, ordered by (distance, id) and carries the distance of the row it names is
    this contract's.  Then rows appended behind the graph: the brute-force tail merged into the result."""
    from helpers import data
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph2000x32.npz"))
    for metric in (0, 1, 2):
        X, Q = data(2000, 32, 42), data(16, 32, 43)
        ix = amd.GpuIndex(32, metric)
        ix.attach_rows(X)
        ix.set_graph(z["off"].astype(np.int64), z["nbr"].astype(np.int64), int(z["nav"]))
        ref = xr.Ref(X, Q, metric)
        for T in (1, 4):
            held(amd, ix, X, Q, metric, 10, ref, "golden graph", four=False, tree=False, engine="graph", mode=amd.MODE_REFERENCE, intra_threads=T, what="T %d" % T)
        ix.close()
    n, d = 20_000, 128
    X, Q = xr.make("gaussian", n + 3000, d, 16, seed=1100)
    ix = amd.GpuIndex(d, 0)
    ix.attach_rows(X[:n])
    ix.build()
    ref = xr.Ref(X[:n], Q, 0)
    for T in (1, 4):
        held(amd, ix, X[:n], Q, 0, 10, ref, "built graph", four=False, tree=False, engine="graph", mode=amd.MODE_REFERENCE, intra_threads=T, what="T %d" % T)
    ix.append_rows(X[n:])
    ref = xr.Ref(X, Q, 0)
    for T in (1, 4):
        held(amd, ix, X, Q, 0, 10, ref, "built graph + tail", four=False, tree=False, engine="graph", mode=amd.MODE_REFERENCE, intra_threads=T, what="T %d" % T)
    ix.close()


@pytest.mark.parametrize("metric,name", [(0, "integers -8..8"), (2, "integers -8..8"), (1, "integers / 16")])
def test_shard_merge_on_a_table_of_ties(amd, metric, name):
    """rows split over two shards (global row = local row x 2 + shard): every tie is between rows of different shards somewhere; the merge
    orders them by GLOBAL id"""
    n, d = 40_001, 128
    X, Q = xr.make(name, n, d, 5, seed=1200)
    ix = amd.GpuIndex(d, metric, devices=[0, 0])
    ix.attach_rows(X)
    ref = xr.Ref(X, Q, metric)
    for k in (10, 100, 1024):
        ids, dist, cnt = ix.search(Q, k, mode=amd.MODE_FLAT)
        xr.check_exact(ids, dist, cnt, X, Q, metric, k, ref=ref, what="two shards k %d" % k)
    ix.close()


# ------------------------------------------------------------------------------------------------ NaN and infinity
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("engine", ["stream", "mfma", "mfma_i8", "auto"])
def test_nan_sorts_last(amd, metric, engine):
    """device_common.hpp: "NaN sorts last".  5000 finite rows, one row holding a NaN, one holding +inf, one holding -inf; query 0 has a zero in
    the column of the infinities (DOT_PRODUCT: inf x 0 = NaN; L2: (inf - 0)^2 = inf), query 1 has 0.5 there (DOT_PRODUCT: -inf and +inf).
    While k finite-distance rows are visible no NaN is returned and the finite part meets the contract; when k reaches them, NaN rows come
    after every finite and infinite distance.  DOT_PRODUCT negates the sum - the sign bit of a NaN with it - so the key's ordinal must not
    depend on a NaN's sign."""
    n, d, col = 5003, 64, 17
    rng = np.random.default_rng(1300)
    X = rng.standard_normal((n, d), dtype=F)
    Q = rng.standard_normal((2, d), dtype=F)
    r_nan, r_pinf, r_ninf = 1234, 2345, 3456
    X[r_nan, 5] = np.nan
    X[r_pinf, col] = np.inf
    X[r_ninf, col] = -np.inf
    Q[0, col], Q[1, col] = 0.0, 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        d64 = xr.dist64(X, Q, metric)
    finite = np.isfinite(d64)
    assert not finite[r_nan].any() and np.isnan(d64[r_nan]).all()
    if metric == 2:
        assert np.isnan(d64[[r_pinf, r_ninf], 0]).all() and d64[r_pinf, 1] == -np.inf and d64[r_ninf, 1] == np.inf
    else:
        assert (d64[[r_pinf, r_ninf]] == np.inf).all()
    ix = amd.GpuIndex(d, metric)
    ix.attach_rows(X)
    Xf = np.where(np.isfinite(X), X, F(0))
    for k in (10, n):
        ids, dist, cnt = ix.search(Q, k, mode=amd.MODE_FLAT, flat_engine=engines(amd)[engine])
        st = ix.stats()
        print("exact-pin: nan/inf m%d %-7s k %4d first rows %s first distances %s bits %d one_pass %d" % (
            metric, engine, k, ids[:, :3].tolist(), dist[:, :3].tolist(), st["main_kernel_bits"], st["one_pass"]))
        for q in range(2):
            m = int(cnt[q])
            got_d, got_i = dist[q, :m], ids[q, :m]
            nans = np.flatnonzero(np.isnan(d64[:, q]))
            infs = np.flatnonzero(d64[:, q] == np.inf)
            ninf = np.flatnonzero(d64[:, q] == -np.inf)
            nan_at = np.flatnonzero(np.isnan(got_d))
            first_nan = int(nan_at[0]) if len(nan_at) else m
            assert m == k, (q, m, k)
            if k == 10:
                assert first_nan == m, "query %d: row %d comes back with a NaN distance at rank %d while %d rows have finite distances" % (
                    q, got_i[first_nan] if first_nan < m else -1, first_nan, int(finite[:, q].sum()))
            else:
                assert np.isnan(got_d[first_nan:]).all(), "query %d: a NaN distance at rank %d (row %d) ahead of a number" % (q, first_nan, got_i[first_nan])
                assert list(got_i[first_nan:]) == list(nans), "query %d: the NaN rows are one group of equal keys at the end, in id order: %s" % (q, got_i[first_nan:][:8])
                assert list(got_i[first_nan - len(infs):first_nan]) == list(infs) and (got_d[first_nan - len(infs):first_nan] == np.inf).all(), "query %d: +inf rows come last of the numbers" % q
            assert list(got_i[:len(ninf)]) == list(ninf) and (got_d[:len(ninf)] == -np.inf).all(), "query %d: -inf rows come first" % q
            # the finite part under the contract: the rows whose fp64 distance is finite, as the visible set
            fin = np.isfinite(got_d)
            kk = min(k - len(ninf), int(finite[:, q].sum()))
            fi, fd = got_i[fin][None, :], got_d[fin][None, :]
            xr.check_topk(fi, fd, np.array([fi.shape[1]]), Xf, None, metric, kk, visible=finite[:, q], ref=xr.Ref(Xf, Q[q:q + 1], metric), bound="tree",
                          what="nan/inf m%d %s q%d k%d" % (metric, engine, q, k))
    ix.close()
