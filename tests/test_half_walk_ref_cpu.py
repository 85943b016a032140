"""half_walk_ref held to what it does not compute itself: its merged lists to np.lexsort over the visible rows, its hit counts to walks short
enough to count by hand and to "every round of an open slice hits", its plan to the literals of half_walk_ref.SHAPES (which
tests/native/half_host_check.cpp holds csrc/half_host.hpp to, under a sanitizer: tests/test_half_host_cpu.py); and, from the model alone, the
premise of tests/test_gpu_half_rounds.py: which of its tables leave rounds off the hit path.  No device."""
import numpy as np
import pytest

import exact_ref as xr
import half_walk_ref as hw
import test_gpu_half_rounds as gr
import test_gpu_half_search as hs


def test_plan_is_the_table_of_shapes():
    for tag, (shape, form, tiles, (slices, rps), sr, seed) in hw.SHAPES.items():
        p = hw.plan(*shape)
        assert ((p["cols"], p["kpl"], p["nb"]), p["tiles"], (p["slices"], p["rows_per_slice"]), p["seed_rows"]) == (form, tiles, (slices, rps), sr), tag
        assert (p["seed"] and (p["seed"]["slices"], p["seed"]["rows_per_slice"])) == seed and hw.seed_rows(shape[0], shape[3]) == sr, tag
        assert rps > 64 and p["rounds"] == -(-shape[0] // 64) * tiles, tag      # the premise of the GPU tests: no shape falls back to one round
    # the shapes of tests/test_gpu_half_search.py, as its issue lists them: 64 rows per slice
    for shape, slices, seed in (((1500, 72, 70, 64), 24, None), ((1500, 72, 70, 1024), 24, None), ((32767, 40, 20, 10), 512, None), ((40000, 40, 20, 10), 628, (64, 64)),
                                ((40000, 40, 20, 100), 628, (64, 64))):
        p = hw.plan(*shape)
        assert (p["slices"], p["rows_per_slice"]) == (slices, 64) and (p["seed"] and (p["seed"]["slices"], p["seed"]["rows_per_slice"])) == seed, shape


def lexsort_top(D, visible, k, opening=None):
    o = hw.ordinal(np.ascontiguousarray(D.T)).astype(np.int64)
    out = []
    for u in range(D.shape[1]):
        rows = np.flatnonzero(visible & (True if opening is None else o[u] < opening[u]))
        out.append(rows[np.lexsort((rows, o[u, rows]))][:k])
    return out


@pytest.mark.parametrize("k", (1, 10, 64, 70, 200))
@pytest.mark.parametrize("bitset", (False, True))
def test_merged_lists_are_the_plain_top_k(k, bitset):
    """tables of ties cut into slices of 4 and of 3 rounds (the last one ragged, one empty), open and under opening bounds"""
    rng = np.random.default_rng([k, bitset])
    for metric, (n, slices, rps) in enumerate(((1000, 4, 256), (700, 5, 192), (130, 4, 64))):
        X, Q = hs.widen(hs.ties(rng, n, 6, metric, "float16"), "float16"), hs.widen(hs.ties(rng, 5, 6, metric, "float16"), "float16")
        D = xr.dist64(X, Q, metric)
        visible = rng.random(n) < 0.5 if bitset else np.ones(n, bool)
        pad = xr.dist64(np.zeros((1, 6), np.float32), Q, metric)[0]
        for opening in (None, hw.ordinal(np.median(D, axis=0)).astype(np.int64) + 1):
            hits, top = hw.walk(D, visible, dict(slices=slices, rows_per_slice=rps, cols=4), k, np.arange(7) % 5, pad, opening)
            want = lexsort_top(D, visible, k, opening)
            for u in range(5):
                m = len(want[u])
                assert np.array_equal(top[u, :m] & np.uint64(0xFFFFFFFF), want[u].astype(np.uint64)) and (top[u, m:] == hw.EMPTY).all()
                assert np.array_equal(hw.ord2f((top[u, :m] >> np.uint64(32)).astype(np.uint32)).astype(np.float64), D[want[u], u])
            assert 0 < hits <= -(-n // 64) * 2


def test_search_is_the_plain_top_k_on_each_side_of_the_seed_rule():
    rng = np.random.default_rng(5)
    for n in (32767, 33000):
        X, Q = hs.widen(hs.ties(rng, n, 6, 0, "float16"), "float16"), hs.widen(hs.ties(rng, 3, 6, 0, "float16"), "float16")
        D, visible = xr.dist64(X, Q, 0), rng.random(n) < 0.5
        m = hw.search(D, visible, 6, 10, np.arange(3), xr.dist64(np.zeros((1, 6), np.float32), Q, 0)[0])
        want = lexsort_top(D, visible, 10)
        assert (m["seed"] is not None) == (n >= 32768) and (m["counts"] == 10).all()
        for u in range(3):
            assert np.array_equal(m["rows"][u], want[u]) and np.array_equal(m["dist"][u].astype(np.float64), D[want[u], u])
        if m["seed"] is not None:   # the seed is one above the prefix's k-th visible distance
            kth = [np.sort(D[:4096][visible[:4096], u])[9] for u in range(3)]
            assert np.array_equal(m["seed"], hw.ordinal(np.array(kth)).astype(np.int64) + 1) and m["seed_hit_rounds"] == 64


def counted(D, k, visible=None, pad=0.0, opening=None, slices=1, cols=1, qmap=(0,)):
    D = np.asarray(D, np.float64)
    D = D[:, None] if D.ndim == 1 else D
    rps = -(-len(D) // (64 * slices)) * 64
    return hw.walk(D, visible, dict(slices=slices, rows_per_slice=rps, cols=cols), k, np.asarray(qmap), np.full(D.shape[1], pad), opening)[0]


def test_walks_short_enough_to_count_by_hand():
    five = [5.0] * 64
    assert counted(five * 3, 1) == 1                                   # open; then only ties with the k-th distance: both end at the vote
    assert counted(five * 2 + [4.0] + five[1:], 1) == 2                # a closer row in the third round
    assert counted(five * 3, 65) == 2                                  # the list fills in the second round: still open there
    assert counted(five + [6.0] * 64 + five, 64) == 1 and counted(five + [6.0] * 64 + five, 65) == 3   # the 65th distance is 6: the third round's 5 passes
    vis = np.ones(192, bool)
    vis[64] = False
    assert counted(five + [4.0] + five[1:] + [4.5] + five[1:], 1, vis) == 3      # a deleted row votes and does not enter: 4.5 still passes
    assert counted(five + [4.0] + five[1:] + [4.5] + five[1:], 1) == 2           # visible, it enters: 4.5 does not
    vis[:64] = False
    assert counted(five * 3, 1, vis) == 2                              # nothing entered in the first round: the second is still open
    assert counted(five * 2 + [5.0], 1, pad=7.0) == 1 and counted(five * 2 + [5.0], 1, pad=4.0) == 2   # the zero rows behind n vote
    assert counted(five * 2 + [5.0], 1, ~np.ones(129, bool), pad=4.0) == 3
    nan = [np.nan] + five[1:]
    assert counted(five + nan + five, 1) == 2 and counted(nan + five + five, 64) == 2   # a NaN always votes; as a k-th distance it lets numbers pass
    assert counted(nan + five + five, 128) == 3 and counted([np.nan] * 64 + five * 2, 1) == 2
    # opening bounds: one above 5 lets the ties of every round pass until the list fills; one above 4 lets nothing pass; a NaN's opens all
    o = lambda d: hw.ordinal(np.array([d])).astype(np.int64) + 1
    assert counted(five * 3, 1, opening=o(5.0)) == 1 and counted(five * 3, 200, opening=o(5.0)) == 3 and counted(five * 3, 1, opening=o(4.0)) == 0
    assert counted(five * 3, 200, opening=o(np.nan)) == 3 and counted(five + [6.0] * 128, 200, opening=o(5.0)) == 1
    # two slices of two rounds, the second slice ragged and its own list; two queries of one tile: a round is hit if either votes; two tiles: each counts
    two = np.stack([five * 2 + five + [4.0] + five[1:32], [3.0] + five[1:] + five + [3.0] + five[1:] + five[:32]], axis=1)
    assert counted(two[:, :1], 1, slices=2) == 3 and counted(two[:, 1:], 1, slices=2, pad=9.0) == 2
    assert counted(two, 1, slices=2, cols=2, qmap=(0, 1), pad=9.0) == 3 and counted(two, 1, slices=2, cols=1, qmap=(0, 1), pad=9.0) == 5
    assert counted(two, 1, slices=4, cols=2, qmap=(0, 1, 1), pad=9.0) == 2 * 4   # one round per slice: all open, the slices past the table not walked


def test_every_round_of_one_round_slices_hits():
    rng = np.random.default_rng(2)
    n, dim, nq, k = 1500, 72, 70, 64
    X, Q = hs.widen(hs.ties(rng, n, dim, 0, "float16"), "float16"), hs.widen(hs.ties(rng, nq, dim, 0, "float16"), "float16")
    m = hw.search(xr.dist64(X, Q, 0), None, dim, k, np.arange(nq), xr.dist64(np.zeros((1, dim), np.float32), Q, 0)[0])
    assert m["plan"]["rows_per_slice"] == 64 and m["hit_rounds"] == m["plan"]["rounds"] == 24 * 2


@pytest.mark.parametrize("tag", sorted(hw.SHAPES))
def test_which_tables_leave_rounds_off_the_hit_path(tag, dtype="float16"):
    """the premise of test_gpu_half_rounds' `hit_rounds < rounds`, from the model alone: on the mostly-one-vector tables every shape with k <= 257
    does, the two with k = 1024 do not (no list fills in 256 or 384 rows, and the seed is the one vector's distance)"""
    metric = gr.METRICS[tag][0]
    (n, dim, nq, k) = hw.SHAPES[tag][0]
    X, Qd, qmap, _ = gr.case(tag, dtype, metric, "plain")
    Xw, Qw = hs.widen(X, dtype), hs.widen(Qd, dtype)
    m = hw.search(xr.dist64(Xw, Qw, metric), None, dim, k, qmap, xr.dist64(np.zeros((1, dim), np.float32), Qw, metric)[0])
    print("%s: model hit %d of %d rounds, seed pass %d" % (tag, m["hit_rounds"], m["plan"]["rounds"], m["seed_hit_rounds"]))
    assert 0 < m["hit_rounds"] <= m["plan"]["rounds"] and (m["hit_rounds"] < m["plan"]["rounds"]) == (tag in gr.PARTIAL)
    assert m["rows"][0, 0] == 1 and n - 1 in m["rows"][0] and (k < 3 or (n - 1) // 64 * 64 in m["rows"][0])   # the planted rows are found


def test_a_fully_random_table_hits_every_round():
    X, Qd, qmap, _ = gr.case("R1", "float16", 2, "random")
    n, dim, nq, k = hw.SHAPES["R1"][0]
    Xw, Qw = hs.widen(X, "float16"), hs.widen(Qd, "float16")
    m = hw.search(xr.dist64(Xw, Qw, 2), None, dim, k, qmap, xr.dist64(np.zeros((1, dim), np.float32), Qw, 2)[0])
    assert m["hit_rounds"] == m["plan"]["rounds"] == 16896
