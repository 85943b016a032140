"""GpuHalfIndex (csrc/half.hip) where a slice of half_scan_kernel walks more than one round of 64 rows - the grid capped by the number of query
tiles or by the merge's keys - against half_walk_ref: results exact through exact_ref.check_exact, and stats()["hit_rounds"] /
["seed_hit_rounds"] EQUAL to the model's count of rounds that take the hit path, so that a threshold that is stale, too loose or never
refreshed is seen although its answers are right.  The shapes are half_walk_ref.SHAPES (pinned to half_plan by tests/native/half_host_check.cpp
and to the model's plan by tests/test_half_walk_ref_cpu.py).  A batch is a few distinct queries repeated with a period coprime to the tile
width: the reference is computed for the distinct ones and every repetition must equal its first occurrence.

Tables are tables of ties (test_gpu_half_search.ties) of which about 98 % of the rows are one vector: once a list has filled, a round of nothing
else only ties with its k-th distance and must end at the vote.  Where that leaves rounds off the hit path is the model's to say, from the table
alone (PARTIAL, checked on the CPU in tests/test_half_walk_ref_cpu.py): with k = 1024 no slice's list fills and the seed is the one vector's
distance, so every round hits."""
import numpy as np
import pytest

import exact_ref as xr
import half_walk_ref as hw
import test_gpu_half_search as hs

pytestmark = pytest.mark.gpu

# tag -> the metric under (float16, bfloat16): every metric meets a seeded (R1s, R2, R3) and an unseeded shape; the two long dims stay off
# EUCLIDEAN, whose fp64 reference is term by term
METRICS = {"R1": (0, 1), "R1s": (1, 2), "R2": (2, 0), "R3": (0, 1), "R4": (2, 0), "R5": (1, 2), "R6": (1, 2), "R7": (2, 1), "R8": (0, 2)}
VARIANT_NAMES = ("plain", "bitset", "id_map", "random")
VARIANTS = {"R1": ("plain", "bitset"), "R1s": ("plain", "bitset", "id_map"), "R2": ("plain", "bitset")}
CASES = [(tag, dtype, METRICS[tag][j], v) for tag in hw.SHAPES for j, dtype in enumerate(hs.DTYPES) for v in VARIANTS.get(tag, ("plain",))] + \
        [("R1", "float16", 2, "random")]
# the cases whose model leaves rounds off the hit path (the others: every round hits)
PARTIAL = {"R1", "R1s", "R4", "R5", "R6", "R7", "R8"}


def period(tag):
    return min(hw.SHAPES[tag][0][2], 13 if tag == "R3" else 97)


def case(tag, dtype, metric, variant):
    """(X, distinct queries, qmap, hidden or None) of a case, from its name alone"""
    n, dim, nq, _ = hw.SHAPES[tag][0]
    rps = hw.SHAPES[tag][3][1]
    rng = np.random.default_rng([n, dim, nq, metric, hs.DTYPES.index(dtype), VARIANT_NAMES.index(variant)])
    X = hs.ties(rng, n, dim, metric, dtype)
    if variant != "random":
        X[rng.random(n) >= 0.02] = hs.ties(rng, 1, dim, metric, dtype)[0]
    Qd = hs.ties(rng, period(tag), dim, metric, dtype)
    planted = [1, (n - 1) // 64 * 64, n - 1]   # the first slice; the last non-empty slice's last round; the last row
    X[planted] = Qd[0]
    hidden = None
    if variant == "bitset":
        hidden = rng.random(n) < 0.5
        hidden[3 * rps + 64:3 * rps + 128] = True   # the whole second round of slice 3
        hidden[planted] = False
    return X, Qd, np.arange(nq) % len(Qd), hidden


def run(ix, Q, k, qmap, id_map=(0, 1)):
    """search; every repetition of a query answers as its first occurrence; (rows, dist, counts) of the distinct queries"""
    ids, dist, cnt = (hs.np_(a) for a in ix.search(Q, k))
    U = int(qmap.max()) + 1
    assert np.array_equal(ids, ids[:U][qmap]) and np.array_equal(dist.view(np.uint32), dist[:U][qmap].view(np.uint32)) and np.array_equal(cnt, cnt[:U][qmap])
    ids = ids[:U]
    assert ((ids < 0) | ((ids - id_map[0]) % id_map[1] == 0)).all()
    return np.where(ids >= 0, (ids - id_map[0]) // id_map[1], -1), dist[:U], cnt[:U]


def held_to_model(ix, model, what):
    s = ix.stats()
    pl = model["plan"]
    print("half rounds %s: hit %d of %d rounds (model %d), seed pass %d (model %d)" % (what, s["hit_rounds"], s["rounds"], model["hit_rounds"], s["seed_hit_rounds"],
                                                                                      model["seed_hit_rounds"]))
    assert (s["live_columns"], s["kpl"], s["rounds"], s["seed_rows"], s["seeded"]) == (pl["cols"], pl["kpl"], pl["rounds"], pl["seed_rows"], pl["seed_rows"] > 0)
    assert s["hit_rounds"] == model["hit_rounds"] and s["seed_hit_rounds"] == model["seed_hit_rounds"], what
    return s


@pytest.mark.parametrize("tag,dtype,metric,variant", CASES)
def test_rounds(tag, dtype, metric, variant):
    (n, dim, nq, k), rps = hw.SHAPES[tag][0], hw.SHAPES[tag][3][1]
    X, Qd, qmap, hidden = case(tag, dtype, metric, variant)
    Xw, Qw = hs.widen(X, dtype), hs.widen(Qd, dtype)
    ref = xr.Ref(Xw, Qw, metric)
    visible = None if hidden is None else ~hidden
    model = hw.search(ref.d64, visible, dim, k, qmap, xr.dist64(np.zeros((1, dim), np.float32), Qw, metric)[0])
    assert rps > 64 and model["plan"]["rows_per_slice"] == rps
    id_map = (3, 8) if variant == "id_map" else (0, 1)
    what = "%s %s %s %s" % (tag, dtype, hs.METRIC[metric], variant)
    ix = hs.index(dim, metric, dtype)
    ix.attach_rows(X)
    ix.set_id_map(*id_map)
    if hidden is not None:
        ix.set_deleted(np.packbits(hidden, bitorder="little"))
    rows, dist, cnt = run(ix, Qd[qmap], k, qmap, id_map)
    s = held_to_model(ix, model, what)
    ix.close()
    xr.check_exact(rows, dist, cnt, Xw, Qw, metric, k, visible, ref=ref, what=what)
    assert 0 < s["hit_rounds"] <= s["rounds"] and (s["hit_rounds"] < s["rounds"]) == (tag in PARTIAL and variant != "random")


def test_a_nan_seed_opens_every_slice(tag="R2", dtype="float16", metric=0):
    """a NaN element in a prefix row and exactly k visible rows in the prefix: the prefix's k-th key is the NaN row, the seed one above ORD_NAN -
    a NaN threshold, everything passes - and the answer is exact all the same: the finite rows by (distance, row), as
    test_nan_and_infinite_rows_order_as_in_the_flat_search orders them (the NaN row, last of all visible rows, lies beyond k)"""
    n, dim, nq, k = hw.SHAPES[tag][0]
    sr = hw.SHAPES[tag][4]
    X, Qd, qmap, _ = case(tag, dtype, metric, "plain")
    rng = np.random.default_rng(11)
    hidden = rng.random(n) < 0.5
    hidden[:sr] = True
    hidden[rng.choice(sr, k, replace=False)] = False
    nan_row = int(np.flatnonzero(~hidden[:sr])[k // 2])
    X[nan_row, 7] = np.nan
    d64 = xr.dist64(hs.widen(X, dtype), hs.widen(Qd, dtype), metric)
    model = hw.search(d64, ~hidden, dim, k, qmap, xr.dist64(np.zeros((1, dim), np.float32), hs.widen(Qd, dtype), metric)[0])
    assert (model["seed"] == int(hw.ORD_NAN) + 1).all() and model["hit_rounds"] == model["plan"]["rounds"]
    ix = hs.index(dim, metric, dtype)
    ix.attach_rows(X)
    ix.set_deleted(np.packbits(hidden, bitorder="little"))
    rows, dist, cnt = run(ix, Qd[qmap], k, qmap)
    held_to_model(ix, model, "NaN seed")
    ix.close()
    vis = np.flatnonzero(~hidden & (np.arange(n) != nan_row))
    for q in range(len(Qd)):
        want = vis[np.lexsort((vis, d64[vis, q]))][:k]
        assert cnt[q] == k and np.array_equal(rows[q], want) and np.array_equal(dist[q].astype(np.float64), d64[want, q]), q
        assert np.array_equal(rows[q], model["rows"][q]) and np.array_equal(dist[q], model["dist"][q])


@pytest.mark.parametrize("metric", (2, 0))
def test_subnormal_fp16_elements_are_read_not_flushed(metric, dtype="float16"):
    """rows of small integers x 2^-24 - every element a subnormal half - against queries of small integers (DOT_PRODUCT) or of small integers
    x 2^-24 (EUCLIDEAN): every product and sum is an fp32 number, so the matrix cores' dot products agree with the norm terms (computed from the
    widened floats) and the answer is exact bit for bit only if v_mfma_f32_16x16x32_f16 reads subnormal operands as their values"""
    rng = np.random.default_rng(24)
    n, dim, nq, k = 300, 40, 7, 10
    tiny = np.float32(2.0 ** -24)
    X = (rng.integers(-8, 9, (n, dim)).astype(np.float32) * tiny).astype(np.float16)
    Q = (rng.integers(-8, 9, (nq, dim)).astype(np.float32) * (tiny if metric == 0 else np.float32(1))).astype(np.float16)
    assert ((X.view(np.uint16) & 0x7C00) == 0).all() and (X != 0).any() and np.array_equal(X.astype(np.float32) / tiny, np.rint(X.astype(np.float32) / tiny))
    ix = hs.index(dim, metric, dtype)
    ix.attach_rows(X)
    hs.exact(ix, X, Q, metric, dtype, k, what="subnormal %s" % hs.METRIC[metric])
    ix.close()
