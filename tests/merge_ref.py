"""What eps_merge_range / eps_merge_select (csrc/merge_lists.hip) are held to, in numpy, twice over:

  merge_range / merge_select      the definition: the valid elements of all lists concatenated, sorted by key, cut to the window.  A radius key is
                                  (ordinal of the fp32 distance as make_key of csrc/device_common.hpp computes it: -0 folded into +0, every NaN ONE
                                  ordinal above +inf; then the 64-bit id); a select key is the id.  The distance written is the ordinal's.
  rank_range / rank_select        the kernel's rule restated element by element: rank(e in list s at position p) = p + sum over t < s of
                                  #{x in list t : x <= e} + sum over t > s of #{x in list t : x < e}; an element is written iff its rank lies in the
                                  window.  It also reports whether any slot was written twice.

tests/test_merge_ref_cpu.py holds the two to each other and - through range_ref / select_ref - to the claim the merge exists for: the answers of
the shards i mod G of a table, merged, are the answer of the whole table.  tests/test_gpu_merge_lists.py feeds the device's answers to the same
functions.  Every comparison is equality of integers and of float bit patterns."""
import numpy as np

F = np.float32
ORD_NAN = np.uint32(0xFFC00000)


def ordinal(d):
    """make_key's high word, float32 array -> uint32 array"""
    d = np.asarray(d, F) + F(0)
    u = d.view(np.uint32)
    o = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(d), ORD_NAN, o)


def ord2f(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000) != 0, o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(F)


def bits(d):
    return np.ascontiguousarray(d, F).view(np.uint32)


def _lens(counts, L):
    return np.clip(np.asarray(counts, np.int64), 0, L)


def merge_range(ids, dist, counts, totals, skip=0):
    """ids int64 / dist float32 [G][nq][cap], counts [G][nq], totals [G][nq] -> (ids [nq][cap], dist [nq][cap], counts int32 [nq], totals int64 [nq])"""
    ids, dist = np.asarray(ids, np.int64), np.asarray(dist, F)
    G, nq, cap = ids.shape
    lens = _lens(counts, cap)
    out_ids = np.full((nq, cap), -1, np.int64)
    out_dist = np.full((nq, cap), np.inf, F)
    out_counts = np.zeros(nq, np.int32)
    for j in range(nq):
        i = np.concatenate([ids[s, j, :lens[s, j]] for s in range(G)])
        o = np.concatenate([ordinal(dist[s, j, :lens[s, j]]) for s in range(G)])
        order = np.lexsort((i, o))[skip:skip + cap]
        m = out_counts[j] = len(order)
        out_ids[j, :m] = i[order]
        out_dist[j, :m] = ord2f(o[order])
    return out_ids, out_dist, out_counts, np.asarray(totals, np.int64).sum(axis=0)


def merge_select(ids, counts, totals, skip, limit):
    """ids [G][len], counts [G], totals [G] -> (ids of the window, total)"""
    ids = np.asarray(ids, np.int64)
    lens = _lens(counts, ids.shape[1])
    allids = np.sort(np.concatenate([ids[s, :lens[s]] for s in range(ids.shape[0])]), kind="stable")
    return allids[skip:skip + limit], int(np.asarray(totals, np.int64).sum())


def _ranks(keys_by_list):
    """keys_by_list: per list a sorted array of keys (python ints) -> per list the ranks of its elements, by counting"""
    out = []
    for s, mine in enumerate(keys_by_list):
        r = np.arange(len(mine), dtype=np.int64)
        for t, other in enumerate(keys_by_list):
            if t != s:
                r += np.searchsorted(other, mine, side="right" if t < s else "left")
        out.append(r)
    return out


def _keys(o, i):
    """(ordinal, id) as one python int per element: 32 + 64 bits, ids ordered as signed"""
    return np.array([(int(a) << 64) | (int(b) + (1 << 63)) for a, b in zip(o, i)], dtype=object)


def rank_range(ids, dist, counts, totals, skip=0):
    """as merge_range, by the rank rule; returns (..., clash): clash = some slot was written twice or a rank was not a permutation"""
    ids, dist = np.asarray(ids, np.int64), np.asarray(dist, F)
    G, nq, cap = ids.shape
    lens = _lens(counts, cap)
    out_ids = np.full((nq, cap), -1, np.int64)
    out_dist = np.full((nq, cap), np.inf, F)
    out_counts = np.zeros(nq, np.int32)
    clash = False
    for j in range(nq):
        os_ = [ordinal(dist[s, j, :lens[s, j]]) for s in range(G)]
        ranks = _ranks([_keys(os_[s], ids[s, j, :lens[s, j]]) for s in range(G)])
        allr = np.concatenate(ranks) if G else np.zeros(0, np.int64)
        clash |= not np.array_equal(np.sort(allr), np.arange(len(allr)))
        for s in range(G):
            for p, r in enumerate(ranks[s]):
                if skip <= r < skip + cap:
                    out_ids[j, r - skip] = ids[s, j, p]
                    out_dist[j, r - skip] = ord2f(os_[s][p])
        out_counts[j] = min(max(int(lens[:, j].sum()) - skip, 0), cap)
    return out_ids, out_dist, out_counts, np.asarray(totals, np.int64).sum(axis=0), clash


def rank_select(ids, counts, totals, skip, limit):
    ids = np.asarray(ids, np.int64)
    G = ids.shape[0]
    lens = _lens(counts, ids.shape[1])
    ranks = _ranks([ids[s, :lens[s]] for s in range(G)])
    count = min(max(int(lens.sum()) - skip, 0), limit)
    out = np.full(count, np.iinfo(np.int64).min, np.int64)
    for s in range(G):
        sel = (ranks[s] >= skip) & (ranks[s] < skip + limit)
        out[ranks[s][sel] - skip] = ids[s, :lens[s]][sel]
    allr = np.concatenate(ranks)
    return out, int(np.asarray(totals, np.int64).sum()), not np.array_equal(np.sort(allr), np.arange(len(allr)))


def same_range(a, b, what=""):
    """ids, distance bit patterns, counts, totals"""
    for x, y, name in zip(a, b, ("ids", "dist", "counts", "totals")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "dist":
            x, y = bits(x), bits(y)
        assert x.shape == y.shape, "%s %s: shapes %s %s" % (what, name, x.shape, y.shape)
        bad = np.argwhere(x != y)
        assert len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def random_lists(rng, G, nq, cap, plant=True, first_kind=0):
    """sorted lists with what can go wrong planted: unequal lengths, empty lists, one full list among empty ones, all-empty queries, a shard whose
    total exceeds cap, equal distances across shards, -0.0 / +0.0, +inf, the same id in several shards.  Tails hold garbage, not -1 / +inf:
    only counts says where a list ends.  Query j is of kind (j + first_kind) % 7: 0 all lists empty, 1 one full list among empty ones, 2 every list
    full, 3 the same id in every element, 4 .. 6 random lengths.  Returns (ids, dist, counts int32, totals int64)."""
    ids = rng.integers(-5, 1 << 40, (G, nq, cap)).astype(np.int64)
    dist = rng.random((G, nq, cap)).astype(F)
    counts = np.zeros((G, nq), np.int32)
    totals = np.zeros((G, nq), np.int64)
    pool_d = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, 3.0, np.inf], F)
    for j in range(nq):
        kind = (j + first_kind) % 7
        for s in range(G):
            if kind == 0:
                m = 0                                          # an all-empty query
            elif kind == 1:
                m = cap if s == (j // 7 + 1) % G else 0            # one full list among empty ones
            elif kind == 2:
                m = cap                                        # every list full
            else:
                m = int(rng.integers(0, cap + 1))
            if plant and m:
                few = max(2, min(cap, 4))                      # few distinct distances and ids: ties across and inside shards
                d = rng.choice(pool_d, m)
                i = rng.integers(0, few * G, m).astype(np.int64) * (1 << 33) + 7   # (beyond 32 bits)
                if kind == 3:
                    i[:] = 5                                   # the same id everywhere: only the shard number orders them
            else:
                d = rng.random(m).astype(F) * 4 - 1
                i = rng.integers(0, 1 << 40, m).astype(np.int64)
            order = np.lexsort((i, ordinal(d)))
            ids[s, j, :m], dist[s, j, :m] = i[order], d[order]
            counts[s, j] = m
            totals[s, j] = m + (int(rng.integers(1, 1000)) if m == cap and rng.random() < 0.5 else 0)   # (total > cap: the list is a cut)
    return ids, dist, counts, totals
