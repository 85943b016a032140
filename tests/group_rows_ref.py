"""What an answer of GpuIndex.search_group_rows (eps_index_search_group_rows) is held to, in numpy: for tests/test_group_rows_ref_cpu.py (fed with
hand-written cases and planted faults) and tests/test_gpu_group_rows.py (fed with what the device returns).  Nothing here is fitted to device
output.

The rule, for query j, with V_j, the distances and the (distance, row) key order of groups_ref.  The groups are those of groups_ref.numpy_groups;
of the s-th group g the answer holds the c = min(m, |V_j n g|) smallest keys of V_j n g in ascending order, row_counts = c, group_sizes =
|V_j n g|.  Equivalently: walk V_j in ascending key order, admit a group on its first row until k groups are admitted, keep a row iff its group is
admitted and holds fewer than m rows; every visible row of an admitted group counts towards its size.  numpy_group_rows computes both forms and
asserts that they agree."""
import numpy as np

import groups_ref as gr

F = np.float32
NAMES = ("ids", "dist", "group_keys", "row_counts", "group_sizes", "counts")


def by_groups(d, vis, keys, k, m):
    """form 1: the groups of groups_ref (their representatives, in answer order), then per group a sort by key cut at m"""
    reps = gr.by_representatives(d, vis, keys, k)
    out = []
    for r in reps.tolist():
        mine = np.flatnonzero(vis & (keys == keys[r]))
        mine = mine[gr.key_order(d[mine], mine)]
        out.append((int(keys[r]), mine[:m].tolist(), len(mine)))
    return out


def by_walk(d, vis, keys, k, m):
    """form 2: one walk over the visible rows in ascending key order"""
    rows = np.flatnonzero(vis)
    slot, out = {}, []
    for r in rows[gr.key_order(d[rows], rows)].tolist():
        g = int(keys[r])
        if g not in slot:
            if len(out) == k:
                continue
            slot[g] = len(out)
            out.append([g, [], 0])
        e = out[slot[g]]
        if len(e[1]) < m:
            e[1].append(r)
        e[2] += 1
    return [tuple(e) for e in out]


def numpy_group_rows(d32, keys, k, m, visible=None):
    """the answer from fp32 distances d32 [n][nq] and int64 keys [n]: (ids [nq][k][m] ROW numbers, dist [nq][k][m], group_keys [nq][k],
    row_counts [nq][k], group_sizes [nq][k], counts [nq])"""
    n, nq = d32.shape
    keys = np.asarray(keys, np.int64)
    assert keys.shape == (n,)
    vis = gr.rr.visible2(n, nq, visible)
    ids = np.full((nq, k, m), -1, np.int64)
    dist = np.full((nq, k, m), np.inf, F)
    gk = np.zeros((nq, k), np.int64)
    rc = np.zeros((nq, k), np.int32)
    gs = np.zeros((nq, k), np.int64)
    counts = np.zeros(nq, np.int32)
    for q in range(nq):
        a = by_groups(d32[:, q], vis[:, q], keys, k, m)
        b = by_walk(d32[:, q], vis[:, q], keys, k, m)
        assert a == b, "the two forms of the rule disagree on query %d" % q
        counts[q] = len(a)
        for s, (g, rows, size) in enumerate(a):
            c = len(rows)
            ids[q, s, :c] = rows
            dist[q, s, :c] = d32[rows, q]
            gk[q, s], rc[q, s], gs[q, s] = g, c, size
    return ids, dist, gk, rc, gs, counts


def same(got, want, what=""):
    """ids, distance bits (a NaN equals a NaN), group keys, row counts, group sizes, counts: equality, position by position"""
    assert len(got) == len(want) == len(NAMES)
    for x, y, name in zip(got, want, NAMES):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, "%s %s: shape %s != %s" % (what, name, x.shape, y.shape)
        if name == "dist":
            x, y = np.where(np.isnan(x), np.uint32(0xFFC00000), gr.bits(x)), np.where(np.isnan(y), np.uint32(0xFFC00000), gr.bits(y))
        bad = np.argwhere(x != y)
        assert len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def mapped(ans, base=0, stride=1):
    """a model answer with its row numbers under the id map (base, stride)"""
    return (np.where(ans[0] >= 0, ans[0] * stride + base, -1),) + tuple(ans[1:])


def check_group_rows(got, d32, keys, k, m, visible=None, base=0, stride=1, what=""):
    """got = the six arrays as the call returns them, ids under the id map (base, stride)"""
    same(got, mapped(numpy_group_rows(d32, keys, k, m, visible), base, stride), what)
