"""What an answer of GpuIndex.search_among (eps_index_search_among) is held to, in numpy: for tests/test_among_ref_cpu.py (fed with numpy's own
answer, with the oracle's and with planted faults) and tests/test_gpu_search_among.py (fed with what the device returns).  Nothing here is
fitted to device output.

Query j's answer is the k smallest (distance, id) keys over the rows its list names that are visible.  A list is turned into rows by the id rule
(rows_of): id = row * stride + base names `row`; an id that is no such number for a row of the table names nothing; a row named twice is one row.
From there the list is just one more visibility mask, and the result is held to what a search is held to: exact_ref.check_exact on tables fp32
computes exactly (ids position by position, distance bits), exact_ref.check_topk with the documented tree's bound on continuous ones."""
import numpy as np

import exact_ref as er
import range_ref as rr

F = np.float32


# the continuous tables of tests/test_gpu_search_among.py (4096 x 64, 16 queries, seed 7) and their lists: 65, 512 and all 4096 rows.  The fp64
# reference leaves no row undecided on any of them (tests/test_among_ref_cpu.py keeps that run): a condition on the tables, not a measurement
CONT = (("gaussian", 0), ("embedding-like", 1), ("uniform", 2))
CONT_SHAPE = (4096, 64, 16)
CONT_K = (1, 10, 100)


def cont_lists():
    rng = np.random.default_rng(11)
    return [rng.choice(CONT_SHAPE[0], size=m, replace=False).astype(np.int64) for m in (65, 512, 4096)]


def names_a_row(ids, base, stride, n):
    """bool per entry: id = row * stride + base for a row of [0, n) (python integers: no id is too large or too small to be judged)"""
    base, stride = int(base), int(stride)
    return np.array([i >= base and (i - base) % stride == 0 and (i - base) // stride < n for i in np.asarray(ids).reshape(-1).tolist()], bool)


def rows_of(ids, base, stride, n):
    """the rows of [0, n) the ids name, each once, ascending"""
    ids = np.asarray(ids).reshape(-1)
    named = [(int(i) - int(base)) // int(stride) for i in ids[names_a_row(ids, base, stride, n)].tolist()]
    return np.array(sorted(set(named)), np.int64)


def list_masks(lists, n, nq):
    """lists: ONE array of rows (every query's list) or a sequence of nq of them -> bool [n][nq]"""
    shared = isinstance(lists, np.ndarray) and lists.ndim == 1 and lists.dtype != object
    assert shared or len(lists) == nq, "one list, or one per query"
    m = np.zeros((n, nq), bool)
    for q in range(nq):
        m[np.asarray(lists if shared else lists[q], np.int64), q] = True
    return m


def numpy_among(d32, lists, k, visible=None):
    """the answer from fp32 distances d32 [n][nq] and lists of ROWS (rows_of): (ids [nq][k] row numbers, dist [nq][k], counts [nq])"""
    n, nq = d32.shape
    take = list_masks(lists, n, nq) & rr.visible2(n, nq, visible)
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F)
    counts = np.zeros(nq, np.int32)
    for q in range(nq):
        row = np.flatnonzero(take[:, q])
        d = d32[row, q]
        o = np.lexsort((row, d))[:k]
        m = counts[q] = len(o)
        ids[q, :m] = row[o]
        dist[q, :m] = d[o]
    return ids, dist, counts


def check_among(ids, dist, counts, ref, lists, k, visible=None, exact=False, what=""):
    """ids [nq][k] are ROW numbers (undo an id map first); lists as for numpy_among; ref: exact_ref.Ref of (table, queries, metric).  exact: a
    table fp32 computes exactly - no band; else the tree bound, and the undecided rows over the queries are returned."""
    ids, dist, counts = np.asarray(ids), np.asarray(dist), np.asarray(counts)
    n, nq = ref.n, ref.nq
    assert ids.shape == (nq, k) and dist.shape == (nq, k) and counts.shape == (nq,), "%s: shapes" % what
    take = list_masks(lists, n, nq) & rr.visible2(n, nq, visible)
    und = 0
    for q in range(nq):
        one = ref.take([q])
        w = "%s query %d" % (what, q)
        if exact:
            er.check_exact(ids[q:q + 1], dist[q:q + 1], counts[q:q + 1], None, None, ref.metric, k, visible=take[:, q], ref=one, what=w)
        else:
            und += er.check_topk(ids[q:q + 1], dist[q:q + 1], counts[q:q + 1], None, None, ref.metric, k, visible=take[:, q], bound="tree", ref=one, what=w)
    return und
