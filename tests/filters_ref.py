"""What an answer of GpuIndex.search_filters (eps_index_search_filters) is held to, in numpy.  Nothing here is fitted to device output.

Query q sees row r iff r is visible under the standing state (select_ref.visible_rows) AND program query_prog[q] leaves a non-zero value on r
(select_ref.eval_program, `@distance` = 0; the empty program passes every row).  A query's filter is then one more visibility mask, held to what
search_among's answer is (among_ref): exactly on tables fp32 computes exactly, under exact_ref's tree bound on continuous ones."""
import numpy as np

import among_ref as ar
import select_ref as sr

FILTERS_CHUNK = 512   # csrc/filters_host.hpp: list entries per wavefront of the gather


def program_masks(n, programs, rows, standing=None):
    """bool [n][len(programs)]: the rows each program shows, the standing mask (bool [n]) ANDed in"""
    m = np.ones((n, len(programs)), bool)
    for j, prog in enumerate(programs):
        if prog:
            m[:, j] = sr.eval_program(prog, rows[:n])[:n] != 0.0
    if standing is not None:
        m &= np.asarray(standing, bool)[:, None]
    return m


def numpy_filters(d32, masks, query_prog, k):
    """(ids [nq][k] row numbers, dist [nq][k], counts [nq], visible int64 [nq]) from fp32 distances d32 [n][nq] and program_masks' masks"""
    query_prog = np.asarray(query_prog)
    lists = [np.flatnonzero(masks[:, j]) for j in query_prog]
    ids, dist, counts = ar.numpy_among(d32, lists, k)
    return ids, dist, counts, np.array([len(x) for x in lists], np.int64)


def check_filters(ids, dist, counts, visible, ref, masks, query_prog, k, exact=False, what=""):
    """ids [nq][k] are ROW numbers (undo an id map first); ref: exact_ref.Ref.  Returns the undecided rows (0 on an exact table)"""
    query_prog = np.asarray(query_prog)
    lists = [np.flatnonzero(masks[:, j]) for j in query_prog]
    want_vis = np.array([len(x) for x in lists], np.int64)
    assert np.array_equal(np.asarray(visible, np.int64), want_vis), "%s: visible %s, expected %s" % (what, np.asarray(visible)[:8], want_vis[:8])
    return ar.check_among(ids, dist, counts, ref, lists, k, exact=exact, what=what)
