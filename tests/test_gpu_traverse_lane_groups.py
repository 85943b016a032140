"""The exact 8-bit lower-bound test that both traversal kernels share (csrc/traverse_steps.hpp mirror_dots) at the lane groups the other suites do
not reach: 64 lanes per mirror row in the search kernel (3 rows in flight per lane group), 16, 32 and 64 lanes per row in the build's Link search
(2 rows in flight).  The test only ever drops what `dist > bound` would drop, so everything is the same bit for bit with it off and on."""
import numpy as np
import pytest

from helpers import data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


@pytest.mark.parametrize("d,T,L", [(1552, 1, 100), (1540, 4, 200)])   # 64 lanes per row; 1540: a ragged last piece
def test_search_prefilter_is_invisible_at_64_lanes_per_row(amd, monkeypatch, d, T, L):
    n = 4000
    X, Q = data(n, d, 11 + d), data(32, d, 12 + d)
    ix = amd.GpuIndex(d, 0)
    ix.attach_rows(X)
    ix.build(n)
    res = {}
    for pf in ("0", "1"):
        monkeypatch.setenv("EPS_TRV_PREFILTER", pf)
        ids, dist, cnt = ix.search(Q, min(L, 100), mode=amd.MODE_GRAPH, intra_threads=T, master_queue=L, local_queue=L)
        st = ix.stats()
        res[pf] = (ids.copy(), dist.copy(), cnt.copy(), st["dist_evals"], st["expansions"], st["rerank_rows"])
    ix.close()
    a, b = res["0"], res["1"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and a[4] == b[4]
    assert b[5] > 0, "the 8-bit test did not run"


@pytest.mark.parametrize("d", [400, 772, 1552])   # 16, 32, 64 lanes per row
def test_link_prefilter_is_invisible_at_wide_rows(amd, monkeypatch, capfd, d):
    n = 3000
    X = data(n, d, 21 + d)
    ix = amd.GpuIndex(d, 0)
    ix.attach_rows(X)
    knn = ix.knn_graph()
    ix.close()
    monkeypatch.setenv("EPS_DEBUG", "1")   # Link's report says whether its searches ran the 8-bit test (csrc/graph_build.hip link_report)
    res, ran = [], []
    for pf in ("0", "1"):
        monkeypatch.setenv("EPS_BUILD_PREFILTER", pf)
        ix = amd.GpuIndex(d, 0)
        ix.attach_rows(X)
        capfd.readouterr()
        res.append(ix.link(knn, -1))
        ran.append("Link: 8-bit prefilter on" in capfd.readouterr().err)
        ix.close()
    (ids0, deg0, nav0), (ids1, deg1, nav1) = res
    assert ran == [False, True], "the 8-bit test did not run"
    assert nav0 == nav1 and np.array_equal(deg0, deg1) and np.array_equal(ids0, ids1)
    assert deg0.min() >= 1
