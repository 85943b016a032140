"""The rule of GpuIndex.search_hybrid (eps_index_search_hybrid) in numpy, and nothing more: from the two fp32 distance tables D[nq][n] (dense) and
S[nq][n] (sparse), the weights and a visibility mask, the k smallest scores per query.  score = (w_dense * D) + (w_sparse * S): two rounded fp32
multiplies and one rounded fp32 add.  Keys order as make_key orders them: -0 equals +0, every NaN after +inf, ties to the smaller row."""
import numpy as np

F = np.float32


def canon(a):
    """uint32 words as a key holds a value: after + 0.0f, every NaN as the one quiet NaN"""
    a = np.asarray(a, F) + F(0)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


def score(D, S, w_dense, w_sparse):
    with np.errstate(all="ignore"):
        return (F(w_dense) * np.asarray(D, F)) + (F(w_sparse) * np.asarray(S, F))   # (float32 arrays: numpy rounds every operation to fp32)


def topk(D, S, w_dense, w_sparse, k, visible=None, base=0, stride=1):
    """-> ids int64[nq, k], score, dense, sparse float32[nq, k], counts int32[nq]; unused slots -1 / +inf / +inf / +inf"""
    D, S = np.asarray(D, F), np.asarray(S, F)
    nq, n = D.shape
    sc = score(D, S, w_dense, w_sparse) + F(0)
    rows = np.arange(n) if visible is None else np.flatnonzero(visible)
    ids = np.full((nq, k), -1, np.int64)
    out = [np.full((nq, k), np.inf, F) for _ in range(3)]
    counts = np.zeros(nq, np.int32)
    for j in range(nq):
        s = sc[j, rows]
        nan = np.isnan(s)
        order = rows[np.lexsort((rows, np.where(nan, F(0), s), nan))[:k]]
        m = counts[j] = len(order)
        ids[j, :m] = order * stride + base
        for o, src in zip(out, (sc, D, S)):
            o[j, :m] = src[j, order]
    return (ids, *out, counts)


def same(got, want, what=""):
    """ids, counts and the words of score, dense and sparse are EQUAL (got's dense / sparse may be None: not asked for)"""
    names = ("ids", "score", "dense", "sparse", "counts")
    for g, w, name in zip(got, want, names):
        if g is None:
            continue
        g = np.asarray(g.cpu() if hasattr(g, "cpu") else g)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        gw, ww = (g, w) if name in ("ids", "counts") else (canon(g), canon(w))
        bad = np.argwhere(gw != ww)
        assert len(bad) == 0, "%s: %s differ at %s: got %s, expected %s" % (what, name, bad[:5].tolist(), g[gw != ww][:5].tolist(), w[gw != ww][:5].tolist())
