"""The reference the sparse-vector tests trust (GpuSparseIndex / eps_sparse_index_*), in numpy alone.

  dist_seq      the reference's GetL2DistSqr / GetCosineDist / GetInnerProductDist (engine/db/vector.cpp:7-96) restated line by line on fp32 scalars:
                one accumulator from 0, the two-pointer merge, every product rounded before it is added.  fma=True fuses the product into the
                add - the fault a contracting compiler plants; used for nothing else.
  dist_dense    the same distances of a TIES table through its dense image (columns compressed to their rank): integers, so any order is exact
  topk          the k smallest (distance, id) keys over the visible rows - -0 equals +0, every NaN after +inf, ties by id
  same_answer   the comparator: ids, distance bits after + 0.0f (NaN equals NaN) and counts, nothing tolerated
  ties_table / piece_table / cont_table / hand_vectors   the tables"""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_MAX = 2 ** 31 - 1
L2, COSINE, DOT = 0, 1, 2
METRIC_NAMES = {L2: "EUCLIDEAN", COSINE: "COSINE", DOT: "DOT_PRODUCT"}


def host_constant(name):
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "sparse_host.hpp")).read()
    return int(re.search(r"constexpr \w+ %s = (\d+);" % name, src).group(1))


# ---------------------------------------------------------------- CSR helpers: a table is (offsets int64[n + 1], indices int32[nnz], values float32[nnz])
def csr(rows):
    """[(indices, values), ...] -> CSR"""
    off = np.zeros(len(rows) + 1, np.int64)
    for i, (ri, _) in enumerate(rows):
        off[i + 1] = off[i] + len(ri)
    idx = np.concatenate([np.asarray(ri, np.int64) for ri, _ in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate([np.asarray(rv, F) for _, rv in rows] + [np.zeros(0, F)]).astype(F)
    return off, idx, val


def row(t, r):
    return t[1][t[0][r]:t[0][r + 1]], t[2][t[0][r]:t[0][r + 1]]


def rows_of(t):
    return [row(t, r) for r in range(len(t[0]) - 1)]


def n_rows(t):
    return len(t[0]) - 1


# ---------------------------------------------------------------- the sequential model
def _acc(s, a, b, fma):
    """s + a * b: the product rounded to fp32 first, or (fma) the exact product added and rounded once (fp64 holds a 24 x 24-bit product exactly;
    the sum of it and an fp32 value is rounded to fp64 and then to fp32 - a double rounding that is harmless for a PLANTED fault)"""
    if fma:
        return F(np.float64(a) * np.float64(b) + np.float64(s))
    return F(s + F(a * b))


def dist_seq(xi, xv, qi, qv, metric, fma=False, drop_tail=False, norm64=False):
    """distance(v1 = row (xi, xv), v2 = query (qi, qv)).  drop_tail / norm64: planted faults - L2 without the tail of the longer side, COSINE
    with its norms summed in fp64"""
    n1, n2 = len(xi), len(qi)
    i1 = i2 = 0
    s = F(0)
    if metric == L2:   # vector.cpp:71-96
        while i1 < n1 or i2 < n2:
            if i1 < n1 and i2 < n2:
                if xi[i1] == qi[i2]:
                    d = F(xv[i1] - qv[i2])
                    i1 += 1
                    i2 += 1
                elif xi[i1] > qi[i2]:
                    d = qv[i2]
                    i2 += 1
                else:
                    d = xv[i1]
                    i1 += 1
            elif drop_tail:
                break
            elif i1 == n1:
                d = qv[i2]
                i2 += 1
            else:
                d = xv[i1]
                i1 += 1
            s = _acc(s, d, d, fma)
        return s
    while i1 < n1 and i2 < n2:   # vector.cpp:11-25, :35-45
        if xi[i1] == qi[i2]:
            s = _acc(s, xv[i1], qv[i2], fma)
            i1 += 1
            i2 += 1
        elif xi[i1] > qi[i2]:
            i2 += 1
        else:
            i1 += 1
    if metric == DOT:
        return F(-s)
    if norm64:
        a = F(np.sum(np.asarray(xv, np.float64) ** 2))
        b = F(np.sum(np.asarray(qv, np.float64) ** 2))
    else:
        a = F(0)
        for v in xv:   # vector.cpp:29-34
            a = _acc(a, v, v, fma)
        b = F(0)
        for v in qv:
            b = _acc(b, v, v, fma)
    with np.errstate(all="ignore"):
        return F(F(1) - F(s / np.sqrt(F(a * b))))   # :46 (an empty side: 0 / 0)


def dist_table(X, Q, metric, **fault):
    """float32 [n, nq] by the sequential model"""
    xs, qs = rows_of(X), rows_of(Q)
    out = np.empty((len(xs), len(qs)), F)
    for r, (xi, xv) in enumerate(xs):
        for j, (qi, qv) in enumerate(qs):
            out[r, j] = dist_seq(xi, xv, qi, qv, metric, **fault)
    return out


# ---------------------------------------------------------------- dense image of a ties table
def dense_images(X, Q, dtype=F):
    cols = np.unique(np.concatenate([X[1], Q[1]]))
    def image(t):
        n = n_rows(t)
        out = np.zeros((n, max(len(cols), 1)), dtype)
        r = np.repeat(np.arange(n), np.diff(t[0]))
        out[r, np.searchsorted(cols, t[1])] = t[2]
        return out
    return image(X), image(Q)


def dist_dense(X, Q, metric, dtype=F):
    """[n, nq] through the dense image, in `dtype` arithmetic.  COSINE: exact integer dot and norms, then the three fp32 operations of the epilogue"""
    Xd, Qd = dense_images(X, Q, dtype)
    if metric == L2:   # (|x|^2 + |q|^2 - 2 x.q: on integers as exact as the sum of squared differences)
        return (Xd ** 2).sum(1, dtype=dtype)[:, None] + (Qd ** 2).sum(1, dtype=dtype)[None, :] - dtype(2) * (Xd @ Qd.T)
    dot = Xd @ Qd.T
    if metric == DOT:
        return -dot
    a = (Xd ** 2).sum(1, dtype=dtype)[:, None]
    b = (Qd ** 2).sum(1, dtype=dtype)[None, :]
    with np.errstate(all="ignore"):
        return dtype(1) - dot / np.sqrt(a * b)


# ---------------------------------------------------------------- top-k and the comparator
def bits(d):
    """uint32 image after + 0.0f, every NaN as ONE word"""
    d = np.asarray(d, F) + F(0)
    u = d.view(np.uint32).copy()
    u[np.isnan(d)] = 0x7FC00000
    return u


def topk(dist, k, visible=None, base=0, stride=1):
    """dist [n, nq] -> ids int64 [nq, k], dist float32 [nq, k], counts int32 [nq]; unused slots -1 / +inf"""
    dist = np.asarray(dist, F)
    n, nq = dist.shape
    ids = np.full((nq, k), -1, np.int64)
    out = np.full((nq, k), np.inf, F)
    counts = np.zeros(nq, np.int32)
    rows = np.arange(n) if visible is None else np.flatnonzero(visible)
    for j in range(nq):
        d = dist[rows, j] + F(0)
        nan = np.isnan(d)
        order = np.lexsort((rows, np.where(nan, F(0), d), nan))[:k]
        m = len(order)
        ids[j, :m] = rows[order] * stride + base
        out[j, :m] = d[order]
        counts[j] = m
    return ids, out, counts


def same_answer(got, want, what=""):
    """ids, distance bits and counts are EQUAL - no tolerance"""
    gi, gd, gc = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in got)
    wi, wd, wc = want
    assert gi.shape == wi.shape and gd.shape == wd.shape and gc.shape == wc.shape, (what, gi.shape, wi.shape)
    assert np.array_equal(gc, wc), "%s: counts differ at queries %s: got %s, expected %s" % (
        what, np.flatnonzero(gc != wc)[:5].tolist(), gc[gc != wc][:5].tolist(), wc[gc != wc][:5].tolist())
    bad = np.argwhere(gi != wi)
    assert len(bad) == 0, "%s: ids differ at (query, rank) %s: got %s, expected %s" % (what, bad[:5].tolist(), gi[gi != wi][:5].tolist(), wi[gi != wi][:5].tolist())
    gb, wb = bits(gd), bits(wd)
    bad = np.argwhere(gb != wb)
    assert len(bad) == 0, "%s: distance bits differ at (query, rank) %s: got %s, expected %s" % (
        what, bad[:5].tolist(), gd[gb != wb][:5].tolist(), wd[gb != wb][:5].tolist())


# ---------------------------------------------------------------- tables
def ties_table(n, nq, seed, max_nz=40, pool=150, dim=DIM_MAX):
    """integer values -4 .. 4 (stored zeros included) on a pool of `pool` columns spread over [0, dim) that holds 0 and dim - 1; rows and queries
    of 0 .. max_nz non-zeros.  Asserts what the tests lean on: fp32 in any order equals fp64 for L2 and dot."""
    rng = np.random.default_rng(seed)
    cols = np.unique(np.concatenate([[0, dim - 1], rng.integers(0, dim, size=pool - 2)]))
    def make(m):
        out = []
        for i in range(m):
            z = int(rng.integers(0, min(max_nz, len(cols)) + 1))
            out.append((np.sort(rng.choice(cols, size=z, replace=False)), rng.integers(-4, 5, size=z).astype(F)))
        return out
    rows = make(n)
    if n > 2:
        rows[n // 2] = (np.zeros(0, np.int64), np.zeros(0, F))   # an empty row whatever the draw: COSINE's NaN
    X, Q = csr(rows), csr(make(nq))
    if n * nq <= 1 << 16:
        for metric in (L2, DOT):
            assert np.array_equal(dist_dense(X, Q, metric, F).astype(np.float64), dist_dense(X, Q, metric, np.float64)), "the ties table is not exact"
    return X, Q


def piece_lengths():
    """130 row lengths around SPARSE_PIECE (sparse_host.hpp: the step of the kernel form that staged a wavefront's 64 rows in LDS; the lengths stay
    as the edges any chunked form has).  A wavefront's round is 64 rows, so rows 64 .. 68 start one, and their ends fall exactly on multiples of
    the piece counted from the round's first element: 512 | 200 + 312 | an empty row on the boundary | 1024"""
    P = host_constant("SPARSE_PIECE")
    L = [3, 0, 7, 1, 12, 5] * 22
    L = L[:130]
    L[0] = P - 1                          # first
    L[9], L[20], L[31], L[40] = P + 1, 2 * P + 3, P, P - 1   # between short rows
    L[64], L[65], L[66], L[67], L[68] = P, 200, P - 200, 0, 2 * P
    L[100] = 2 * P + 3
    L[128] = P + 1
    L[129] = 2 * P + 3                    # last
    return L


def piece_table(seed=11):
    """rows of piece_lengths(), queries of 0, 1 and SPARSE_MAX_QUERY_NNZ non-zeros; integer values, so the dense image is exact"""
    rng = np.random.default_rng(seed)
    qmax = host_constant("SPARSE_MAX_QUERY_NNZ")
    cols = np.unique(np.concatenate([[0, DIM_MAX - 1], rng.integers(0, DIM_MAX, size=qmax + 1500)]))
    assert len(cols) >= qmax
    def vec(z):
        return np.sort(rng.choice(cols, size=z, replace=False)), rng.integers(-4, 5, size=z).astype(F)
    X = csr([vec(z) for z in piece_lengths()])
    Q = csr([vec(0), vec(1), vec(qmax), vec(37)])
    return X, Q


def cont_table(n=300, nq=7, max_row=60, max_query=40, dim=400, seed=5):
    """the recipe the model was measured on against the reference: values +-U[0.25, 4) (no denormals), 0 .. max non-zeros over `dim` columns"""
    rng = np.random.default_rng(seed)
    def table(m, maxnz):
        out = []
        for _ in range(m):
            z = int(rng.integers(0, maxnz + 1))
            c = np.sort(rng.choice(dim, size=z, replace=False))
            out.append((c, (rng.uniform(0.25, 4, z) * rng.choice([-1, 1], z)).astype(F)))
        return csr(out)
    return table(n, max_row), table(nq, max_query)


def hand_vectors():
    """the vectors the fixture holds as rows AND as queries: empty; one index at 0; one at 2^31 - 2; disjoint supports; identical vectors; a prefix
    of another (L2's tail on either side); a common index at 0 and at 2^31 - 2"""
    top = DIM_MAX - 1
    return [
        ([], []),
        ([0], [1.7]),
        ([top], [2.3]),
        ([3, 7, 9], [1.1, 2.6, -3.3]),
        ([4, 8], [0.7, 1.3]),
        ([3, 7], [1.1, 2.6]),
        ([3, 7, 9, 11, 12], [1.1, 2.6, -3.3, 0.9, -1.9]),
        ([0, 5, top], [2.9, 1.3, -1.7]),
    ]


def fixture_tables():
    """rows and queries of tests/golden/sparse_reference_distances.npz: the recipe's 300 x 7 table, then the hand-made vectors"""
    X, Q = cont_table()
    hand = [(np.asarray(i, np.int64), np.asarray(v, F)) for i, v in hand_vectors()]
    return csr(rows_of(X) + hand), csr(rows_of(Q) + hand)
