"""What the STAGES of the graph build (csrc/graph_build.hip, csrc/traverse_kernel.hpp) are held to on tables of ties, with no tolerance at
all - for tests/test_build_ref_cpu.py (the restatement against the oracle wherever the oracle is defined, planted faults, the conditions on
the tables) and tests/test_gpu_build_ties.py (fed with what GpuIndex.knn_graph / select_edges / inter_insert / link / build return).  numpy
and fp64, plus the oracle front-end where noted; nothing here is fitted to device output.

The oracle cannot be the reference on tables of ties: its header says the reference's std::sort on Neighbor is unstable and that the oracle
"agrees on tie-free inputs".  The device's rule is the stated one - everything is ordered by (distance, id) - so the reference is this
restatement of the documented rule (the comments of prune_kernel), and test_build_ref_cpu.py proves it equal to the oracle
on continuous tables, where no two distances are equal.

  knn_lists      per row the other rows by (distance, id) under the field's metric, the first K = min(knng, n - 1); self excluded BY ID.
  select_edge    SyncPrune's sort + SelectEdge: L2 keys; sort by (dist, id); where more than PRUNE_POOL keys arrive the PRUNE_POOL smallest,
                 repeats counted; repeated (dist, id) dropped; the depth limit passes the positions 0 .. depth of that list, THE NODE'S OWN
                 INCLUDED when it is there (nsg.cpp:557-567, 655-685: depth candidates when the node is in its pool, depth + 1 when it is
                 not); the node is dropped wherever it sorts; the first candidate is kept; p is kept iff no kept r has d(r, p) < d(v, p);
                 stop at R kept.  depth <= 0: unlimited, and then everything is kept when the candidates fit into R.
  inter_insert   per node select_edge(unlimited) over its own edges and every offer v of an edge v -> u.
  nav_node       the smallest id among the rows closest to the centroid, for tables whose centroid is exact.
  check_link_lists   the properties of a Link result that need no restatement of its search.

Tie tables are walk_ref's (integers in [-v, v], / 16 under COSINE) plus the clustered and the paired tables below: every product and every
partial sum of a distance is a multiple of 1/256 below 2^24, so fp32 computes it exactly in any summation order, and fp64 computes the same
value from the Gram matrix."""
import numpy as np

import exact_ref as xr
import walk_ref as wr

F = np.float32
PRUNE_POOL = 4096          # keys of prune_kernel's pool (csrc/graph_host.hpp), restated
TIE_FLOOR = wr.TIE_FLOOR
METRIC_NAMES = wr.METRIC_NAMES


# ------------------------------------------------------------------------------------------------ distances
_GRID = {}


def on_grid(X):
    """integers / 16 of small magnitude: fp64 evaluates any sum of products of such values exactly, in any form.  (Answered once per array:
    the tables are not written to after they are made.)"""
    X = np.asarray(X)
    hit = _GRID.get(id(X))
    if hit is not None and hit[0] is X:
        return hit[1]
    s = X.astype(np.float64) * 16.0
    ok = bool((s == np.rint(s)).all() and np.abs(s).max(initial=0.0) < 2.0 ** 20)
    _GRID[id(X)] = (X, ok)
    return ok


def pair_dist(X, a, b, metric=0):
    """fp64 distances [len(a)][len(b)] between the rows a and the rows b.  On a grid table from the Gram matrix (exact, and seconds where the
    term-by-term form takes minutes); otherwise exact_ref.dist64 itself."""
    A, B = np.asarray(X)[np.asarray(a, np.int64)].astype(np.float64), np.asarray(X)[np.asarray(b, np.int64)].astype(np.float64)
    if not len(A) or not len(B):
        return np.zeros((len(A), len(B)))
    if not on_grid(X):
        return xr.dist64(A, B, metric)
    G = A @ B.T
    if metric == 0:
        return (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * G
    return 1.0 - G if metric == 1 else -G


def _order(dist, ids, descending_ids=False):
    """positions in (dist, id) order"""
    ids = np.asarray(ids, np.int64)
    return np.lexsort((-ids if descending_ids else ids, dist))


# ------------------------------------------------------------------------------------------------ kNN lists
def knn_lists(X, metric, K, rows=None, block=1024):
    """(ids [m][K], distances [m][K]) of the rows `rows` (None: all), K = min(K, n - 1): the other rows by (distance, id)"""
    X = np.asarray(X)
    n = len(X)
    K = min(int(K), n - 1)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    ids = np.empty((len(rows), K), np.int64)
    dist = np.empty((len(rows), K), np.float64)
    allr = np.arange(n, dtype=np.int64)
    for r0 in range(0, len(rows), block):
        blk = rows[r0:r0 + block]
        D = pair_dist(X, blk, allr, metric)                    # [b][n]
        D[np.arange(len(blk)), blk] = np.inf                   # the row itself leaves by id, whatever its distance
        for i in range(len(blk)):
            part = np.flatnonzero(D[i] <= np.partition(D[i], K - 1)[K - 1])   # the K smallest with every tie of the K-th
            o = part[_order(D[i][part], part)][:K]
            ids[r0 + i], dist[r0 + i] = o, D[i][o]
    return ids, dist


# ------------------------------------------------------------------------------------------------ SelectEdge
class Pool:
    """A node's candidate list as prune_kernel sees it: sorted by (dist, id), cut to the PRUNE_POOL smallest keys (repeats counted), repeats
    dropped; the node itself still in it."""

    def __init__(self, X, v, cands, descending_ids=False, first_arrivals=False, keep_repeats=False):
        c = np.asarray(cands, np.int64).ravel()
        c = c[c >= 0]
        if first_arrivals:                                   # planted fault: the pool keeps whatever came first
            c = c[:PRUNE_POOL]
        dv = pair_dist(X, [v], c, 0)[0] if len(c) else np.zeros(0)
        o = _order(dv, c, descending_ids)[:PRUNE_POOL]
        c, dv = c[o], dv[o]
        if len(c) and not keep_repeats:
            keep = np.r_[True, c[1:] != c[:-1]]              # (equal ids have equal distances: a repeated key is a repeated id next to itself)
            c, dv = c[keep], dv[keep]
        self.X, self.v, self.ids, self.dv, self._rows = X, int(v), c, dv, {}

    def row(self, i):
        """distances from pool entry i to every pool entry"""
        if i not in self._rows:
            self._rows[i] = pair_dist(self.X, [self.ids[i]], self.ids, 0)[0]
        return self._rows[i]


def select_from_pool(pool, depth, R, strict=True, keep_self=False, depth_shift=0):
    """the walk over a Pool; strict / keep_self / depth_shift: the planted faults of test_build_ref_cpu.py"""
    ids, dv = pool.ids, pool.dv
    pos = np.arange(len(ids))
    if depth > 0:
        pos = pos[:depth + 1 + depth_shift]                  # the positions 0 .. depth, the node's own among them
    if not keep_self:
        pos = pos[ids[pos] != pool.v]
    if depth <= 0 and len(pos) <= R:
        return ids[pos].copy()
    kept = []
    from_kept = np.empty((min(R, len(pos)), len(ids)))       # row k: distances from the k-th kept entry to every pool entry
    for p in pos:
        if len(kept) >= R:
            break
        d_rp = from_kept[:len(kept), p]
        if ((d_rp < dv[p]) if strict else (d_rp <= dv[p])).any():
            continue
        if len(kept) < len(from_kept):
            from_kept[len(kept)] = pool.row(int(p))
        kept.append(int(p))
    return ids[kept].copy()


def select_edge(X, v, cands, depth, R):
    return select_from_pool(Pool(X, v, cands), depth, R)


# ------------------------------------------------------------------------------------------------ InterInsert
def offers_of(ids, deg):
    """per node the nodes v with an edge v -> node, in (v, position) order"""
    ids, deg = np.asarray(ids, np.int64), np.asarray(deg, np.int64)
    n, R = ids.shape
    valid = np.arange(R)[None, :] < deg[:, None]
    src = np.repeat(np.arange(n, dtype=np.int64), R).reshape(n, R)[valid]
    dst = ids[valid]
    o = np.argsort(dst, kind="stable")
    src, dst = src[o], dst[o]
    cut = np.searchsorted(dst, np.arange(n + 1))
    return [src[cut[u]:cut[u + 1]] for u in range(n)]


def inter_insert(X, ids, deg, R, nodes=None, **pool_faults):
    """(ids [n][R] -1 padded, deg [n]) after InterInsert; nodes: only these (the others come back empty)"""
    ids, deg = np.asarray(ids, np.int64), np.asarray(deg, np.int64)
    n = len(ids)
    off = offers_of(ids, deg)
    out = np.full((n, R), -1, np.int64)
    od = np.zeros(n, np.int64)
    for u in (range(n) if nodes is None else nodes):
        pool = Pool(X, u, np.r_[ids[u, :deg[u]], off[u]], **pool_faults)
        sel = select_from_pool(pool, 0, R)
        out[u, :len(sel)], od[u] = sel, len(sel)
    return out, od


def pool_sizes(ids, deg):
    """keys that arrive at every node's InterInsert pool: own edges + offers, repeats counted"""
    ids, deg = np.asarray(ids, np.int64), np.asarray(deg, np.int64)
    valid = np.arange(ids.shape[1])[None, :] < deg[:, None]
    return deg + np.bincount(ids[valid], minlength=len(ids))


# ------------------------------------------------------------------------------------------------ navigation node
def nav_node(X):
    """the smallest id among the rows of minimal |x - c|^2, c the centroid - defined for tables whose centroid is exact (integer sums that
    divide by n, below 2^24)"""
    X64 = np.asarray(X, np.float64)
    s = X64.sum(0)
    assert on_grid(X) and (np.abs(X64).sum(0) < 2.0 ** 24).all(), "not a table whose column sums fp32 adds exactly in any order"
    c = s / len(X64)
    assert (c * len(X64) == s).all() and (c.astype(F).astype(np.float64) == c).all(), "the centroid is not exact in fp32"
    d = ((X64 - c) ** 2).sum(1)
    return int(np.flatnonzero(d == d.min())[0]), d


# ------------------------------------------------------------------------------------------------ properties of a Link result
def check_link_lists(X, knn, ids, deg, R, what=""):
    """no self, no repeated id, no -1 inside deg; 1 <= deg <= R; the kept list in (dist, id) order; the MRNG rule among the kept, pair by
    pair; the first entry no farther than anything in the node's kNN row (the pool contains the row).  Returns the kept distances per node."""
    ids, deg = np.asarray(ids, np.int64), np.asarray(deg, np.int64)
    n = len(ids)
    assert ids.shape == (n, R) and deg.shape == (n,), (what, ids.shape, deg.shape)
    assert (deg >= 1).all() and (deg <= R).all(), "%s: degrees outside [1, %d]: nodes %s" % (what, R, np.flatnonzero((deg < 1) | (deg > R))[:8].tolist())
    dists = []
    for v in range(n):
        l = ids[v, :deg[v]]
        ctx = "%s node %d list %s" % (what, v, l.tolist())
        assert (ids[v, deg[v]:] == -1).all(), ctx + ": the tail is not -1"
        assert (l >= 0).all() and (l < n).all() and (l != v).all() and len(set(l.tolist())) == len(l), ctx + ": self, repeat or no id"
        dv = pair_dist(X, [v], l, 0)[0]
        key_ok = (dv[1:] > dv[:-1]) | ((dv[1:] == dv[:-1]) & (l[1:] > l[:-1]))
        assert key_ok.all(), ctx + " distances %s: not in (dist, id) order" % dv.tolist()
        pp = pair_dist(X, l, l, 0)
        bad = np.argwhere(np.triu(pp < dv[None, :], 1))      # i < j kept both, yet d(k_i, k_j) < d(v, k_j)
        assert len(bad) == 0, ctx + ": kept %d although kept %d is closer to it (%r) than the node is (%r)" % (l[bad[0][1]], l[bad[0][0]], pp[bad[0][0], bad[0][1]], dv[bad[0][1]])
        row = np.asarray(knn[v], np.int64)
        row = row[row >= 0]
        if len(row):
            assert dv[0] <= pair_dist(X, [v], row, 0)[0].min(), ctx + ": the first entry is farther than the node's closest kNN entry"
        dists.append(dv)
    return dists


def connected(off, nbr, nav):
    n = len(off) - 1
    seen = np.zeros(n, bool)
    seen[nav] = True
    todo = [int(nav)]
    while todo:
        x = todo.pop()
        for y in nbr[off[x]:off[x + 1]]:
            if not seen[y]:
                seen[y] = True
                todo.append(int(y))
    return bool(seen.all())


# ------------------------------------------------------------------------------------------------ tables
def tie_table(n, d, metric, seed=0, v=None):
    return wr.tie_table(n, d, 1, metric, seed, v)[0]


WIDE_DIMS = [1030, 2048, 4096, 6520]       # 6520: the widest row a build at out_degree 50 has the LDS for (163 840 bytes a workgroup)


def wide_table(n, d, seed):
    """the tie table of the wide-row cases.  At d = 6520 the distances between rows of {-1, 0, 1} spread so far that 100 neighbours out of
    600 rows hold too few equal ones (a share of 0.25 to 0.29, at the floor): that table is a quarter-width tie table four times side by
    side, so every distance is a multiple of 4 and every column still carries values."""
    if d < 6520:
        return tie_table(n, d, 0, seed=seed)
    assert d % 4 == 0
    return np.ascontiguousarray(np.tile(tie_table(n, d // 4, 0, seed=seed), (1, 4)))


def fine_table(n, d, seed):
    """the continuous stand-in for the comparisons with the fp32 oracle: multiples of 1/512 in [0, 1).  Every term of a distance is a multiple
    of 2^-18, every sum of up to 32 of them has at most 23 bits: the oracle's fp32 values ARE the fp64 values, so the two sides can differ
    only where the rule differs - and with 2^18 d levels equal distances are rare enough to be ruled out list by list (distinct())."""
    assert d <= 32
    return np.ascontiguousarray(np.random.default_rng([seed, n, d]).integers(0, 512, (n, d)).astype(F) / F(512))


def distinct(dists):
    return len(np.unique(dists)) == len(dists)


def runs_table(n, d, metric, run=140, seed=3):
    """runs of `run` identical rows (more than K + 1 = 101), shuffled: a row is then not among its own K + 1 best keys"""
    rng = np.random.default_rng([seed, n, d])
    base = rng.integers(-2, 3, ((n + run - 1) // run, d)).astype(F)
    X = np.repeat(base, run, axis=0)[:n][rng.permutation(n)]
    return np.ascontiguousarray(X / F(16) if metric == 1 else X)


CLUSTER_OFFSETS = 3        # non-zero offsets per row among the 16 centre columns, and as many among the further ones


def _sparse_offsets(rng, n, cols, nz):
    """[n][cols] of {-1, 0, 1}, exactly min(nz, cols) of a row non-zero, at random columns and signs"""
    O = np.zeros((n, cols), np.int64)
    nz = min(nz, cols)
    if nz:
        at = np.argsort(rng.random((n, cols)), axis=1)[:, :nz]
        O[np.arange(n)[:, None], at] = rng.choice([-1, 1], size=(n, nz))
    return O


def clustered_table(centres, per, d, metric, seed=5):
    """`centres` distinct centres in {-100, +100}^16, `per` rows each = the centre plus offsets in {-1, 0, 1}; d - 16 further columns of
    {-1, 0, 1}; rows shuffled.  The offsets are SPARSE (CLUSTER_OFFSETS non-zero per row in each of the two column groups): under the dot
    metrics the distance from a row to a mate is -(|c|^2 + c.o_i + c.o_j + o_i.o_j), and with dense offsets c.o_j spreads over dozens of
    values - a list of 23 or 100 mates then holds too few equal distances for the floor.  With three non-zero offsets c.o_j takes 4 values
    and o_i.o_j 7, so the mates' distances tie under every metric, while the distance between two centres (a column that differs by 200)
    is what it was.  Returns (X, cluster id per row)."""
    assert d >= 16 and centres <= 1 << 16
    rng = np.random.default_rng([seed, centres, per, d])
    codes = rng.choice(1 << 16, size=centres, replace=False)
    C = (((codes[:, None] >> np.arange(16)[None, :]) & 1) * 200 - 100).astype(np.int64)
    n = centres * per
    X = np.zeros((n, d), np.int64)
    X[:, :16] = np.repeat(C, per, axis=0) + _sparse_offsets(rng, n, 16, CLUSTER_OFFSETS)
    X[:, 16:] = _sparse_offsets(rng, n, d - 16, CLUSTER_OFFSETS)
    perm = rng.permutation(n)
    X, cl = X[perm].astype(F), np.repeat(np.arange(centres), per)[perm]
    return np.ascontiguousarray(X / F(16) if metric == 1 else X), cl


def clustered_lists(X, cl, metric):
    """(ids [n][per - 1], distances): every row's mates by exact (distance, id).  mates_closer() is the condition that makes this the kNN list."""
    n = len(X)
    order = np.argsort(cl, kind="stable")
    per = n // (cl.max() + 1)
    grp = order.reshape(-1, per)                                         # rows of every cluster, ascending id
    A = np.asarray(X, np.float64)[grp]                                   # [c][per][d]
    G = np.einsum("cid,cjd->cij", A, A)
    if metric == 0:
        sq = (A * A).sum(2)
        D = sq[:, :, None] + sq[:, None, :] - 2.0 * G
    else:
        D = 1.0 - G if metric == 1 else -G
    D[:, np.arange(per), np.arange(per)] = np.inf                        # the row itself leaves by id: last of its own order, then cut
    G = np.broadcast_to(grp[:, None, :], D.shape)
    o = np.lexsort((G, D), axis=-1)[:, :, :per - 1]                      # per row of a cluster: its mates by (dist, id)
    ids = np.empty((n, per - 1), np.int64)
    dist = np.empty((n, per - 1), np.float64)
    ids[grp] = np.take_along_axis(G, o, axis=-1)
    dist[grp] = np.take_along_axis(D, o, axis=-1)
    return ids, dist


def mates_closer(X, cl, metric, sample, seed=1):
    """on `sample` random rows: every mate is strictly closer than every outsider (fp64, exact)"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(X), size=min(sample, len(X)), replace=False)
    D = pair_dist(X, rows, np.arange(len(X)), metric)
    mate = cl[rows][:, None] == cl[None, :]
    return bool((np.where(mate, D, -np.inf).max(1) < np.where(mate, np.inf, D).min(1)).all())


def paired_table(n, d, seed=7):
    """+- row pairs around an integer centre c: the centroid is exactly c.  Returns (X, c)."""
    assert n % 2 == 0
    rng = np.random.default_rng([seed, n, d])
    c = rng.integers(-5, 6, d)
    e = rng.integers(-2, 3, (n // 2, d))
    X = np.concatenate([c + e, c - e])[rng.permutation(n)].astype(F)
    return np.ascontiguousarray(X), c


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def exact_in_fp32(X, metric):
    """every product and every partial sum of a distance between two rows stays below 2^24 in units of the table's grid: bounded through the
    largest magnitudes (L2: d (2m)^2, the dot metrics: d m^2, in units of 1/256 under COSINE's / 16)"""
    X = np.asarray(X, np.float64)
    assert on_grid(X), "not integers (/ 16)"
    unit = 16.0 if metric == 1 else 1.0
    assert (X * unit == np.rint(X * unit)).all(), "not on the metric's grid"
    m = np.abs(X * unit).max()
    worst = ((2 * m) ** 2 if metric == 0 else m * m) * X.shape[1] + (256 if metric == 1 else 0)
    return worst < 2.0 ** 24


def preconditions(X, metric, dist_lists, what=""):
    """1 the table is one fp32 computes exactly (exact_in_fp32);  2 at least TIE_FLOOR of the adjacent positions of the compared lists
    (dist_lists: one array of reference distances per list) hold equal distances.  A table that misses one is replaced, never the floor.
    Returns the tie share."""
    assert exact_in_fp32(X, metric), "%s: a product or partial sum can reach 2^24 - not a table fp32 computes exactly" % what
    share = wr.tie_share(dist_lists)
    assert share >= TIE_FLOOR, "%s: only %.3f of the adjacent positions are ties (floor %.2f) - change the TABLE, not the floor" % (what, share, TIE_FLOOR)
    return share


# ------------------------------------------------------------------------------------------------ the comparator
def assert_same_lists(got, gdeg, want, wdeg, X, what="", metric=0, nodes=None):
    """every node, position by position, no tolerance.  got / want: [m][R] -1 padded; gdeg / wdeg: [m] or None (the whole row)"""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if gdeg is not None:
        bad = np.flatnonzero(np.asarray(gdeg, np.int64) != np.asarray(wdeg, np.int64))
    else:
        bad = np.zeros(0, np.int64)
    diff = np.flatnonzero((got != want).any(1))
    first = sorted(set(bad.tolist()) | set(diff.tolist()))
    if first:
        i = first[0]
        v = i if nodes is None else int(nodes[i])
        pos = int(np.flatnonzero(got[i] != want[i])[0]) if (got[i] != want[i]).any() else -1
        g, w = got[i][got[i] >= 0], want[i][want[i] >= 0]
        raise AssertionError("%s: %d of %d lists differ; node %d, first difference at position %d\n  returned %s\n  distances %s\n  expected %s\n  distances %s" % (
            what, len(first), len(got), v, pos, g.tolist(), pair_dist(X, [v], g, metric)[0].tolist() if len(g) else [], w.tolist(),
            pair_dist(X, [v], w, metric)[0].tolist() if len(w) else []))


# ------------------------------------------------------------------------------------------------ the cases of the SelectEdge and InterInsert pins
SELECT_DIMS = [3, 16, 33, 100, 768]
SELECT_POOLS = [1, 2, 5, 64, 420, 2048, 4096]
SELECT_DEPTHS = [0, 1, 40, 300]
SELECT_RS = [1, 4, 5, 8, 50, 512]
SELECT_N = 6000
TWIN, TWINS = 7, np.arange(100, 140)       # rows 100 .. 139 are copies of row 7: candidates at distance 0 of their node
POOL_SHAPES = ["plain", "node", "node x3", "repeats", "holes+node", "one distance", "twins", "drawn with repeats"]
_SELECT = {}


def select_table(d, metric=0):
    key = (d, metric)
    if key not in _SELECT:
        X = tie_table(SELECT_N, d, metric, seed=11).copy()
        X[TWINS] = X[TWIN]
        X.setflags(write=False)
        _SELECT[key] = X
    return _SELECT[key]


def select_pools(X, cpn, seed=0):
    """(nodes [8], cands [8][cpn], shape names): one pool per POOL_SHAPES entry.  Pools WITHOUT the node: plain, repeats, one distance,
    drawn with repeats; with it once: node, holes+node, twins; several times: node x3."""
    n = len(X)
    rng = np.random.default_rng([seed, cpn, X.shape[1]])
    nodes = rng.choice(np.arange(200, n), size=len(POOL_SHAPES), replace=False).astype(np.int64)
    nodes[6] = TWIN
    cands = np.full((len(POOL_SHAPES), cpn), -1, np.int64)
    for i, v in enumerate(nodes):
        others = np.setdiff1d(np.arange(n), [v])
        c = rng.choice(others, size=cpn, replace=False)
        shape = POOL_SHAPES[i]
        if shape in ("node", "holes+node"):
            c[rng.integers(cpn)] = v
        if shape == "node x3":
            c[rng.integers(cpn, size=3)] = v
        if shape == "repeats" and cpn >= 2:
            c[cpn // 2:2 * (cpn // 2)] = c[:cpn // 2]
            c = c[rng.permutation(cpn)]
        if shape == "holes+node" and cpn >= 5:
            c[rng.choice(cpn, size=cpn // 5, replace=False)] = -1
            if not (c == v).any():
                c[rng.integers(cpn)] = v
        if shape == "one distance":
            dv = pair_dist(X, [v], others, 0)[0]
            vals, cnt = np.unique(dv, return_counts=True)
            level = others[dv == vals[np.argmax(cnt)]][:cpn]
            c = np.r_[level, np.full(cpn - len(level), -1, np.int64)][rng.permutation(cpn)]
        if shape == "twins":
            k = min(len(TWINS), max(cpn - 1, 0))
            c[:k] = TWINS[:k]
            c[-1] = v if cpn > 1 else c[-1]
            if cpn >= 4:
                c[k:k + 2] = TWINS[:2] if k + 2 < cpn else c[k:k + 2]    # two of them twice
            c = c[rng.permutation(cpn)]
        if shape == "drawn with repeats":
            c = rng.choice(others[:max(cpn // 2, 1)], size=cpn, replace=True)
        cands[i] = c
    return nodes, cands, list(POOL_SHAPES)


def select_params():
    return [(depth, R) for depth in SELECT_DEPTHS for R in SELECT_RS]


HUB_N, HUB_D, HUB_R = 6000, 16, 50


def hub_lists():
    """every node's single edge points at node 0 (node 0's at node 1): node 0 receives 5999 offers next to its own edge"""
    X = tie_table(HUB_N, HUB_D, 0, seed=13)
    ids = np.full((HUB_N, HUB_R), -1, np.int64)
    ids[:, 0] = 0
    ids[0, 0] = 1
    return X, ids, np.ones(HUB_N, np.int64)


LINK_N, LINK_D, LINK_K = 3000, 16, 30
_LINK = {}


def link_lists(R):
    """(X, ids, deg): SelectEdge(depth 300) over every node's exact kNN row of a tie table - edge lists as Link leaves them"""
    if R not in _LINK:
        X = tie_table(LINK_N, LINK_D, 0, seed=17)
        if "knn" not in _LINK:
            _LINK["knn"] = knn_lists(X, 0, LINK_K)[0]
        ids = np.full((LINK_N, R), -1, np.int64)
        deg = np.zeros(LINK_N, np.int64)
        for v in range(LINK_N):
            sel = select_edge(X, v, _LINK["knn"][v], 300, R)
            ids[v, :len(sel)], deg[v] = sel, len(sel)
        _LINK[R] = (X, ids, deg)
    return _LINK[R]


# ------------------------------------------------------------------------------------------------ the clustered tables of the matrix path
CLUSTER_CASES = [(659, 101, 16), (659, 101, 72), (2774, 24, 16)]      # (centres, rows per centre, d): 66 559 / 66 559 / 66 576 rows, a partial last block


def accumulator_gap(xi, acc0, qi, cl, rows):
    """8-bit accumulators dot(xi, qi) + acc0 of the queries `rows` (rows of the table themselves) against every row: per query the smallest
    among its mates (itself included) minus the largest among the outsiders.  > 0: the rows taken by approximate key hold every mate as
    long as a cluster has no more rows than are taken."""
    acc = qi.astype(np.int64) @ xi.astype(np.int64).T + np.asarray(acc0, np.int64)[None, :]
    mate = cl[np.asarray(rows)][:, None] == cl[None, :]
    return np.where(mate, acc, np.iinfo(np.int64).max).min(1) - np.where(mate, np.iinfo(np.int64).min, acc).max(1)
