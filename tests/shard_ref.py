"""What the hash-sharded index (eps_index_create_sharded; csrc/shard_group.cpp, csrc/shard_host.hpp) is held to, in numpy, and the list of cases
the device is asked (CASES): tests/test_shard_ref_cpu.py holds this model to tests/exact_ref.py and shows that every planted fault changes the
answer of some case; tests/test_gpu_shard_ties.py feeds the same cases to a shard group, to one plain index and to G plain indices.

The model restates the group step by step: the hash split of the caller's memory - rows (attach and appends), the deleted bitset bit by bit, a
strided filter column, packed attribute rows - addressed the way the shards address it (base + l * pitch into the caller's flat buffer); per shard
the exact top-k of its visible rows by (ordinal of the fp32 distance as make_key orders it: -0 = +0, every NaN one ordinal above +inf; then the
GLOBAL id l * G + s), padded with -1 / +inf; the k-way merge of the G lists by the same key, padded again, with counts.  Rows are exact_ref's
exact tables (small integers: fp32 computes every distance exactly in any order), so every comparison is equality of ids, of distance bits and of
counts.  `fault=` plants one named mistake (FAULTS)."""
import numpy as np

import exact_ref as er
import merge_ref as mr

F = np.float32
METRIC_TABLE = {0: "integers -8..8", 1: "integers / 16", 2: "integers -8..8"}
OPS = ("<", "<=", "==", ">=", ">", "!=")
FAULTS = ("append_first", "bit_order", "local_ids", "tie_by_shard", "nan_raw", "pad_is_row", "counts_shard0", "no_pad_short")


# ------------------------------------------------------------------------------------------------ the split
def rows_of(s, n, G):
    return (n - s + G - 1) // G if n > s else 0


def append_span(s, n0, n_new, G, fault=None):
    """(first, count): shard s takes rows first, first + G, ... of a block of n_new rows appended to a table of n0 rows"""
    first = (s - n0) % G
    count = (n_new - first + G - 1) // G if n_new > first else 0
    if fault == "append_first":
        first += 1
    return first, count


def split_rows(n0, appends, G, fault=None):
    """per shard the SOURCE row held at each local position, after attach(n0) and the appends (lengths), as the shards copy them: row l of the
    block at base + l * pitch"""
    src = [np.arange(s, n0, G, dtype=np.int64) for s in range(G)]
    n = n0
    for m in appends:
        for s in range(G):
            first, count = append_span(s, n, m, G, fault)
            rows = n + first + G * np.arange(count, dtype=np.int64)
            src[s] = np.concatenate([src[s], np.minimum(rows, n + m - 1)])   # (a planted fault may step off the block: its last row then)
        n += m
    return src


def split_bits(bits, n, s, G, fault=None):
    """the shard's packed bitset: local bit l = bit l * G + s of the table's, least significant bit first"""
    ns = rows_of(s, n, G)
    out = np.zeros((ns + 7) // 8, np.uint8)
    for l in range(ns):
        i = l * G + s
        bit = (7 - (i & 7)) if fault == "bit_order" else (i & 7)
        if (int(bits[i >> 3]) >> bit) & 1:
            out[l >> 3] |= np.uint8(1 << (l & 7))
    return out


def unpack(bits, n):
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:n].astype(bool)


def split_column(buf, stride, width, n, s, G):
    """the shard's values of a column whose row i holds a signed `width`-byte integer at buf[i * stride]: base + s * stride, pitch G * stride"""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    ns = rows_of(s, n, G)
    base, pitch = s * stride, G * stride
    out = np.empty(ns, np.int64)
    for l in range(ns):
        out[l] = int.from_bytes(buf[base + l * pitch: base + l * pitch + width].tobytes(), "little", signed=True)
    return out


def split_attr(buf, stride, n_rows, s, G):
    """the shard's attribute rows, packed at `stride`: count rows of `stride` bytes read at pitch G * stride from base s * stride"""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    count = rows_of(s, n_rows, G)
    base, pitch = s * stride, G * stride
    return np.stack([buf[base + l * pitch: base + l * pitch + stride] for l in range(count)]) if count else np.zeros((0, stride), np.uint8)


def compare(values, op, constant):
    return {"<": values < constant, "<=": values <= constant, "==": values == constant, ">=": values >= constant, ">": values > constant,
            "!=": values != constant}[op]


# ------------------------------------------------------------------------------------------------ per shard, then merged
def _keys(d32, ids):
    return (mr.ordinal(d32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)   # (ids below 2^32 here)


def topk_lists(d32, ids, visible, k):
    """d32 [rows][nq], ids [rows] (>= 0), visible [rows] -> (ids [nq][k], dist [nq][k], counts [nq]) by (ordinal, id), -1 / +inf padded"""
    nq = d32.shape[1]
    out_ids, out_dist = np.full((nq, k), -1, np.int64), np.full((nq, k), np.inf, F)
    rows = np.flatnonzero(visible)
    m = min(k, len(rows))
    if m:
        keys = np.sort(_keys(d32[rows], np.broadcast_to(ids[rows, None], (len(rows), nq))), axis=0)[:m].T
        out_ids[:, :m] = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        out_dist[:, :m] = mr.ord2f((keys >> np.uint64(32)).astype(np.uint32))
    return out_ids, out_dist, np.full(nq, m, np.int32)


def merge(ids, dist, k, fault=None, shard_counts=None):
    """ids / dist [G][nq][k] -> (ids [nq][k], dist [nq][k], counts [nq]): the k smallest of the lists' rows by (ordinal, id); an id < 0 ends a list"""
    G, nq, _ = ids.shape
    O = mr.ordinal(dist).astype(np.uint64)
    live = np.ones(ids.shape, bool) if fault == "pad_is_row" else np.cumprod(ids >= 0, axis=2).astype(bool)
    if fault == "tie_by_shard":
        low = np.broadcast_to((np.arange(G, dtype=np.uint64)[:, None, None] << np.uint64(20)) | np.arange(k, dtype=np.uint64)[None, None, :], ids.shape)
    else:
        low = (ids + 1).astype(np.uint64)      # (ids below 2^32 - 1 here; a padding -1 that a fault lets in orders in front of every row)
    key = np.where(live, (O << np.uint64(32)) | low, np.uint64(0xFFFFFFFFFFFFFFFF))
    flat = lambda a: a.transpose(0, 2, 1).reshape(G * k, nq)      # noqa: E731
    order = np.argsort(flat(key), axis=0, kind="stable")[:k]
    took = np.take_along_axis(flat(live), order, 0).T
    out_ids = np.where(took, np.take_along_axis(flat(ids), order, 0).T, -1).astype(np.int64)
    out_dist = np.where(took, mr.ord2f(np.take_along_axis(flat(O), order, 0).T.astype(np.uint32)), F(np.inf)).astype(F)
    counts = took.sum(axis=1).astype(np.int32)
    if fault == "nan_raw":
        for q in np.flatnonzero(np.isnan(dist).any(axis=(0, 2))):
            got = _merge_raw_floats(ids[:, q], dist[:, q], k)
            out_ids[q], out_dist[q], counts[q] = -1, np.inf, len(got)
            for e, (i, d) in enumerate(got):
                out_ids[q, e], out_dist[q, e] = i, d
    if fault == "counts_shard0":
        counts = np.asarray(shard_counts[0], np.int32).copy()
    return out_ids, out_dist, counts


def _merge_raw_floats(ids, dist, k):
    """the planted fault: heads compared with `<` on the floats, where every comparison with a NaN is false"""
    G = len(ids)
    head, got = [0] * G, []
    for _ in range(k):
        best = -1
        for s in range(G):
            if head[s] >= k or ids[s, head[s]] < 0:
                continue
            d, i = dist[s, head[s]], ids[s, head[s]]
            if best < 0 or d < dist[best, head[best]] or (d == dist[best, head[best]] and i < ids[best, head[best]]):
                best = s
        if best < 0:
            break
        got.append((int(ids[best, head[best]]), dist[best, head[best]]))
        head[best] += 1
    return got


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """one table and what is asked of it.  n: rows attached first; appends: lengths appended after (every stage is compared); ks; deleted / column:
    names resolved by data(); program: "plain" | "longer" (attribute rows for ATTR_EXTRA more rows than the table holds); nan: {row: value} planted in column 0; repeat: every distinct vector 2G + 1 times at consecutive ids"""

    def __init__(self, kind, G, n, metric, nq, ks, d=8, appends=(), deleted=None, column=None, nan=None, repeat=False, program=None, seed=0):
        self.kind, self.G, self.n, self.metric, self.nq, self.d, self.seed = kind, G, n, metric, nq, d, seed
        self.ks = tuple(sorted({k for k in ks if k > 0}))
        self.appends, self.deleted, self.column, self.nan, self.repeat, self.program = tuple(appends), deleted, column, nan, repeat, program
        self.total = n + sum(self.appends)

    @property
    def name(self):
        extra = [str(v) for v in (self.deleted, self.column, self.program, "nan" if self.nan else None, "+".join(map(str, self.appends)) if self.appends else None) if v]
        return "%s G%d n%d m%d nq%d%s" % (self.kind, self.G, self.n, self.metric, self.nq, (" " + " ".join(extra)) if extra else "")

    def stages(self):
        """row counts at which the table is searched: after the attach and after every append"""
        return list(np.cumsum((self.n,) + self.appends))


# packed attribute rows of the filter program: 24 bytes a row
ATTR = np.dtype([("a", "<i4"), ("p", "<f4"), ("b", "u1"), ("pad", "V7"), ("x", "<f8")])
ATTR_EXTRA = 5
PROGRAM = [("i32", 0), ("const", 3), ("%",), ("const", 1), ("=",), ("f32", 4), ("const", 0.5), ("<",), ("and",),
           ("i8", 8), ("const", 2), ("=",), ("f64", 16), ("const", 0.0), (">=",), ("and",), ("or",)]


def program_mask(rows):
    """PROGRAM over structured rows: (a % 3 = 1 and p < 0.5) or (b = 2 and x >= 0); % is fmod"""
    return ((np.fmod(rows["a"], 3) == 1) & (rows["p"] < 0.5)) | ((rows["b"] == 2) & (rows["x"] >= 0))


def attr_rows(case, n):
    """the caller's attribute rows for a table of n rows (+ ATTR_EXTRA for "longer"): exactly that many rows of 24 bytes"""
    m = n + (ATTR_EXTRA if case.program == "longer" else 0)
    rng = np.random.default_rng([case.seed, 99])
    big = case.total + ATTR_EXTRA
    rows = np.zeros(big, ATTR)
    rows["a"], rows["p"] = rng.integers(-50, 51, big), rng.integers(0, 9, big) / F(8)
    rows["b"], rows["x"] = rng.integers(0, 4, big), rng.integers(-8, 9, big) / 4.0
    return rows[:m].copy()


# filter columns: (width, stride, offset into the record)
COLUMNS = {"i8": (1, 1, 0), "i16": (2, 2, 0), "i32": (4, 4, 0), "i64": (8, 8, 0), "rec12": (4, 12, 4)}
_DATA = {}


def data(case):
    """everything a case is made of, from its fields alone (cached, never changed): X [total][d], Q, ref (exact_ref.Ref over all rows), per stage n:
    bits(n) the caller's deleted bitset of exactly ceil(n / 8) bytes (or None), the column record buffer of exactly (n - 1) * stride + width bytes
    behind `offset`, visible(n) from the WHOLE table's point of view"""
    if case in _DATA:
        return _DATA[case]
    G, total, d = case.G, case.total, case.d
    if case.repeat:
        rep = 2 * G + 1
        base, Q = er.make(METRIC_TABLE[case.metric], (total + rep - 1) // rep, d, case.nq, seed=case.seed)
        X = np.repeat(base, rep, axis=0)[:total].copy()
    else:
        X, Q = er.make(METRIC_TABLE[case.metric], total, d, case.nq, seed=case.seed)
        X = X.copy()
    for row, value in (case.nan or {}).items():
        X[row, 0] = value
    with np.errstate(invalid="ignore", over="ignore"):      # (planted inf / NaN rows)
        out = {"X": X, "Q": Q, "ref": er.Ref(X, Q, case.metric) if total and case.nq else None}
    rng = np.random.default_rng([case.seed, total, G, 77])
    values = rng.integers(-100, 101, total)
    if G > 1:
        values[1::G] = -np.abs(values[1::G])      # shard 1 holds no positive value: `> 0` passes nothing there, `> 100` nothing anywhere
    out["values"] = values
    _DATA[case] = out
    return out


def deleted_bits(case, n):
    """the caller's bitset for a table of n rows: exactly ceil(n / 8) bytes"""
    G, spec = case.G, case.deleted
    if spec is None:
        return None
    dead = np.zeros((n + 7) // 8 * 8, bool)
    if spec.startswith("class"):            # every row of one residue class: that shard has no visible row, the others no deletion
        dead[int(spec[5:]):n:G] = True
    elif spec == "but3same":                # all rows deleted but three on the same shard
        dead[:n] = True
        dead[[1, 1 + G, n - 1 - ((n - 2) % G)]] = False
    elif spec == "but3diff":                # ... but three on different shards
        dead[:n] = True
        dead[[0, 1 + G, 2 + 2 * G]] = False
    elif spec == "last":
        dead[n - 1] = True
    elif spec == "beyond":                  # bits set beyond n in the last byte (and a few rows)
        dead[n:] = True
        dead[[3, n - 2]] = True
    elif spec == "random":
        dead[:n] = np.random.default_rng([case.seed, n]).random(n) < 0.4
    else:
        raise KeyError(spec)
    return np.packbits(dead, bitorder="little")


def column_buffer(case, n):
    """(record buffer uint8, offset, stride, width, op, constant): the buffer ends with the last row's value"""
    name, op, constant = case.column
    width, stride, offset = COLUMNS[name]
    values = data(case)["values"][:n]
    buf = np.full(offset + (n - 1) * stride + width if n else 0, 0xEE, np.uint8)
    for i in range(n):
        buf[offset + i * stride: offset + i * stride + width] = np.frombuffer(int(values[i]).to_bytes(width, "little", signed=True), np.uint8)
    return buf, offset, stride, width, op, constant


def visible(case, n):
    """the WHOLE table's visible rows at n rows, without any split"""
    vis = np.ones(n, bool)
    bits = deleted_bits(case, n)
    if bits is not None:
        vis &= ~unpack(bits, n)
    if case.column:
        vis &= compare(data(case)["values"][:n], case.column[1], case.column[2])
    if case.program:
        vis &= program_mask(attr_rows(case, n)[:n])
    return vis


def shard_visible(case, n, fault=None):
    """per shard the visible local rows, through the split of the caller's buffers"""
    G = case.G
    out = [np.ones(rows_of(s, n, G), bool) for s in range(G)]
    bits = deleted_bits(case, n)
    if bits is not None:
        for s in range(G):
            out[s] &= ~unpack(split_bits(bits, n, s, G, fault), len(out[s]))
    if case.column:
        buf, offset, stride, width, op, constant = column_buffer(case, n)
        for s in range(G):
            out[s] &= compare(split_column(buf[offset:], stride, width, n, s, G), op, constant)
    if case.program:
        rows = attr_rows(case, n)
        for s in range(G):
            mine = split_attr(rows.view(np.uint8), ATTR.itemsize, len(rows), s, G)
            out[s] &= program_mask(np.ascontiguousarray(mine).view(ATTR).reshape(-1))[:len(out[s])]
    return out


def model(case, k, stage=-1, fault=None):
    """the group's answer at stage `stage` of the case: (ids [nq][k], dist [nq][k], counts [nq], per-shard lists)"""
    G = case.G
    dd = data(case)
    st = case.stages()
    n = int(st[stage])
    n_app = len(st) - 1 if stage < 0 else stage
    src = split_rows(case.n, case.appends[:n_app], G, fault)
    vis = shard_visible(case, n, fault)
    d32 = dd["ref"].d64.astype(F)
    lists = []
    for s in range(G):
        local = np.arange(len(src[s]), dtype=np.int64)
        gid = local if fault == "local_ids" else local * G + s
        lists.append(topk_lists(d32[src[s]], gid, vis[s], k))
    ids, dist = np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists])
    counts = [l[2] for l in lists]
    if fault == "no_pad_short":        # the tail of a short list keeps what the buffer held: zeros read as (row 0, distance 0)
        short = ids < 0
        ids, dist = np.where(short, 0, ids), np.where(short, F(0), dist)
    return merge(ids, dist, k, fault, counts) + ((ids, dist),)


def whole_table(case, k, stage=-1):
    """the answer of the unsharded table by the flat contract: visible rows by (ordinal, id), NaN rows last in id order"""
    n = int(case.stages()[stage])
    d32 = data(case)["ref"].d64[:n].astype(F)
    return topk_lists(d32, np.arange(n, dtype=np.int64), visible(case, n), k)


def same(a, b, what=""):
    """ids, distance bits, counts"""
    for x, y, name in zip(a[:3], b[:3], ("ids", "dist", "counts")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "dist":
            x, y = mr.bits(x), mr.bits(y)
        assert x.shape == y.shape, "%s %s: shapes %s %s" % (what, name, x.shape, y.shape)
        bad = np.argwhere(x != y)
        assert len(bad) == 0, "%s %s: %d places differ, first %s: %r != %r" % (what, name, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def differs(a, b):
    return any(not np.array_equal(np.asarray(x) if i != 1 else mr.bits(x), np.asarray(y) if i != 1 else mr.bits(y)) for i, (x, y) in enumerate(zip(a[:3], b[:3])))


EDGE_GS = (1, 2, 3, 5, 8, 16)


def edge_ns(G):
    return sorted({n for n in (1, G - 1, G, G + 1, 8 * G - 1, 8 * G + 1, 1003) if n > 0})


def _cases():
    out = []
    # a. split edges
    for G in EDGE_GS:
        for n in edge_ns(G):
            for metric in (0, 1, 2):
                for nq in (1, 129):
                    out.append(Case("edges", G, n, metric, nq, (1, 10, n, n + 3), seed=1))
    # b. ties across shards: every distinct vector 2G + 1 times at consecutive ids; k inside a tie group
    for G in (2, 3, 5):
        for metric in (0, 1, 2):
            out.append(Case("ties", G, 40 * (2 * G + 1) + 1, metric, 9, (G, 2 * G + 2, 3 * G + 1, 2 * (2 * G + 1) + 1), repeat=True, seed=2))
    # c. the deleted bitset
    for G in (3, 5):
        for spec in ("class1", "class%d" % (G - 1), "but3same", "but3diff", "last", "beyond"):
            out.append(Case("deleted", G, 1003, 0, 5, (10,), deleted=spec, seed=3))
    # d. the column filter: every width, every operator; constants that empty one shard / the table are chosen in the GPU test from `values`
    for G in (3, 5):
        for i, name in enumerate(COLUMNS):
            for j, op in enumerate(OPS):
                out.append(Case("column", G, 1003, (0, 2)[(i + j) % 2], 3, (10,), column=(name, op, (-7, 0, 13)[(i + j) % 3]), seed=4))
        out.append(Case("column", G, 1003, 0, 3, (10,), column=("rec12", ">", 0), seed=4))       # passes nothing on shard 1
        out.append(Case("column", G, 1003, 0, 3, (10,), column=("i16", ">", 100), seed=4))       # passes nothing at all
    # e. the filter program over packed rows {i32, f32, u8, pad, f64}
    for prog in ("plain", "longer"):
        out.append(Case("program", 3, 1003, 0, 3, (10,), program=prog, seed=7))
    out.append(Case("program", 3, 1001, 0, 3, (10,), program="plain", appends=(2, 5, 12), seed=7))       # (the append_only flow)
    # f. appends: n0 mod G != 0, then 1, 1, G - 1, G + 1, 0, 37 rows
    for G in (2, 3, 5):
        out.append(Case("append", G, 1001, 0, 4, (10,), appends=(1, 1, G - 1, G + 1, 0, 37), seed=5))
    out.append(Case("append", 3, 2, 2, 4, (10,), appends=(1, 1, 2, 4, 0, 37), seed=5))      # (from a table shorter than G)
    # i. NaN / inf rows on different shards: last, in id order
    for G in (3, 5):
        for metric in (0, 1, 2):
            nan = {0: np.nan, 1: np.inf, G + 2: np.nan, 2 * G + 1: -np.inf, 50: np.nan}
            out.append(Case("nan", G, 53, metric, 3, (10, 48, 53, 60), nan=nan, seed=6))
    return out


CASES = _cases()
SHORT = [c for c in CASES if c.kind == "edges" and c.n < 8 * c.G - 1]       # "short shard" cases: some shard holds fewer rows than some k
EMPTY = [c for c in SHORT if c.n < c.G]                                      # ... and some shard holds none
