"""The hash-sharded index (eps_index_create_sharded; csrc/shard_group.cpp, host arithmetic csrc/shard_host.hpp) held to an exact reference on tables
of ties.  All shards run on device 0 (devices=[0] * G), one process.  Rows are exact_ref's exact tables (small integers: fp32 computes every
distance exactly in any order), so there is no tolerance anywhere: every comparison is equality of ids, of distance BITS and of counts.

Every answer of a group is compared with all three of
  1 the whole table's exact answer (exact_ref.check_exact; the NaN / inf tables, which check_exact refuses by design, with shard_ref.whole_table:
    the flat contract of DESIGN 3.3 stated without a split),
  2 one plain GpuIndex over the whole table,
  3 G plain indices over X[s::G] with set_id_map(s, G), searched with the same parameters and merged by amd.merge_topk.
The cases are tests/shard_ref.CASES, which tests/test_shard_ref_cpu.py shows to be strong enough (every planted fault of the model changes some
answer) and to be what they claim (ties across shards at the k-th place, all-zero bit slices, short and empty shards).

The groups and the plain indices are created once per module and re-attached per case: a group of 16 creates 16 indices and 16 worker threads."""
import os
import time

import numpy as np
import pytest

import exact_ref as er
import shard_ref as sh

pytestmark = pytest.mark.gpu
F = np.float32
USER, UNSUPPORTED = 30000, 50002


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


class Pool:
    """the module's indices: one group per (G, metric, d), one plain index and up to 16 shard-sized plain indices per (metric, d)"""

    def __init__(self, amd):
        self.amd, self.groups, self.plains = amd, {}, {}

    def group(self, G, metric, d=8, tag=""):
        key = (G, metric, d, tag)
        if key not in self.groups:
            t = time.perf_counter()
            self.groups[key] = self.amd.GpuIndex(d, metric, devices=[0] * G)
            print("shard-ties: a group of %d created in %.3f s" % (G, time.perf_counter() - t))
        return self.groups[key]

    def plain(self, metric, d=8, slot="one"):
        key = (metric, d, slot)
        if key not in self.plains:
            self.plains[key] = self.amd.GpuIndex(d, metric)
        return self.plains[key]

    def close(self):
        for ix in list(self.groups.values()) + list(self.plains.values()):
            ix.close()


@pytest.fixture(scope="module")
def pool(amd):
    p = Pool(amd)
    yield p
    p.close()


class Trio:
    """a group, one plain index and G plain shard indices over the same table; the plain sides are sliced with numpy, never with the group's arithmetic"""

    def __init__(self, pool, G, metric, d=8, tag=""):
        self.amd, self.G, self.metric, self.d = pool.amd, G, metric, d
        self.grp, self.one = pool.group(G, metric, d, tag), pool.plain(metric, d)
        self.parts = [pool.plain(metric, d, s) for s in range(G)]
        for s, ix in enumerate(self.parts):
            ix.set_id_map(s, G)
        self.X = None

    def everyone(self):
        return [self.grp, self.one] + self.parts

    def clear(self):
        for ix in self.everyone():
            ix.set_deleted(None)
            ix.set_int_filter(None, None, 0)
            ix.set_filter_program(None)

    def attach(self, X):
        self.X = np.ascontiguousarray(X, F)
        self.grp.attach_rows(self.X)
        self.one.attach_rows(self.X)
        self._parts_rows()
        self.clear()

    def _parts_rows(self):
        for s, ix in enumerate(self.parts):
            ix.attach_rows(np.ascontiguousarray(self.X[s::self.G]))

    def append(self, rows):
        rows = np.ascontiguousarray(rows, F).reshape(-1, self.d)
        self.grp.append_rows(rows)
        self.one.append_rows(rows)
        self.X = np.concatenate([self.X, rows])
        self._parts_rows()

    def set_deleted(self, bits, n=None):
        n = len(self.X) if n is None else n
        self.grp.set_deleted(bits)
        self.one.set_deleted(bits)
        dead = None if bits is None else sh.unpack(bits, n)
        for s, ix in enumerate(self.parts):
            ix.set_deleted(None if bits is None else np.packbits(dead[s::self.G], bitorder="little"))

    def set_column(self, buf, offset, stride, width, op, constant, values):
        for ix in (self.grp, self.one):
            ix.set_int_filter(buf, op, constant, stride=stride, width=width, offset=offset)
        for s, ix in enumerate(self.parts):
            ix.set_int_filter(np.ascontiguousarray(values[s::self.G], np.int64), op, constant)

    def set_program(self, rows, append_only=False):
        for ix in (self.grp, self.one):
            ix.set_filter_program(sh.PROGRAM, rows, append_only=append_only)
        for s, ix in enumerate(self.parts):
            ix.set_filter_program(sh.PROGRAM, np.ascontiguousarray(rows[s::self.G]))

    def search(self, Q, k, **kw):
        """(group, plain, merged parts): each (ids, dist, counts)"""
        kw.setdefault("mode", self.amd.MODE_FLAT)
        Q = np.ascontiguousarray(Q, F)
        g = self.grp.search(Q, k, **kw)
        o = self.one.search(Q, k, **kw)
        nq = len(Q)
        ids, dist = np.empty((self.G, nq, k), np.int64), np.empty((self.G, nq, k), F)
        for s, ix in enumerate(self.parts):
            ids[s], dist[s], _ = ix.search(Q, k, **kw)
        md, mi = self.amd.merge_topk(dist, ids, np.empty((nq, k), F), np.empty((nq, k), np.int64))
        return g, o, (mi, md, (mi >= 0).sum(axis=1).astype(np.int32))

    def held(self, case, k, stage=-1, what="", **kw):
        """one search of the case under all three comparisons"""
        dd = sh.data(case)
        n = int(case.stages()[stage])
        assert n == len(self.X)
        what = "%s stage %d k %d %s" % (case.name, stage, k, what)
        g, o, m = self.search(dd["Q"], k, **kw)
        sh.same(g, o, what + " [group vs one plain index]")
        sh.same(g, m, what + " [group vs G plain indices merged]")
        if case.nan:
            sh.same(g, sh.whole_table(case, k, stage), what + " [group vs the flat contract]")
        else:
            er.check_exact(g[0], g[1], g[2], dd["X"][:n], None, case.metric, k, visible=sh.visible(case, n), ref=_ref_rows(dd["ref"], n), what=what)
        return g


def _ref_rows(ref, n):
    if n == ref.n:
        return ref
    r = object.__new__(er.Ref)
    r.n, r.d, r.metric, r.nq = n, ref.d, ref.metric, ref.nq
    r.d64 = ref.d64[:n]
    r.mag = r.d64 if ref.metric == 0 else ref.mag[:n]
    return r


def _cases(kind, **where):
    return [c for c in sh.CASES if c.kind == kind and all(getattr(c, a) == v for a, v in where.items())]


def _code(f):
    """the call's status code (0: it went through) and its message"""
    import vectordb_amd
    try:
        f()
    except vectordb_amd.EpsillaError as e:
        return e.code, str(e)
    return 0, ""


# ------------------------------------------------------------------------------------------------ a. split edges
@pytest.mark.parametrize("G", sh.EDGE_GS)
def test_split_edges(pool, G):
    """n in {1, G-1, G, G+1, 8G-1, 8G+1, 1003} x k in {1, 10, n, n+3} x nq in {1, 129} x the three metrics, host buffers: empty shards, shards shorter
    than k, k beyond the table, the merge kernel's second block.  The G = 16 group is shared by all of its cases (16 indices are created once)."""
    cases = _cases("edges", G=G)
    assert len(cases) == len(sh.edge_ns(G)) * 3 * 2
    t = time.perf_counter()
    for metric in (0, 1, 2):
        trio = Trio(pool, G, metric)
        for c in (c for c in cases if c.metric == metric):
            trio.attach(sh.data(c)["X"])
            assert trio.grp.row_count == c.n
            for k in c.ks:
                trio.held(c, k)
    print("shard-ties: split edges G %2d: %d cases in %.2f s" % (G, len(cases), time.perf_counter() - t))


@pytest.mark.parametrize("G", [3, 16])
def test_empty_table_and_empty_batch_as_a_plain_index(pool, G):
    """n = 0 and nq = 0: the same code and the same output state as a plain index (results in caller-provided buffers that hold a sentinel)"""
    trio = Trio(pool, G, 0)
    X, Q = er.make("integers -8..8", 5, 8, 3, seed=9)
    for n, nq in ((0, 3), (0, 0), (5, 0)):
        trio.attach(X[:n])
        outs = []
        for ix in (trio.grp, trio.one):
            out = (np.full((nq, 4), -7, np.int64), np.full((nq, 4), -7, F), np.full(nq, -7, np.int32))
            code = _code(lambda: ix.search(Q[:nq].reshape(nq, 8), 4, out=out, mode=pool.amd.MODE_FLAT))[0]
            outs.append((code, out))
        assert outs[0][0] == outs[1][0] == 0, (n, nq, outs[0][0], outs[1][0])
        sh.same(outs[0][1], outs[1][1], "n %d nq %d" % (n, nq))
        if nq:
            assert (outs[0][1][0] == -1).all() and np.isposinf(outs[0][1][1]).all() and (outs[0][1][2] == 0).all()
        assert trio.grp.row_count == trio.one.row_count == n


# ------------------------------------------------------------------------------------------------ b. ties across shards
@pytest.mark.parametrize("G", [2, 3, 5])
def test_ties_across_shards(pool, G):
    """every distinct vector 2G + 1 times at consecutive ids: every shard holds copies, k cuts inside a tie group - the id alone decides the merge"""
    for c in _cases("ties", G=G):
        trio = Trio(pool, G, c.metric)
        trio.attach(sh.data(c)["X"])
        for k in c.ks:
            trio.held(c, k)


# ------------------------------------------------------------------------------------------------ c. the deleted bitset
@pytest.mark.parametrize("G", [3, 5])
def test_deleted_bitset(pool, G):
    """one residue class deleted (one shard without a visible row, the others on the no-deletions path), all but three rows on one shard / on three
    shards, only the last row, bits set beyond n in the last byte; then set_deleted(None)"""
    cases = _cases("deleted", G=G)
    assert len(cases) == 6
    trio = Trio(pool, G, 0)
    for c in cases:
        trio.attach(sh.data(c)["X"])
        bits = sh.deleted_bits(c, c.n)
        assert len(bits) == (c.n + 7) // 8
        trio.set_deleted(bits)
        g = trio.held(c, 10)
        if c.deleted.startswith("but3"):
            assert (g[2] == 3).all()
        trio.set_deleted(None)
        plain = sh.Case("deleted", G, c.n, c.metric, c.nq, c.ks, seed=c.seed)      # the same table, nothing deleted
        trio.held(plain, 10, what="after set_deleted(None)")


# ------------------------------------------------------------------------------------------------ d. the column filter
@pytest.mark.parametrize("G", [3, 5])
def test_column_filter(pool, G):
    """widths 1 / 2 / 4 / 8 with negative values and a 12-byte record with the value at offset 4 (the buffer ends with the last row's value), all six
    operators; a filter that passes nothing on shard 1 and one that passes nothing at all"""
    cases = _cases("column", G=G)
    assert len(cases) == 5 * 6 + 2
    for metric in (0, 2):
        trio = Trio(pool, G, metric)
        for c in (c for c in cases if c.metric == metric):
            trio.attach(sh.data(c)["X"])
            buf, offset, stride, width, op, constant = sh.column_buffer(c, c.n)
            trio.set_column(buf, offset, stride, width, op, constant, sh.data(c)["values"][:c.n])
            g = trio.held(c, 10)
            if c.column == ("i16", ">", 100):
                assert (g[2] == 0).all()
            if c.column == ("rec12", ">", 0):
                assert (g[0][g[0] >= 0] % G != 1).all()


# ------------------------------------------------------------------------------------------------ e. the filter program
def test_filter_program(pool):
    """packed rows {i32, f32, u8, pad, f64}, G = 3: plain; attribute rows longer than the table; append_only=True across three appends with a row
    edited in place between calls WITHOUT the flag - the edit must be seen"""
    G = 3
    trio = Trio(pool, G, 0)
    for c in _cases("program", appends=()):
        trio.attach(sh.data(c)["X"])
        trio.set_program(sh.attr_rows(c, c.n))
        trio.held(c, 10)
    (c,) = [c for c in _cases("program") if c.appends]
    dd = sh.data(c)
    st = [int(v) for v in c.stages()]
    rows = sh.attr_rows(c, c.total)            # ONE array all calls hand over a prefix of (the append-only promise is about this memory)
    trio.attach(dd["X"][:st[0]])
    trio.set_program(rows[:st[0]], append_only=True)
    trio.held(c, 10, stage=0)
    for stage in range(1, len(st)):
        trio.append(dd["X"][st[stage - 1]:st[stage]])
        trio.set_program(rows[:st[stage]], append_only=True)
        trio.held(c, 10, stage=stage, what="append_only")
    # an edit in place, handed over without the flag: rows that passed now fail, on every shard
    n = st[-1]
    vis = sh.visible(c, n)
    edit = np.flatnonzero(vis)[:3 * G]
    assert len({int(i) % G for i in edit}) == G
    edited = rows.copy()
    edited["a"][edit], edited["b"][edit] = 0, 0
    rows[:] = edited                           # (the same memory)
    assert not sh.program_mask(rows[edit]).any()
    trio.set_program(rows[:n], append_only=False)
    g, o, m = trio.search(dd["Q"], 10)
    sh.same(g, o, "edited rows [group vs one plain index]")
    sh.same(g, m, "edited rows [group vs G plain indices merged]")
    vis2 = sh.program_mask(rows[:n])
    assert vis2.sum() == vis.sum() - len(edit)
    er.check_exact(g[0], g[1], g[2], dd["X"][:n], None, c.metric, 10, visible=vis2, ref=dd["ref"], what="edited rows")


# ------------------------------------------------------------------------------------------------ f. appends
@pytest.mark.parametrize("c", _cases("append"), ids=lambda c: c.name.replace(" ", "_"))
def test_appends(pool, c):
    """attach n0 (n0 mod G != 0, or n0 < G), then append 1, 1, G - 1, G + 1, 0, 37 rows: compared after each"""
    dd = sh.data(c)
    st = [int(v) for v in c.stages()]
    trio = Trio(pool, c.G, c.metric)
    trio.attach(dd["X"][:st[0]])
    trio.held(c, 10, stage=0)
    for stage in range(1, len(st)):
        trio.append(dd["X"][st[stage - 1]:st[stage]])
        assert trio.grp.row_count == st[stage]
        trio.held(c, 10, stage=stage)


@pytest.mark.parametrize("G", [3, 5])
def test_filters_set_before_an_append_are_refused_by_name(pool, G):
    """a bitset / column / program of the old length: the group refuses the search with EPS_USER_ERROR and names the call to repeat, as the plain
    index does; after that call the answer is right"""
    c = sh.Case("append", G, 1001, 0, 4, (10,), appends=(37,), seed=5)
    dd = sh.data(c)
    n0, n1 = c.stages()
    values = dd["values"]
    rows = sh.attr_rows(sh.Case("program", G, n1, 0, 4, (10,), program="plain", seed=7), n1)
    col = np.ascontiguousarray(values, np.int32)
    setters = {
        "set_deleted": lambda t, n: t.set_deleted(sh.deleted_bits(sh.Case("d", G, n, 0, 1, (1,), deleted="random", seed=5), n)),
        "set_int_filter": lambda t, n: t.set_column(col[:n].copy(), 0, 4, 4, ">=", 0, values[:n]),
        "set_filter_program": lambda t, n: t.set_program(rows[:n]),
    }
    masks = {
        "set_deleted": lambda n: ~sh.unpack(sh.deleted_bits(sh.Case("d", G, n, 0, 1, (1,), deleted="random", seed=5), n), n),
        "set_int_filter": lambda n: values[:n] >= 0,
        "set_filter_program": lambda n: sh.program_mask(rows[:n]),
    }
    for call, setter in setters.items():
        trio = Trio(pool, G, 0)
        trio.attach(dd["X"][:n0])
        setter(trio, n0)
        trio.append(dd["X"][n0:n1])
        codes = [_code(lambda: ix.search(dd["Q"], 10, mode=pool.amd.MODE_FLAT)) for ix in (trio.grp, trio.one)]
        for code, msg in codes:
            assert code == USER and ("call %s again" % call) in msg, (call, code, msg)
        setter(trio, n1)
        g, o, m = trio.search(dd["Q"], 10)
        sh.same(g, o, call + " [group vs one plain index]")
        sh.same(g, m, call + " [group vs G plain indices merged]")
        er.check_exact(g[0], g[1], g[2], dd["X"], None, 0, 10, visible=masks[call](n1), ref=dd["ref"], what=call)


@pytest.mark.parametrize("G", [3, 5, 16])
def test_a_stale_bitset_is_refused_wherever_the_appended_rows_land(pool, G):
    """n0 = 32 G rows (every shard's slice ends with its byte, as the whole bitset does), only rows of shard 1 deleted: the other shards keep no
    bitset at all.  One appended row lands on shard 0: the plain index refuses the next search (its bitset is a byte short), and so must the
    group, whose shard 1 did not grow and whose shard 0 has nothing to compare with.  A bitset with no bit set is no bitset on either side.  One
    handed over for a longer table than attached stays good on the plain index until the table outgrows it; the group's slices are cut for the
    rows it had, so it refuses from the first appended row on - earlier than the plain index, never later, and never with another answer."""
    amd = pool.amd
    n0 = 32 * G
    c = sh.Case("stale", G, n0, 0, 4, (10,), appends=(1,), seed=16)
    dd = sh.data(c)
    trio = Trio(pool, G, 0)
    dead = np.zeros(n0 + 8, bool)
    dead[1:n0:G] = True
    bits = np.packbits(dead[:n0], bitorder="little")
    assert len(bits) == n0 // 8 and all(not sh.split_bits(bits, n0, s, G).any() for s in range(G) if s != 1)
    for what, first in (("one shard's rows", bits), ("no bit set", np.zeros(n0 // 8, np.uint8))):
        trio.attach(dd["X"][:n0])
        trio.set_deleted(first)
        trio.append(dd["X"][n0:])
        codes = [_code(lambda: ix.search(dd["Q"], 10, mode=amd.MODE_FLAT)) for ix in (trio.grp, trio.one)]
        want = (USER, USER) if first.any() else (0, 0)
        assert (codes[0][0], codes[1][0]) == want, "%s: the group returns %d, the plain index %d" % (what, codes[0][0], codes[1][0])
        if first.any():
            assert all("call set_deleted again" in msg for _, msg in codes), codes
        vis = ~dead[:n0 + 1] if first.any() else np.ones(n0 + 1, bool)
        trio.set_deleted(np.packbits(~vis, bitorder="little") if first.any() else None)
        g, o, m = trio.search(dd["Q"], 10)
        sh.same(g, o, what + " [group vs one plain index]")
        sh.same(g, m, what + " [group vs G plain indices merged]")
        er.check_exact(g[0], g[1], g[2], dd["X"], None, 0, 10, visible=vis, ref=dd["ref"], what=what)
    # a bitset for more rows than attached (8 to spare, shard 1's among them deleted): the plain index reads the caller's bits for the appended
    # rows, the group has none for them and refuses; after the call is repeated both give the whole table's answer
    trio.attach(dd["X"][:n0 - 8])
    trio.set_deleted(bits)
    trio.append(dd["X"][n0 - 8:n0])
    box = []
    assert _code(lambda: box.append(trio.one.search(dd["Q"], 10, mode=amd.MODE_FLAT)))[0] == 0
    er.check_exact(box[0][0], box[0][1], box[0][2], dd["X"][:n0], None, 0, 10, visible=~dead[:n0], ref=_ref_rows(dd["ref"], n0), what="plain, spare bits")
    code, msg = _code(lambda: trio.grp.search(dd["Q"], 10, mode=amd.MODE_FLAT))
    assert code == USER and "call set_deleted again" in msg, (code, msg)
    trio.grp.set_deleted(bits)
    sh.same(trio.grp.search(dd["Q"], 10, mode=amd.MODE_FLAT), box[0], "spare bits, after set_deleted again")
    trio.append(dd["X"][n0:])
    g, o = (_code(lambda: ix.search(dd["Q"], 10, mode=amd.MODE_FLAT))[0] for ix in (trio.grp, trio.one))
    assert o == USER and g == USER, (g, o)
    # a new, longer table drops a bitset that is too short for it - on every shard, as the plain index does
    trio.attach(dd["X"][:n0 - 8])
    trio.set_deleted(bits[:-1])
    for ix in (trio.grp, trio.one):
        ix.attach_rows(dd["X"])
    g, o = (ix.search(dd["Q"], 10, mode=amd.MODE_FLAT) for ix in (trio.grp, trio.one))
    sh.same(g, o, "a longer table attached over a short bitset")
    er.check_exact(g[0], g[1], g[2], dd["X"], None, 0, 10, ref=dd["ref"], what="a longer table attached over a short bitset")


# ------------------------------------------------------------------------------------------------ g. device buffers
def test_device_buffers_back_to_back(pool):
    """queries and results as torch tensors on device 0, counts included; three calls back to back with no synchronize between them, (nq, k) =
    (4, 10), (64, 100), (4, 10) - the middle one makes the gathered buffer regrow while a merge is pending -, one synchronize, all three compared;
    then results in host memory right after a device-results call"""
    import torch
    G = 3
    c = sh.Case("device", G, 1003, 0, 64, (10, 100), repeat=True, seed=11)
    dd = sh.data(c)
    trio = Trio(pool, G, 0, tag="fresh")           # (a group whose gathered buffer has not grown yet)
    trio.attach(dd["X"])
    Qd = torch.from_numpy(dd["Q"]).cuda()
    shapes = ((4, 10), (64, 100), (4, 10))
    outs = [(torch.full((nq, k), -7, dtype=torch.int64, device="cuda"), torch.full((nq, k), -7, dtype=torch.float32, device="cuda"),
             torch.full((nq,), -7, dtype=torch.int32, device="cuda")) for nq, k in shapes]
    torch.cuda.synchronize()       # (the shards run on their own streams: the fills above must have landed)
    for (nq, k), o in zip(shapes, outs):
        trio.grp.search(Qd[:nq], k, out=o, mode=pool.amd.MODE_FLAT)
    trio.grp.synchronize()
    host = trio.grp.search(dd["Q"][:5], 10, mode=pool.amd.MODE_FLAT)      # host results right after device-results calls
    for (nq, k), o in zip(shapes, outs):
        got = tuple(t.cpu().numpy() for t in o)
        want = trio.one.search(dd["Q"][:nq], k, mode=pool.amd.MODE_FLAT)
        sh.same(got, want, "device buffers nq %d k %d" % (nq, k))
        er.check_exact(got[0], got[1], got[2], dd["X"], None, 0, k, ref=dd["ref"].take(np.arange(nq)), what="device buffers nq %d k %d" % (nq, k))
    sh.same(host, trio.one.search(dd["Q"][:5], 10, mode=pool.amd.MODE_FLAT), "host results after device results")
    # once more with a call pending when the host-results call comes
    trio.grp.search(Qd[:4], 10, out=outs[0], mode=pool.amd.MODE_FLAT)
    host = trio.grp.search(dd["Q"][:64], 100, mode=pool.amd.MODE_FLAT)
    trio.grp.synchronize()
    sh.same(host, trio.one.search(dd["Q"][:64], 100, mode=pool.amd.MODE_FLAT), "host results behind a pending merge")
    sh.same(tuple(t.cpu().numpy() for t in outs[0]), trio.one.search(dd["Q"][:4], 10, mode=pool.amd.MODE_FLAT), "the pending call")
    # fewer visible rows than k: the counts of the device merge (the kernel's) and of the host path (read off the ids) are the same numbers
    dead = np.ones(c.n, bool)
    dead[[5, 6, 7 + G]] = False
    trio.set_deleted(np.packbits(dead, bitorder="little"))
    trio.grp.search(Qd[:4], 10, out=outs[0], mode=pool.amd.MODE_FLAT)
    trio.grp.synchronize()
    dev = tuple(t.cpu().numpy() for t in outs[0])
    sh.same(dev, trio.grp.search(dd["Q"][:4], 10, mode=pool.amd.MODE_FLAT), "three visible rows [device results vs host results]")
    sh.same(dev, trio.one.search(dd["Q"][:4], 10, mode=pool.amd.MODE_FLAT), "three visible rows [group vs one plain index]")
    assert (dev[2] == 3).all() and (dev[0][:, 3:] == -1).all() and np.isposinf(dev[1][:, 3:]).all()


# ------------------------------------------------------------------------------------------------ h. large k
def test_large_k_as_a_plain_index(pool):
    """n = 3000, G = 3 (shards of 1000 rows), k in {1000, 1024, 1025, 2048, 3003}: k >= rows per shard, the result pages beyond 1024, k beyond the
    table - whatever a plain index returns for that k, refusal codes included"""
    G = 3
    c = sh.Case("largek", G, 3000, 0, 3, (1000, 1024, 1025, 2048, 3003), seed=12)
    dd = sh.data(c)
    trio = Trio(pool, G, 0)
    trio.attach(dd["X"])
    for k in c.ks:
        res = []
        for ix in (trio.grp, trio.one):
            box = []
            code = _code(lambda: box.append(ix.search(dd["Q"], k, mode=pool.amd.MODE_FLAT)))[0]
            res.append((code, box))
        assert res[0][0] == res[1][0], "k %d: the group returns %d, the plain index %d" % (k, res[0][0], res[1][0])
        if res[0][0] == 0:
            trio.held(c, k)


# ------------------------------------------------------------------------------------------------ i. NaN / inf rows
@pytest.mark.parametrize("G", [3, 5])
def test_nan_and_inf_rows_come_last_in_id_order(pool, G):
    """NaN and +-inf rows on different shards: numbers first, then +inf, then the NaN rows in id order, under every metric"""
    cases = _cases("nan", G=G)
    assert len(cases) == 3
    for c in cases:
        trio = Trio(pool, G, c.metric)
        trio.attach(sh.data(c)["X"])
        for k in c.ks:
            g = trio.held(c, k)
        nans = np.flatnonzero(np.isnan(sh.data(c)["ref"].d64[:, 0]))
        assert np.array_equal(g[0][0, c.n - len(nans):c.n], nans) and np.isnan(g[1][0, c.n - len(nans):c.n]).all()


# ------------------------------------------------------------------------------------------------ j. the matrix engines
def test_matrix_engines_on_the_shards(pool):
    """2 x 65 537 rows x 32, G = 2: every shard is large enough for the 8-bit matrix engine.  nq = 40 (the staged chain; it also builds the mirror)
    and nq = 3 (the one-pass form), k = 10.  The stats must show that the 8-bit engine ran on the shards."""
    amd = pool.amd
    G, d = 2, 32
    c = sh.Case("matrix", G, 2 * 65537, 0, 40, (10,), d=d, seed=13)
    dd = sh.data(c)
    trio = Trio(pool, G, 0, d=d)
    trio.attach(dd["X"])
    for nq in (40, 3, 3):
        Q = dd["Q"][:nq]
        g, o, m = trio.search(Q, 10, flat_engine=amd.FLAT_MFMA_I8)
        st = trio.grp.stats()
        print("shard-ties: matrix engines nq %2d: bits %d one_pass %d i8_declined %d rerank_rows %d launches %d" % (
            nq, st["main_kernel_bits"], st["one_pass"], st["i8_declined"], st["rerank_rows"], st["main_kernel_launches"]))
        assert st["main_kernel_bits"] == 8 and st["i8_declined"] == 0, st
        what = "matrix engines nq %d" % nq
        sh.same(g, o, what + " [group vs one plain index]")
        sh.same(g, m, what + " [group vs G plain indices merged]")
        er.check_exact(g[0], g[1], g[2], dd["X"], None, 0, 10, ref=dd["ref"].take(np.arange(nq)), what=what)
    assert st["one_pass"] == G, "nq = 3 did not run the one-pass form on every shard: %s" % st


# ------------------------------------------------------------------------------------------------ k. the graph
def test_graph_per_shard(pool, tmp_path):
    """G = 3, n = 2001, d = 16 on a tie table of test_gpu_build_ties.py's family.  Two builds of one plain shard give the identical graph on this table
    (asserted first), so the BUILDS are compared: grp.build() then MODE_GRAPH against three plain indices built and searched with the same
    parameters and merged - ids, distance bits, counts.  (A traversal is approximate: the whole table's exact answer and a plain index over the whole
    table, whose graph is another graph, do not apply here.)  Then the save / load round trip through the .shard<s> files, into the group and into
    the plain indices."""
    import build_ref as br
    amd = pool.amd
    G, n, d = 3, 2001, 16
    X = br.tie_table(n, d, 0, seed=41)
    Q = br.tie_table(24, d, 0, seed=42)
    trio = Trio(pool, G, 0, d=d)
    trio.attach(X)
    first = trio.parts[1]
    graphs = []
    for _ in range(2):
        first.build()
        graphs.append(first.get_graph())
    assert graphs[0][2] == graphs[1][2] and np.array_equal(graphs[0][0], graphs[1][0]) and np.array_equal(graphs[0][1], graphs[1][1]), \
        "two builds of one shard differ on this table"
    for ix in trio.parts:
        ix.build()
    trio.grp.build()
    assert trio.grp.graph_info()[:2] == (n, sum(ix.graph_info()[1] for ix in trio.parts))
    kw = dict(mode=amd.MODE_GRAPH, intra_threads=4)

    def parts_merged(parts, k):
        ids, dist = np.empty((G, len(Q), k), np.int64), np.empty((G, len(Q), k), F)
        for s, ix in enumerate(parts):
            ids[s], dist[s], _ = ix.search(Q, k, **kw)
        md, mi = amd.merge_topk(dist, ids, np.empty((len(Q), k), F), np.empty((len(Q), k), np.int64))
        return mi, md, (mi >= 0).sum(axis=1).astype(np.int32)

    for k in (1, 10, 50):
        g = trio.grp.search(Q, k, **kw)
        sh.same(g, parts_merged(trio.parts, k), "graph k %d [group vs G plain indices merged]" % k)
        assert (g[2] == k).all() and all(len(set(r)) == k for r in g[0])
    want = trio.grp.search(Q, 10, **kw)
    p = str(tmp_path / "ann_graph_1.bin")
    trio.grp.save_graph(p)
    assert all(os.path.exists("%s.shard%d" % (p, s)) for s in range(G))
    again = pool.group(G, 0, d, tag="loaded")
    again.attach_rows(X)
    again.load_graph(p)
    sh.same(again.search(Q, 10, **kw), want, "graph after save / load")
    for s, ix in enumerate(trio.parts):        # the group's shard files are the plain indices' graphs
        mine = ix.get_graph()
        ix.load_graph("%s.shard%d" % (p, s))
        theirs = ix.get_graph()
        assert mine[2] == theirs[2] and np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1]), "shard %d's graph file" % s


# ------------------------------------------------------------------------------------------------ l. clone_rows
def test_clone_rows(pool):
    """group to group with n not a multiple of G and n < rows; appending to the source afterwards does not change the clone's answers.  Refused: a
    plain index as source, a different G, a different dim, n > rows.  And the one-line case on a plain index."""
    amd = pool.amd
    G = 3
    c = sh.Case("clone", G, 1003, 0, 5, (10,), appends=(40,), repeat=True, seed=14)
    dd = sh.data(c)
    n_clone = 1000
    assert n_clone % G and n_clone < c.n
    trio = Trio(pool, G, 0)
    trio.attach(dd["X"][:c.n])
    src = trio.grp
    dst = pool.group(G, 0, 8, tag="clone")
    dst.clone_rows(src, n_clone)
    assert dst.row_count == n_clone and src.row_count == c.n
    ref = _ref_rows(dd["ref"], n_clone)
    before = dst.search(dd["Q"], 10, mode=amd.MODE_FLAT)
    er.check_exact(before[0], before[1], before[2], dd["X"][:n_clone], None, 0, 10, ref=ref, what="clone")
    trio.one.attach_rows(dd["X"][:n_clone])
    sh.same(before, trio.one.search(dd["Q"], 10, mode=amd.MODE_FLAT), "clone [group vs one plain index]")
    src.append_rows(dd["X"][c.n:])
    after = dst.search(dd["Q"], 10, mode=amd.MODE_FLAT)
    sh.same(after, before, "clone after the source grew")
    assert dst.row_count == n_clone and src.row_count == c.total
    g = src.search(dd["Q"], 10, mode=amd.MODE_FLAT)
    er.check_exact(g[0], g[1], g[2], dd["X"], None, 0, 10, ref=dd["ref"], what="the source after its append")
    # the clone can grow on its own
    dst.append_rows(dd["X"][n_clone:c.n])
    g = dst.search(dd["Q"], 10, mode=amd.MODE_FLAT)
    er.check_exact(g[0], g[1], g[2], dd["X"][:c.n], None, 0, 10, ref=_ref_rows(dd["ref"], c.n), what="the clone after its own append")
    # refusals leave the destination as it was
    other_g, other_d, plain = pool.group(2, 0, 8), pool.group(G, 0, 16, tag="dim16"), trio.one
    for bad, n in ((plain, 10), (other_g, 10), (other_d, 10), (src, c.total + 1), (dst, 10)):
        code, msg = _code(lambda: dst.clone_rows(bad, n))
        assert code == USER and "clone_rows" in msg, (code, msg)
    code, msg = _code(lambda: plain.clone_rows(src, 10))
    assert code == USER and "clone_rows" in msg, (code, msg)
    sh.same(dst.search(dd["Q"], 10, mode=amd.MODE_FLAT), g, "after the refused clones")
    # a plain index from a plain index
    twin = pool.plain(0, 8, "twin")
    plain.attach_rows(dd["X"][:c.n])
    twin.clone_rows(plain, n_clone)
    sh.same(twin.search(dd["Q"], 10, mode=amd.MODE_FLAT), before, "plain clone")


# ------------------------------------------------------------------------------------------------ m. refusals and state
def test_refusals_leave_the_state_alone(pool):
    """what a group does not serve returns EPS_DB_UNSUPPORTED_ERROR and leaves the next search's answer unchanged; a group whose shards do not hold a
    hash split refuses search and build; dist_evals is the sum over the G plain indices"""
    import torch
    amd = pool.amd
    G = 3
    c = sh.Case("refusals", G, 1003, 0, 4, (10,), repeat=True, seed=15)
    dd = sh.data(c)
    trio = Trio(pool, G, 0)
    trio.attach(dd["X"])
    grp, Q = trio.grp, dd["Q"]
    want = trio.held(c, 10)
    assert grp.stats()["dist_evals"] == sum(ix.stats()["dist_evals"] for ix in trio.parts) == c.nq * c.n
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    devf = torch.zeros((G, 8), dtype=torch.float32, device="cuda")
    devr = torch.zeros((c.n + 5, 24), dtype=torch.uint8, device="cuda")
    refused = {
        "set_stream": lambda: grp.set_stream(None),
        "set_id_map": lambda: grp.set_id_map(0, 1),
        "set_graph": lambda: grp.set_graph(np.zeros(2, np.int64), np.zeros(1, np.int64), 0),
        "get_graph": lambda: grp.get_graph(),
        "search_walk": lambda: grp.search_walk(Q, 5, 20, mode=amd.MODE_FLAT),
        "select": lambda: grp.select(0, 10),
        "search_range": lambda: grp.search_range(Q, 1.0, 8),
        "search_among": lambda: grp.search_among(Q, np.arange(10, dtype=np.int64), 5),
        "device rows": lambda: grp.attach_rows(devf),
        "device rows appended": lambda: grp.append_rows(devf),
        "device bitset": lambda: grp.set_deleted(dev),
        "device column": lambda: grp.set_int_filter(dev, ">=", 0, stride=4, width=4),
        "device attribute rows": lambda: grp.set_filter_program(sh.PROGRAM, devr, stride=24),
    }
    for name, call in refused.items():
        code, msg = _code(call)
        assert code == UNSUPPORTED and msg, (name, code, msg)
        sh.same(grp.search(Q, 10, mode=amd.MODE_FLAT), want, "after the refused " + name)
        assert grp.row_count == c.n
    # shards that do not hold a hash split: some shards only, or counts that are no split
    loose = pool.group(G, 0, 8, tag="loose")
    loose.attach_shard_rows(0, np.ascontiguousarray(dd["X"][0::G]))
    for call in (lambda: loose.search(Q, 10, mode=amd.MODE_FLAT), lambda: loose.build()):
        code, msg = _code(call)
        assert code == USER and "hash split" in msg, (code, msg)
    loose.attach_shard_rows(1, np.ascontiguousarray(dd["X"][1::G]))
    loose.attach_shard_rows(2, np.ascontiguousarray(dd["X"][2::G][:-1]))      # one row short
    for call in (lambda: loose.search(Q, 10, mode=amd.MODE_FLAT), lambda: loose.build()):
        code, msg = _code(call)
        assert code == USER and "hash split" in msg, (code, msg)
    loose.attach_shard_rows(2, np.ascontiguousarray(dd["X"][2::G]))
    sh.same(loose.search(Q, 10, mode=amd.MODE_FLAT), want, "rows attached shard by shard")
