"""CPU checks of what the hash-sharded index (eps_index_create_sharded; csrc/shard_group.cpp) is held to on the device:

(a) tests/shard_ref.py's model - the hash split of rows, bits, a strided column and attribute rows; per-shard exact top-k; the k-way merge with
    -1 / +inf padding and counts - gives, on EVERY case of shard_ref.CASES and at every stage of its appends, the whole table's answer as
    tests/exact_ref.py states it (check_exact; the NaN / inf cases, whose table check_exact refuses by design, against the flat contract of DESIGN
    3.3 stated without any split);
(b) every planted fault of shard_ref.FAULTS changes the answer of at least one case: the case list can tell a wrong group from a right one;
(c) the cases are what they claim to be, asserted from the case data alone: a tie between rows of different shards at the k-th place, bit slices
    that are all zero on the shards that must take the no-deletions path, shards shorter than k and empty shards, a filter that empties one shard;
(d) the group's host arithmetic (csrc/shard_host.hpp - the header csrc/shard_group.cpp compiles) as a stand-alone program under AddressSanitizer
    and UBSan, every caller buffer at exactly the size the ABI demands (tests/native/shard_host_check.cpp).
No GPU is touched.  Every comparison is equality of integers and of float bit patterns."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_ref as er
import merge_ref as mr
import shard_ref as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KINDS = sorted({c.kind for c in sh.CASES})


def _stages(case):
    return range(len(case.stages()))


# ---- (a)
@pytest.mark.parametrize("kind", KINDS)
def test_model_equals_the_whole_table_on_every_case(kind):
    cases = [c for c in sh.CASES if c.kind == kind]
    assert cases
    for c in cases:
        dd = sh.data(c)
        for stage in _stages(c):
            n = int(c.stages()[stage])
            vis = sh.visible(c, n)
            for k in c.ks:
                got = sh.model(c, k, stage)
                what = "%s stage %d k %d" % (c.name, stage, k)
                sh.same(got, sh.whole_table(c, k, stage), what)
                if not c.nan:
                    er.check_exact(got[0], got[1], got[2], dd["X"][:n], None, c.metric, k, visible=vis, ref=_ref_rows(dd["ref"], n), what=what)


def _ref_rows(ref, n):
    """exact_ref.Ref of the table's first n rows (an append case's earlier stages)"""
    if n == ref.n:
        return ref
    r = object.__new__(er.Ref)
    r.n, r.d, r.metric, r.nq = n, ref.d, ref.metric, ref.nq
    r.d64 = ref.d64[:n]
    r.mag = r.d64 if ref.metric == 0 else ref.mag[:n]
    return r


def test_nan_rows_come_last_in_id_order():
    """the flat contract the NaN cases are held to, spelled out on the model's answer: numbers ascending, then +inf, then the NaN rows by id"""
    for c in (c for c in sh.CASES if c.nan):
        d32 = sh.data(c)["ref"].d64.astype(F)
        k = max(c.ks)
        ids, dist, cnt = sh.model(c, k)[:3]
        assert (cnt == c.n).all()
        for q in range(c.nq):
            nans = np.flatnonzero(np.isnan(d32[:, q]))
            assert len(nans) >= 3 and len({int(r) % c.G for r in nans}) >= 2, "%s: the NaN rows do not sit on different shards" % c.name
            assert np.array_equal(ids[q, c.n - len(nans):c.n], nans) and np.isnan(dist[q, c.n - len(nans):c.n]).all(), c.name
            head = dist[q, :c.n - len(nans)]
            assert not np.isnan(head).any() and np.isposinf(head).any() and (np.diff(mr.ordinal(head).astype(np.int64)) >= 0).all(), c.name


# ---- (b)
WHERE = {"append_first": ("append", "program"), "bit_order": ("deleted",), "local_ids": ("ties", "edges"), "tie_by_shard": ("ties",), "nan_raw": ("nan",),
         "pad_is_row": ("edges",), "counts_shard0": ("edges",), "no_pad_short": ("edges",)}


@pytest.mark.parametrize("fault", sh.FAULTS)
def test_every_planted_fault_changes_some_answer(fault):
    caught = []
    for c in sh.CASES:
        if c.kind not in WHERE[fault] or (c.kind == "edges" and (c.nq > 1 or c.n > 8 * c.G + 1)):     # (the small ones are enough, and quick)
            continue
        for stage in _stages(c):
            for k in c.ks:
                if sh.differs(sh.model(c, k, stage, fault=fault), sh.whole_table(c, k, stage)):
                    caught.append((c.name, stage, k))
    assert caught, "no case of %s notices the fault %r: the cases are too weak" % (WHERE[fault], fault)
    print("shard-ref: fault %-14s changes %d answers, first %s" % (fault, len(caught), caught[0]))


def test_a_fault_free_model_is_not_reported():
    c = next(c for c in sh.CASES if c.kind == "ties")
    assert not sh.differs(sh.model(c, c.ks[0]), sh.whole_table(c, c.ks[0]))


# ---- (c)
def test_tie_cases_cut_a_tie_between_shards():
    cases = [c for c in sh.CASES if c.kind == "ties"]
    assert {c.G for c in cases} == {2, 3, 5}
    for c in cases:
        d64 = sh.data(c)["ref"].d64
        for k in c.ks:
            hit = 0
            for q in range(c.nq):
                order = np.lexsort((np.arange(c.n), d64[:, q]))
                a, b = order[k - 1], order[k]
                hit += d64[a, q] == d64[b, q] and a % c.G != b % c.G
            assert hit, "%s k %d: no query whose k-th and (k+1)-th rows tie across shards" % (c.name, k)


def test_one_shard_deleted_cases_leave_the_other_slices_all_zero():
    cases = [c for c in sh.CASES if c.kind == "deleted" and c.deleted.startswith("class")]
    assert len(cases) == 4
    for c in cases:
        r = int(c.deleted[5:])
        bits = sh.deleted_bits(c, c.n)
        assert len(bits) == (c.n + 7) // 8
        for s in range(c.G):
            local = sh.split_bits(bits, c.n, s, c.G)
            if s == r:
                assert sh.unpack(local, sh.rows_of(s, c.n, c.G)).all() and sh.rows_of(s, c.n, c.G) > 0
            else:
                assert not local.any(), "%s: shard %d's slice is not all zero" % (c.name, s)
    for c in (c for c in sh.CASES if c.kind == "deleted"):
        bits, n, G = sh.deleted_bits(c, c.n), c.n, c.G
        live = np.flatnonzero(~sh.unpack(bits, n))
        if c.deleted == "but3same":
            assert len(live) == 3 and len({int(i) % G for i in live}) == 1
        elif c.deleted == "but3diff":
            assert len(live) == 3 and len({int(i) % G for i in live}) == 3
        elif c.deleted == "last":
            assert np.array_equal(np.flatnonzero(sh.unpack(bits, n)), [n - 1])
        elif c.deleted == "beyond":
            assert n % 8 and (bits[-1] >> (n % 8)) == (0xFF >> (n % 8)) and len(live) == n - 2


def test_short_shard_cases_hold_short_and_empty_shards():
    assert sh.SHORT and sh.EMPTY
    for c in sh.SHORT:
        assert any(sh.rows_of(s, c.n, c.G) < max(c.ks) for s in range(c.G)), c.name
    for c in sh.EMPTY:
        assert any(sh.rows_of(s, c.n, c.G) == 0 for s in range(c.G)), c.name
    assert {c.G for c in sh.EMPTY} == {G for G in sh.EDGE_GS if G > 1}
    for G in sh.EDGE_GS:      # n in {1, G-1, G, G+1, 8G-1, 8G+1, 1003} and a row count with n mod 8 != 0
        assert {c.n for c in sh.CASES if c.kind == "edges" and c.G == G} == {n for n in (1, G - 1, G, G + 1, 8 * G - 1, 8 * G + 1, 1003) if n > 0}
    for c in (c for c in sh.CASES if c.kind == "edges"):
        assert set(c.ks) == {k for k in (1, 10, c.n, c.n + 3)} and c.nq in (1, 129)


def test_column_cases_cover_widths_operators_and_the_empty_filters():
    cases = [c for c in sh.CASES if c.kind == "column"]
    for G in (3, 5):
        mine = [c for c in cases if c.G == G]
        assert {(c.column[0], c.column[1]) for c in mine} >= {(w, op) for w in sh.COLUMNS for op in sh.OPS}
        assert (sh.data(mine[0])["values"] < 0).any()
        one = [c for c in mine if c.column == ("rec12", ">", 0)][0]
        vis = sh.shard_visible(one, one.n)
        assert not vis[1].any() and all(vis[s].any() for s in range(G) if s != 1), "%s: the filter does not empty exactly shard 1" % one.name
        none = [c for c in mine if c.column == ("i16", ">", 100)][0]
        assert not sh.visible(none, none.n).any()
    buf, offset, stride, width, _, _ = sh.column_buffer(next(c for c in cases if c.column[0] == "rec12"), 1003)
    assert (offset, stride, width) == (4, 12, 4) and len(buf) == offset + 1002 * stride + width      # the buffer ends with the last value


def test_append_cases_start_off_a_multiple_of_G():
    cases = [c for c in sh.CASES if c.kind == "append"]
    assert {c.G for c in cases} >= {2, 3, 5}
    for c in cases:
        assert c.n % c.G != 0 and c.appends == (1, 1, c.G - 1, c.G + 1, 0, 37) or c.n < c.G
        src = sh.split_rows(c.n, c.appends, c.G)
        for s in range(c.G):      # the appends tile every shard: local row l is global row l * G + s
            assert np.array_equal(src[s], np.arange(s, c.total, c.G)), (c.name, s)


# ---- (d)
def test_shard_host_arithmetic_is_clean_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "shard_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "shard_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "shard_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_the_library_compiles_the_header_the_native_check_runs():
    """shard_group.cpp keeps no split arithmetic of its own: it includes shard_host.hpp, and the expressions the header now owns are gone from it"""
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "shard_group.cpp")).read()
    chk = open(os.path.join(ROOT, "tests", "native", "shard_host_check.cpp")).read()
    assert '#include "shard_host.hpp"' in src and "vectordb_amd/csrc/shard_host.hpp" in chk
    for name in ("shard_rows_of", "shard_append_span", "shard_split_bits", "shard_column_view", "shard_attr_view", "shard_gather_stride", "shard_counts_from_ids"):
        assert name + "(" in src and name + "(" in chk, name
    for gone in ("% G()", "* 12 + 7", "* G() + s", "(int64_t)s * stride", "(int64_t)s * dim_", "i >> 3"):
        assert gone not in src, "shard_group.cpp still computes %r itself" % gone
