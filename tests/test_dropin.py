"""The drop-in boundary, end to end: the REFERENCE's own DBServer / DBMVP / TableMVP / TableSegmentMVP / filter
engine / WAL (compiled unmodified from /root/reference by dropin/Makefile) running on THIS repository's
ANNGraphSegment + VecSearchExecutor + GetDistFunc (include/db/**, dropin/*.cpp -> libepsilla_gfx950.so).
GPU tests replay the reference's own known-answer gtest cases (engine/test/engine/db/db_server.cpp) through it."""
import os

import numpy as np
import pytest

from helpers import data
from oracle.pyoracle import DROPIN_SO, Ref, dropin_available, ref_available

CITY_SCHEMA = {
    "name": "MyTable",
    "fields": [
        {"name": "ID", "dataType": "INT", "primaryKey": True},
        {"name": "Doc", "dataType": "STRING"},
        {"name": "EmbeddingEuclidean", "dataType": "VECTOR_FLOAT", "dimensions": 4, "metricType": "EUCLIDEAN"},
        {"name": "EmbeddingDotProduct", "dataType": "VECTOR_FLOAT", "dimensions": 4, "metricType": "DOT_PRODUCT"},
        {"name": "EmbeddingCosine", "dataType": "VECTOR_FLOAT", "dimensions": 4, "metricType": "COSINE"},
    ],
}
CITIES = [(1, "Berlin", [0.05, 0.61, 0.76, 0.74]), (2, "London", [0.19, 0.81, 0.75, 0.11]),
          (3, "Moscow", [0.36, 0.55, 0.47, 0.94]), (4, "San Francisco", [0.18, 0.01, 0.85, 0.80]),
          (5, "Shanghai", [0.24, 0.18, 0.22, 0.44])]
Q4 = np.array([0.35, 0.55, 0.47, 0.94], np.float32)


def city_records():
    return [{"ID": i, "Doc": c, "EmbeddingEuclidean": v, "EmbeddingDotProduct": v, "EmbeddingCosine": v} for i, c, v in CITIES]


@pytest.fixture(scope="module")
def dropin():
    if os.path.isdir("/root/reference/engine"):
        from vectordb_amd.build import build
        from oracle.pyoracle import build_dropin
        build()
        build_dropin()
    if not dropin_available():
        pytest.skip("oracle/_ref/dropin/libepsilla_dropin.so not built (needs the reference's sources: `make -C dropin OUT=$PWD/oracle/_ref/dropin`)")
    return Ref(DROPIN_SO)


def test_reference_dbms_compiles_and_links_against_dropin_headers(dropin):
    """CPU: the unmodified reference DBMS layers build against include/db/** and link to libepsilla_gfx950.so;
    ingest works; a search without a GPU fails loudly (no CPU fallback) instead of answering."""
    import tempfile
    import torch
    db = dropin.db(os.path.join(tempfile.mkdtemp(), "db"))
    assert db.create_table(CITY_SCHEMA) == 0
    assert db.insert("MyTable", city_records()) == 0
    rc, res = db.search("MyTable", "EmbeddingEuclidean", Q4, 6, fields=("ID", "Doc"))
    if not torch.cuda.is_available():
        assert rc == 40001 and "gfx950" in res, (rc, res)   # INFRA_UNEXPECTED_ERROR
    db.close()


@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_search_by_attribute_matches_reference(dropin, tmp_path):
    """CPU: DBServer::Project -> VecSearchExecutor::SearchByAttribute (vec_search_executor.cpp:937-1033) has no vector
    arithmetic; the drop-in's host implementation must return what the reference returns: primary-key lists, filters,
    skip/limit windows, deleted rows."""
    ref = Ref()
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "Tag", "dataType": "STRING"},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 4, "metricType": "EUCLIDEAN"}]}
    X = data(300, 4, 3)
    recs = [{"ID": int(i), "Tag": "t%d" % (i % 5), "V": [float(x) for x in X[i]]} for i in range(300)]
    dbs = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        db = lib.db(str(tmp_path / name))
        assert db.create_table(schema) == 0 and db.insert("T", recs) == 0
        assert db.delete("T", [7, 8, 9, 200]) == 0
        dbs.append(db)
    cases = [dict(), dict(flt="ID < 50"), dict(flt="Tag = 't3' AND ID >= 100"), dict(skip=10, limit=25),
             dict(flt="ID > 5", skip=3, limit=7), dict(pks=[5, 7, 250, 9999, 12]), dict(pks=[250, 5], flt="ID < 100"),
             dict(limit=0), dict(skip=1000, limit=10)]
    for kw in cases:
        a = dbs[0].get("T", fields=("ID", "Tag"), **kw)
        b = dbs[1].get("T", fields=("ID", "Tag"), **kw)
        assert a == b, (kw, a, b)
    for db in dbs:
        db.close()


@pytest.mark.gpu
def test_gtest_DenseVector_through_dropin(dropin, tmp_path):
    """DbServer.DenseVector (db_server.cpp:92-319): three metrics, expected orderings :289-292, before and after
    Rebuild(); duplicate PK ignored."""
    db = dropin.db(str(tmp_path / "db"))
    assert db.create_table(CITY_SCHEMA) == 0
    recs = city_records()
    assert db.insert("MyTable", recs + [recs[0]]) == 0          # re-inserting PK 1 must be ignored (:308)
    want = {"EmbeddingEuclidean": ["Moscow", "Berlin", "Shanghai", "San Francisco", "London"],
            "EmbeddingDotProduct": ["Moscow", "Berlin", "San Francisco", "London", "Shanghai"],
            "EmbeddingCosine": ["Moscow", "Shanghai", "Berlin", "San Francisco", "London"]}
    for rebuild in (False, True):
        if rebuild:
            assert db.rebuild() == 0
        for field, order in want.items():
            rc, res = db.search("MyTable", field, Q4, 6, fields=("ID", "Doc", field))
            assert rc == 0, res
            assert [r["Doc"] for r in res] == order
    rc, res = db.search("MyTable", "EmbeddingEuclidean", Q4, 1)
    assert abs(res[0]["@distance"] - 1.0000040e-4) < 1e-8            # SURVEY §8c anchors
    rc, res = db.search("MyTable", "EmbeddingDotProduct", Q4, 1)
    assert abs(res[0]["@distance"] + 1.5329999924) < 1e-6
    db.close()


@pytest.mark.gpu
def test_gtest_DeleteByPK_and_Filter_through_dropin(dropin, tmp_path):
    """DbServer.DeleteByPK (:514-751) and DbServer.DenseVectorFilter (:1407-1630)."""
    db = dropin.db(str(tmp_path / "db"))
    assert db.create_table(CITY_SCHEMA) == 0 and db.insert("MyTable", city_records()) == 0
    rc, res = db.search("MyTable", "EmbeddingEuclidean", Q4, 6, fields=("ID", "Doc"), flt="ID <= 2")
    assert rc == 0 and sorted(r["ID"] for r in res) == [1, 2]
    rc, res = db.search("MyTable", "EmbeddingEuclidean", Q4, 6, fields=("ID", "Doc"), flt="Doc = 'Moscow' OR ID = 5")
    assert rc == 0 and [r["Doc"] for r in res] == ["Moscow", "Shanghai"]      # host-evaluated filter mask
    assert db.delete("MyTable", [1, 2, 3, 4]) == 0
    rc, res = db.search("MyTable", "EmbeddingEuclidean", Q4, 6, fields=("ID", "Doc"))
    assert [r["Doc"] for r in res] == ["Shanghai"] and abs(res[0]["@distance"] - 0.46149999) < 1e-6
    db.close()


@pytest.mark.gpu
def test_gtest_QueryDenseVectorDuringRebuild_through_dropin(dropin, tmp_path):
    """DbServer.QueryDenseVectorDuringRebuild (:1085-1245) at its original size: 10 000 unit vectors
    (cos(pi i/N), sin(pi i/N)), COSINE, query (1,0), limit 500.  Rebuild on a shuffled half -> the 500 smallest
    inserted ids in order (:1172-1180); insert the rest (graph 5000 + brute-force tail 5000) -> exactly 0..499
    (:1195-1199); and again after a second rebuild (:1223-1244)."""
    dropin.L.ref_config(4, 500, 1, 0, 4)
    db = dropin.db(str(tmp_path / "db"), scale=150000)
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 2, "metricType": "COSINE"}]}
    assert db.create_table(schema) == 0
    N = 10000
    recs = [{"ID": i, "V": [float(np.cos(np.pi * i / N)), float(np.sin(np.pi * i / N))]} for i in range(N)]
    order = np.random.default_rng(0).permutation(N)
    first, second = sorted(order[:N // 2].tolist()), sorted(order[N // 2:].tolist())
    q = np.array([1.0, 0.0], np.float32)
    assert db.insert("T", [recs[i] for i in order[:N // 2]]) == 0
    assert db.rebuild() == 0
    rc, res = db.search("T", "V", q, 500)
    assert rc == 0 and [r["ID"] for r in res] == first[:500]
    assert db.insert("T", [recs[i] for i in order[N // 2:]]) == 0
    rc, res = db.search("T", "V", q, 500)
    assert rc == 0 and [r["ID"] for r in res] == list(range(500))
    assert db.rebuild() == 0
    rc, res = db.search("T", "V", q, 500)
    assert rc == 0 and [r["ID"] for r in res] == list(range(500))
    db.close()
    dropin.L.ref_config(4, 500, 1, 0, 16)


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_dropin_matches_reference_dbserver_on_random_data(dropin, tmp_path):
    """Same JSON in, same JSON out: the reference DBServer on its own CPU executor vs. on the gfx950 executor
    (flat, graph + tail, int filter, string filter, deletes). Graphs differ (both builds are valid NSGs), results are
    compared where both are exact (n small enough that the reference search has recall 1)."""
    ref = Ref()
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "Tag", "dataType": "STRING"},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 16, "metricType": "EUCLIDEAN"}]}
    X = data(1800, 16, 21)
    recs = [{"ID": int(i), "Tag": "t%d" % (i % 7), "V": [float(x) for x in X[i]]} for i in range(1800)]
    dbs = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        lib.L.ref_config(1, 500, 1, 0, 2)
        db = lib.db(str(tmp_path / name))
        assert db.create_table(schema) == 0 and db.insert("T", recs[:1200]) == 0
        dbs.append(db)
    Q = data(6, 16, 22)

    def both(limit, flt=""):
        for q in Q:
            a = dbs[0].search("T", "V", q, limit, fields=("ID", "Tag"), flt=flt)
            b = dbs[1].search("T", "V", q, limit, fields=("ID", "Tag"), flt=flt)
            assert a[0] == 0 and b[0] == 0, (a, b)
            assert [r["ID"] for r in a[1]] == [r["ID"] for r in b[1]], flt
            assert np.allclose([r["@distance"] for r in a[1]], [r["@distance"] for r in b[1]], rtol=1e-4)

    both(10)                          # no graph yet: BruteForceSearch on both sides
    both(10, "ID < 300")
    for db in dbs:
        assert db.rebuild() == 0 and db.insert("T", recs[1200:]) == 0
    both(10)                          # graph over 1200 rows + brute-force tail of 600
    both(50, "ID >= 900")
    both(10, "Tag = 't3'")
    for db in dbs:
        assert db.delete("T", list(range(0, 1800, 5))) == 0
    both(10)
    for db in dbs:
        db.close()
    ref.L.ref_config(4, 500, 1, 0, 16)
    dropin.L.ref_config(4, 500, 1, 0, 16)


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_cpp_level_batch_entry_equals_single_searches_and_the_reference(dropin, tmp_path):
    """epsdrop::SearchBatch (include/epsdrop/search_batch.hpp, C++ in libepsilla_dropin.so - what a REST handler of a batched endpoint
    would call; db_server.cpp:458-510 answers one vector per call): N vectors -> ONE device batch -> a JSON array of N result arrays.
    Element q equals DBServer::Search of vector q through the same drop-in, and the REFERENCE DBServer's own answer: three metrics
    (COSINE: queries normalised per vector as table_mvp.cpp:333-343), a device-compiled filter, a host-only (string) filter, deletes,
    before and after a rebuild; errors carry the reference's Status codes."""
    ref = Ref()
    n, d = 1500, 12
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True}, {"name": "Tag", "dataType": "STRING"},
                                       {"name": "E", "dataType": "VECTOR_FLOAT", "dimensions": d, "metricType": "EUCLIDEAN"},
                                       {"name": "C", "dataType": "VECTOR_FLOAT", "dimensions": d, "metricType": "COSINE"},
                                       {"name": "P", "dataType": "VECTOR_FLOAT", "dimensions": d, "metricType": "DOT_PRODUCT"}]}
    X = data(n, d, 41)
    recs = [{"ID": int(i), "Tag": "t%d" % (i % 5), "E": [float(x) for x in X[i]], "C": [float(x) for x in X[i]], "P": [float(x) for x in X[i]]} for i in range(n)]
    Q = data(9, d, 42) * 2.0
    dbs = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        lib.L.ref_config(1, 500, 1, 0, 2)
        db = lib.db(str(tmp_path / name))
        assert db.create_table(schema) == 0 and db.insert("T", recs) == 0 and db.delete("T", [3, 4, 700]) == 0
        dbs.append(db)
    rdb, ddb = dbs

    def check(tag):
        for field in ("E", "C", "P"):
            for flt, limit in (("", 10), ("ID >= 300 AND ID < 1200", 7), ("Tag = 't2'", 5)):
                rc, batch = ddb.search_batch("T", field, Q, limit, fields=("ID", "Tag"), flt=flt)
                assert rc == 0 and len(batch) == len(Q), (tag, field, flt, batch)
                for qi, q in enumerate(Q):
                    rc1, one = ddb.search("T", field, q, limit, fields=("ID", "Tag"), flt=flt)
                    rc2, want = rdb.search("T", field, q, limit, fields=("ID", "Tag"), flt=flt)
                    assert rc1 == 0 and rc2 == 0
                    assert [r["ID"] for r in batch[qi]] == [r["ID"] for r in one] == [r["ID"] for r in want], (tag, field, flt, qi)
                    assert [r["Tag"] for r in batch[qi]] == [r["Tag"] for r in want]
                    assert np.allclose([r["@distance"] for r in batch[qi]], [r["@distance"] for r in want], rtol=1e-4, atol=1e-6)
    check("flat")
    for db in dbs:
        assert db.rebuild() == 0
    check("graph")       # (1500 rows, SearchQueueSize 500: both graphs are exact here)
    # the only vector field is resolved when the name is empty - not here (three fields): the reference's error, its code
    rc, msg = ddb.search_batch("T", "", Q, 5)
    assert rc != 0 and "queryField" in msg
    rc, msg = ddb.search_batch("T", "E", Q, 5, flt="NoSuchField > 3")
    rc2, msg2 = rdb.search("T", "E", Q[0], 5, flt="NoSuchField > 3")
    assert rc == rc2 != 0
    rc, msg = ddb.search_batch("Nope", "E", Q, 5)
    assert rc != 0 and "Table not found" in msg
    rc, msg = ddb.search_batch("T", "E", Q[:, :5], 5)
    assert rc != 0 and "dimension" in msg
    for db in dbs:
        db.close()
    ref.L.ref_config(4, 500, 1, 0, 16)
    dropin.L.ref_config(4, 500, 1, 0, 16)


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_concurrent_clients_are_micro_batched_and_match_reference(dropin, tmp_path):
    """16 client threads issuing single-vector DBServer::Search calls (what concurrent REST requests do): the drop-in
    coalesces them into device batches; every answer must equal the reference DBServer's answer to the same query,
    before and after a rebuild (flat and graph + tail)."""
    ref = Ref()
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 24, "metricType": "EUCLIDEAN"}]}
    X = data(3000, 24, 31)
    recs = [{"ID": int(i) + 7, "V": [float(x) for x in X[i]]} for i in range(3000)]
    Q = data(400, 24, 32)
    dbs = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        lib.L.ref_config(1, 500, 1, 0, 2)
        db = lib.db(str(tmp_path / name))
        assert db.create_table(schema) == 0 and db.insert("T", recs[:2500]) == 0
        dbs.append(db)
    for phase in range(2):
        sec_r, first_r = dbs[0].search_mt("T", "V", Q, 5, 4)
        sec_d, first_d = dbs[1].search_mt("T", "V", Q, 5, 16)
        assert sec_r >= 0 and sec_d >= 0
        assert (first_r == first_d).all(), phase
        # concurrent requests with the same device-compilable filter share device batches as well (r2)
        sec_r, first_r = dbs[0].search_mt("T", "V", Q[:200], 5, 4, flt="ID >= 1000 AND ID < 2600")
        sec_d, first_d = dbs[1].search_mt("T", "V", Q[:200], 5, 16, flt="ID >= 1000 AND ID < 2600")
        assert sec_r >= 0 and sec_d >= 0 and (first_r == first_d).all() and ((first_d >= 1000) & (first_d < 2600)).all(), phase
        # single requests in between are served too
        rc, res = dbs[1].search("T", "V", Q[0], 3, fields=("ID",), flt="ID < 100")
        assert rc == 0 and all(r["ID"] < 100 for r in res)
        if phase == 0:
            for db in dbs:
                assert db.rebuild() == 0 and db.insert("T", recs[2500:]) == 0
    for db in dbs:
        db.close()
    ref.L.ref_config(4, 500, 1, 0, 16)
    dropin.L.ref_config(4, 500, 1, 0, 16)


FILTER_SCHEMA = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                         {"name": "Tag", "dataType": "STRING"},
                                         {"name": "Price", "dataType": "FLOAT"},
                                         {"name": "Weight", "dataType": "DOUBLE"},
                                         {"name": "Small", "dataType": "SMALLINT"},
                                         {"name": "Big", "dataType": "BIGINT"},
                                         {"name": "Flag", "dataType": "BOOL"},
                                         {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 8, "metricType": "EUCLIDEAN"}]}
FILTERS = ["ID >= 100 AND ID < 500", "ID < 50 OR ID > 1700", "NOT (ID < 1000)", "Price < 0.25", "Price * 2 + 1 >= 2.5", "Weight <= 0.1 OR Price > 0.9",
           "Small % 7 = 3", "Big > 2000000000", "Flag = true", "NOT Flag", "(ID < 300 OR ID > 1500) AND Price < 0.5 AND Small <> 4",
           "@distance < 0.35", "@distance >= 0.2 AND ID < 1000", "@distance < 0.5 AND Price < 0.5", "ID / 2 = 50.5", "ID - Small > 1700",
           "Tag = 't3' AND ID >= 100", "Tag <> 't1'", "Tag = 't2' OR @distance < 0.1", "Tag LIKE 't%' AND Price < 0.05", "Tag = 'absent'",
           "Tag = 't4' AND Price < 0.3 AND @distance < 0.6"]


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
@pytest.mark.parametrize("prefilter,rebuild", [(0, False), (0, True), (1, False)])
def test_filter_compiler_matches_reference_dbserver(dropin, tmp_path, prefilter, rebuild):
    """every filter form - int / float / double / bool attributes, arithmetic, AND / OR / NOT, @distance
    (device predicate program), strings / LIKE and mixes of both (host predicate on the walk candidates) - returns through
    the drop-in DBServer exactly what the reference DBServer returns, in the three modes of Search(): brute force
    (no graph yet), graph + post-filter after Rebuild(), and PreFilter."""
    ref = Ref()
    n = 1800
    X = data(n, 8, 21)
    rng = np.random.default_rng(22)
    price, weight = rng.random(n), rng.random(n)
    recs = [{"ID": int(i), "Tag": "t%d" % (i % 5), "Price": float(np.float32(price[i])), "Weight": float(weight[i]), "Small": int(i % 11),
             "Big": int(i) * 3000000, "Flag": bool(i % 3 == 0), "V": [float(x) for x in X[i]]} for i in range(n)]
    Q = data(4, 8, 23)
    out = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        lib.L.ref_config(1, 500, 1, prefilter, 2)          # IntraQueryThreads = 1: deterministic on both sides
        db = lib.db(str(tmp_path / name))
        assert db.create_table(FILTER_SCHEMA) == 0
        for s in range(0, n, 600):
            assert db.insert("T", recs[s:s + 600]) == 0
        assert db.delete("T", [3, 4, 5, 1000, 1001]) == 0
        if rebuild:
            assert db.rebuild() == 0
        res = {}
        for flt in FILTERS:
            for qi, q in enumerate(Q):
                for limit in (10, 200):
                    res[(flt, qi, limit)] = db.search("T", "V", q, limit, fields=("ID",), flt=flt)
        out.append(res)
        db.close()
        lib.L.ref_config(4, 500, 1, 0, 4)
    nonempty = 0
    for key, (rc_r, r) in out[0].items():
        rc_d, d = out[1][key]
        assert rc_r == rc_d == 0, (key, rc_r, rc_d, r if rc_r else d)
        assert [x["ID"] for x in d] == [x["ID"] for x in r], (key, [x["ID"] for x in d][:12], [x["ID"] for x in r][:12])
        assert np.allclose([x["@distance"] for x in d], [x["@distance"] for x in r], rtol=1e-4, atol=1e-7), key
        nonempty += len(r) > 0
    assert nonempty > len(out[0]) * 0.8


def random_filters(seed, count):
    """Random filter expressions over FILTER_SCHEMA from a small grammar (numeric attributes, constants, + - * / %, the six
    comparisons, bool and string leaves, @distance, AND / OR / NOT, parentheses), depth-limited; seeded, so the same list on
    both sides."""
    rng = np.random.default_rng(seed)
    nums = ["ID", "Price", "Weight", "Small", "Big"]

    def const(kind):
        if kind == "ID":
            return str(int(rng.integers(0, 1800)))
        if kind == "Small":
            return str(int(rng.integers(0, 11)))
        if kind == "Big":      # (integer literals beyond int32 overflow the reference parser's stoi: now and then, both sides must reject them)
            return str(int(rng.integers(0, 1800 if rng.random() < 0.05 else 700)) * 3000000)
        return "%.3f" % rng.random()

    def arith(depth):
        r = rng.random()
        if depth <= 0 or r < 0.45:
            a = nums[int(rng.integers(0, len(nums)))]
            return a, a
        if r < 0.55:
            return "@distance", "Price"
        if r < 0.65:
            k = nums[int(rng.integers(0, len(nums)))]
            return const(k), k
        (l, lk), (r2, _) = arith(depth - 1), arith(depth - 1)
        op = ["+", "-", "*", "/", "%"][int(rng.integers(0, 5))]
        if op in "/%":                       # a constant, non-zero right-hand side: no division by zero on either side
            r2 = str(int(rng.integers(2, 9)))
        return "(%s %s %s)" % (l, op, r2), lk

    def leaf(depth):
        r = rng.random()
        if r < 0.1:
            return ["Flag = true", "Flag = false", "Flag", "NOT Flag"][int(rng.integers(0, 4))]
        if r < 0.2:
            return "Tag %s 't%d'" % (["=", "<>"][int(rng.integers(0, 2))], int(rng.integers(0, 6)))
        l, lk = arith(depth)
        op = ["<", "<=", "=", "<>", ">=", ">"][int(rng.integers(0, 6))]
        rhs = const(lk) if rng.random() < 0.7 else arith(depth - 1)[0]
        return "%s %s %s" % (l, op, rhs)

    def expr(depth):
        r = rng.random()
        if depth <= 0 or r < 0.35:
            return leaf(2)
        if r < 0.45:
            return "NOT (%s)" % expr(depth - 1)
        return "(%s) %s (%s)" % (expr(depth - 1), ["AND", "OR"][int(rng.integers(0, 2))], expr(depth - 1))

    return [expr(3) for _ in range(count)]


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
@pytest.mark.parametrize("rebuild", [False, True])
def test_filter_compiler_random_expressions(dropin, tmp_path, rebuild):
    """f4 fuzz: 80 seeded random filter expressions (tests/test_dropin.py::random_filters) through the drop-in DBServer and the
    reference DBServer on the same table: same status, same ids in the same order, same distances - in brute-force mode and
    after Rebuild() (graph walk + post-filter).  Whatever the reference's parser rejects the drop-in must reject too."""
    ref = Ref()
    n = 1800
    X = data(n, 8, 21)
    rng = np.random.default_rng(22)
    price, weight = rng.random(n), rng.random(n)
    recs = [{"ID": int(i), "Tag": "t%d" % (i % 5), "Price": float(np.float32(price[i])), "Weight": float(weight[i]), "Small": int(i % 11),
             "Big": int(i) * 3000000, "Flag": bool(i % 3 == 0), "V": [float(x) for x in X[i]]} for i in range(n)]
    Q = data(2, 8, 24)
    filters = random_filters(int(os.environ.get("EPS_FUZZ_SEED", "1234")), 80)
    out = []
    for lib, name in ((ref, "ref"), (dropin, "drop")):
        lib.L.ref_config(1, 500, 1, 0, 2)
        db = lib.db(str(tmp_path / name))
        assert db.create_table(FILTER_SCHEMA) == 0
        for s in range(0, n, 600):
            assert db.insert("T", recs[s:s + 600]) == 0
        assert db.delete("T", [7, 8, 900]) == 0
        if rebuild:
            assert db.rebuild() == 0
        out.append({(flt, qi): db.search("T", "V", q, 40, fields=("ID",), flt=flt) for flt in filters for qi, q in enumerate(Q)})
        db.close()
        lib.L.ref_config(4, 500, 1, 0, 4)
    ok = nonempty = 0
    for key, (rc_r, r) in out[0].items():
        rc_d, d = out[1][key]
        assert (rc_r == 0) == (rc_d == 0), (key, rc_r, rc_d)
        if rc_r != 0:
            continue
        ok += 1
        assert [x["ID"] for x in d] == [x["ID"] for x in r], (key, [x["ID"] for x in d][:12], [x["ID"] for x in r][:12])
        assert np.allclose([x["@distance"] for x in d], [x["@distance"] for x in r], rtol=1e-4, atol=1e-7), key
        nonempty += len(r) > 0
    assert ok > len(out[0]) * 0.9 and nonempty > ok * 0.5, (ok, nonempty, len(out[0]))


@pytest.mark.gpu
def test_filter_program_through_the_c_abi():
    """eps_index_set_filter_program on packed rows {i32 id; f32 price; u8 flag; pad; f64 w} against numpy: flat (stream and
    MFMA engines), with @distance, on 70k rows; and the candidate walk (eps_index_search_walk)."""
    import vectordb_amd as amd
    n, d = 70_000, 64
    X, Q = data(n, d, 31), data(9, d, 32)
    rng = np.random.default_rng(33)
    rows = np.zeros(n, dtype=np.dtype([("id", "<i4"), ("price", "<f4"), ("flag", "u1"), ("pad", "u1", 7), ("w", "<f8")]))
    rows["id"], rows["price"], rows["flag"], rows["w"] = np.arange(n), rng.random(n), rng.integers(0, 2, n), rng.random(n)
    ix = amd.GpuIndex(d, 0)
    ix.attach_rows(X)
    exact = ((X[None, :, :].astype(np.float64) - Q[:, None, :]) ** 2).sum(2) if n * len(Q) * d < 1e8 else None
    dist = np.stack([((X.astype(np.float64) - q) ** 2).sum(1) for q in Q])
    progs = [
        ([("i32", 0), ("const", 35000), ("<",), ("f32", 4), ("const", 0.5), ("<",), ("and",)], lambda dd: (rows["id"] < 35000) & (rows["price"] < 0.5)),
        ([("bool", 8), ("not",), ("f64", 16), ("const", 0.25), (">=",), ("or",)], lambda dd: (rows["flag"] == 0) | (rows["w"] >= 0.25)),
        ([("i32", 0), ("const", 7), ("%",), ("const", 3), ("=",)], lambda dd: rows["id"] % 7 == 3),
    ]
    for prog, ref_mask in progs:
        ix.set_filter_program(prog, rows)
        for eng in (amd.FLAT_STREAM, amd.FLAT_MFMA):
            ids, dd, cnt = ix.search(Q, 10, mode=amd.MODE_FLAT, flat_engine=eng)
            m = ref_mask(None)
            for qi in range(len(Q)):
                want = np.argsort(np.where(m, dist[qi], np.inf), kind="stable")[:10]
                assert list(ids[qi]) == list(want), (prog, eng, qi)
    # @distance: rows closer than the 200-th nearest are filtered out -> the answer starts at rank 200
    sd = np.sort(dist[0])
    thr = float(0.5 * (sd[199] + sd[200]))   # between two candidates: no fp32 boundary case
    ix.set_filter_program([("dist",), ("const", thr), (">",)], rows)
    ids, dd, cnt = ix.search(Q[:1], 10, mode=amd.MODE_FLAT)
    assert list(ids[0]) == list(np.argsort(dist[0], kind="stable")[200:210])
    ix.set_filter_program(None)
    # candidate walk: flat mode returns the cap closest visible rows
    wi, wd, wc = ix.search_walk(Q[:2], 10, 300, mode=amd.MODE_FLAT)
    for qi in range(2):
        assert int(wc[qi]) == 300 and list(wi[qi]) == list(np.argsort(dist[qi], kind="stable")[:300])
    ix.close()


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="needs oracle/_ref")
def test_configurations_beyond_the_device_ranges_are_answered_not_refused(dropin, tmp_path):
    """VERDICT r4 #10.  The reference accepts SearchQueueSize up to 10^7 and IntraQueryThreads = 128 at any out-degree (config/config.hpp:29,
    37-44); the device traversal refuses queues beyond 2^20 keys and IntraQueryThreads x out-degree beyond 2048 (EPS_DB_UNSUPPORTED_ERROR at
    the C ABI, test_reference_parameter_ranges_run_or_are_refused).  The reference never answers a Search with such an error, so the adapter
    answers with the exact scan - on a table where the reference's own graph search is exact too, the two must agree."""
    ref = Ref()
    n, d = 3000, 16
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "E", "dataType": "VECTOR_FLOAT", "dimensions": d, "metricType": "EUCLIDEAN"}]}
    X = data(n, d, 51)
    recs = [{"ID": int(i), "E": [float(x) for x in X[i]]} for i in range(n)]
    Q = data(6, d, 52)
    try:
        for T, L in ((128, 500), (4, 2_000_000)):
            dbs = []
            for lib, name in ((ref, "ref%d_%d" % (T, L)), (dropin, "drop%d_%d" % (T, L))):
                lib.L.ref_config(T if lib is dropin else 4, L if lib is dropin else 3000, 1, 0, 2)   # (the reference side: a configuration it runs in seconds, exact on 3000 rows)
                db = lib.db(str(tmp_path / name))
                assert db.create_table(schema) == 0 and db.insert("T", recs) == 0 and db.rebuild() == 0
                dbs.append(db)
            for q in Q:
                rc1, got = dbs[1].search("T", "E", q, 10)
                rc2, want = dbs[0].search("T", "E", q, 10)
                assert rc1 == 0 and rc2 == 0, (T, L, got)
                assert [r["ID"] for r in got] == [r["ID"] for r in want], (T, L)
            rc, batch = dbs[1].search_batch("T", "E", Q, 10)
            assert rc == 0 and [[r["ID"] for r in b] for b in batch] == [[r["ID"] for r in dbs[0].search("T", "E", q, 10)[1]] for q in Q]
            for db in dbs:
                db.close()
    finally:
        ref.L.ref_config(4, 500, 1, 0, 16)
        dropin.L.ref_config(4, 500, 1, 0, 16)
