"""The bookkeeping of tests/stream_gate.py on the CPU: its exact answers against exact_ref, and every case of tests/test_gpu_stream_order.py seen to
FAIL for the right reason - with `real` and `decoy` swapped in the numpy comparison the case must fail, and a decoy that shares a first id with the
real input must be refused as vacuous before anything is launched."""
import numpy as np
import pytest

import among_ref as ar
import exact_ref as xr
import range_ref as rr
import stream_gate as sg

F = np.float32

CASES = {
    "a stream (1, 10)": lambda: sg.search_case("A", 1, 10),
    "a stream (70, 100)": lambda: sg.search_case("A", 70, 100),
    "a stream paged k 1500": lambda: sg.search_case("A", 3, 1500),
    "a matrix engines nq 300": lambda: sg.search_case("B", 300, 10),
    "a one pass nq 1": lambda: sg.search_case("B", 1, 10, seed=21),
    "a one pass nq 8": lambda: sg.search_case("B", 8, 10, seed=21),
    "a range A": lambda: sg.range_case("A"),
    "a range B": lambda: sg.range_case("B"),
    "a among one list": lambda: sg.among_case("A", 6, 10, True),
    "a among a list per query": lambda: sg.among_case("A", 6, 10, False),
    "a select": lambda: sg.select_case("A"),
    "b among (32)": lambda: sg.among_case("A", 4, 10, True, seed=32, longest=300),
    "b among (34)": lambda: sg.among_case("A", 5, 10, False, seed=34, longest=2000),
    "b range (36)": lambda: sg.range_case("A", seed=36),
    "c deleted nq 8": lambda: sg.filter_case("B", 8, 10, "deleted"),
    "c column nq 8": lambda: sg.filter_case("B", 8, 10, "column"),
    "c deleted nq 300": lambda: sg.filter_case("B", 300, 10, "deleted"),
    "d queries 255 KB": lambda: sg.search_case("A", 1020, 10, seed=41),
    "d queries 300 KB": lambda: sg.search_case("A", 1200, 10, seed=41),
    "d among (42) one list": lambda: sg.among_case("A", 6, 10, True, seed=42),
    "d among (42) lists": lambda: sg.among_case("A", 6, 10, False, seed=42),
    "d range (43)": lambda: sg.range_case("A", seed=43),
    "e merge topk": lambda: sg.merge_case("topk"),
    "e merge range": lambda: sg.merge_case("range"),
    "e merge select": lambda: sg.merge_case("select"),
    "e normalize": lambda: sg.normalize_case(),
}


@pytest.mark.parametrize("which", sorted(CASES))
def test_every_case_fails_when_real_and_decoy_are_swapped(which):
    case = sg.check_case(CASES[which]())
    sg.same(case["want"], case["want"], which, case["names"])
    decoys = [key for key in case if key.startswith("want_")]
    assert decoys
    for key in decoys:
        with pytest.raises(AssertionError, match="places differ|against"):
            sg.same(case[key], case["want"], which, case["names"])      # the device answered for the decoy
        with pytest.raises(AssertionError, match="VACUOUS"):
            sg.check_case(dict(case, **{key: case["want"]}))          # a decoy that changes nothing is refused
    for o in case["want"]:
        assert not (np.asarray(o) == sg.FILL).all(), "an expected output is all %d: it could not be told from an output never written" % sg.FILL


def test_host_sizes_straddle_the_staging_threshold():
    assert 1020 * 64 * 4 <= (256 << 10) < 1200 * 64 * 4


def test_exact_answers_are_exact_refs():
    """topk_np / int_dists / int_ref against exact_ref, among_ref and range_ref on a small table of the same kind, with ties"""
    X, Q = xr.make(sg.TABLE, 3001, 8, 9, seed=5)
    ref = xr.Ref(X, Q, 0)
    assert np.array_equal(sg.int_dists(X, Q), ref.d64) and np.array_equal(sg.int_ref(X, Q).d64, ref.d64)
    assert np.array_equal(sg.first_ids(X, Q), sg.topk_np(X, Q, 1)[0][:, 0])
    vis = np.random.default_rng(1).random(3001) < 0.5
    for k, v in ((1, None), (10, None), (200, vis)):
        ids, dist, cnt, _ = sg.topk_np(X, Q, k, v)
        xr.check_exact(ids, dist, cnt, X, Q, 0, k, visible=v, ref=ref)
    d32 = rr.dist32(X, Q, 0)
    radius = np.sort(d32, axis=0)[40].astype(F)
    sg.same(sg.topk_np(X, Q, 16, vis, radius=radius), rr.numpy_range(d32, radius, 16, vis), "range")
    lists = [np.random.default_rng(q).choice(3001, size=50 + q, replace=False) for q in range(9)]
    sg.same(sg.topk_np(X, Q, 10, sg.rows_mask(3001, lists, 9) & vis[:, None])[:3], ar.numpy_among(d32, lists, 10, vis), "among")
    with pytest.raises(AssertionError, match="small integers"):
        sg.int_dists(X[:, :7] + F(0.25), Q[:, :7])


def test_same_compares_distance_bits_and_took_names_the_source():
    a = (np.array([[1, 2]], np.int64), np.array([[1.0, 2.0]], F), np.array([2], np.int32))
    b = (a[0], np.nextafter(a[1], F(9)), a[2])
    sg.same(a, a, "x")
    sg.same((a[0], np.array([[-0.0, 2.0]], F), a[2]), (a[0], np.array([[0.0, 2.0]], F), a[2]), "-0 and +0 are one distance")
    with pytest.raises(AssertionError, match="dist"):
        sg.same(b, a, "x")
    with pytest.raises(AssertionError, match="int32"):
        sg.same((a[0], a[1], a[2].astype(np.int64)), a, "x")
    real, decoy = np.array([[1], [2]]), np.array([[3], [4]])
    assert [sg.took(g, real, decoy) for g in (real, decoy, np.array([[1], [4]]), np.array([[1], [9]]))] == ["real", "decoy", "a mix", "neither"]
    with pytest.raises(AssertionError):
        sg.starts_as_fill([np.zeros(3)], "x")
    sg.starts_as_fill([np.full(3, sg.FILL)], "x")
