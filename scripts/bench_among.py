"""Search among given rows (GpuIndex.search_among / eps_index_search_among) against the route a caller had to the same answer before: build the
complement of the list as a deleted bitset, upload it (set_deleted, n / 8 bytes from the host - counted), and run a flat search, on the fp32 stream
engine (EPS_FLAT_STREAM) and with the library's own choice (EPS_FLAT_AUTO).  Table: Gaussian rows, EUCLIDEAN, k = 10; lists of random rows without
repeats.  Per (list length m, batch nq), in one process:
  1. search_among, ids on the device already                      2. search_among, ids uploaded from the host by the call (8 m bytes - counted)
  3. set_deleted(complement) + search(flat, stream)               4. set_deleted(complement) + search(flat, auto)
and for per-query lists (one of m rows per query; the bitset route needs one set_deleted + one single-query search PER QUERY, since one bitset
serves a whole call) the same four.  The answers of all routes are compared - ids, distance bits, counts - BEFORE a time is taken; a mismatch
ends the run.  Warm, device queries and results, wall time around a run of calls with one synchronize at the end (scripts/bench_range.py's `timed`; here the
run is at least `reps` calls AND a quarter of a second long: a single-query call takes 70 us).
The complement bitsets are built before the clock starts: what the caller pays to BUILD its bitset or its list is not part of either side.
One JSON line per (shape, route).  Usage: python scripts/bench_among.py [--rows 1000000] [--dim 768] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def timed(torch, fn, reps):
    """(ms per call, calls timed): warm, then at least `reps` calls and at least a quarter of a second of them, one synchronize at the end"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(reps, min(2000, int(0.25 / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, reps


def complement(n, rows):
    gone = np.ones((n + 7) // 8 * 8, bool)
    gone[rows] = False
    gone[n:] = False
    return np.packbits(gone, bitorder="little")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import torch
    import vectordb_amd as amd
    dev = torch.device("cuda:0")
    n, d, k = a.rows, a.dim, a.k
    g = torch.Generator(device=dev).manual_seed(91)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 19):
        e = min(n, s + (1 << 19))
        X[s:e] = torch.randn((e - s, d), generator=g, device=dev, dtype=torch.float32)
    Qall = torch.randn((1024, d), generator=torch.Generator(device=dev).manual_seed(92), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix = amd.GpuIndex(d, "EUCLIDEAN", device=0).use_torch_stream()
    ix.attach_rows(X)
    rng = np.random.default_rng(93)

    def outs(b):
        return (torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b, k), dtype=torch.float32, device=dev),
                torch.empty((b,), dtype=torch.int32, device=dev))

    def equal(x, y):
        return bool(torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)) and torch.equal(x[2], y[2]))

    # ---- one list for the batch
    for m in (1_000, 10_000, 100_000):
        rows = rng.choice(n, size=m, replace=False).astype(np.int64)
        d_rows = torch.from_numpy(rows).to(dev)
        bits = complement(n, rows)
        torch.cuda.synchronize()
        for b in (1, 64, 1024):
            Q = Qall[:b].contiguous()
            base = dict(form="shared", rows=n, dim=d, k=k, list=m, batch=b)
            o_dev, o_host, o_flat = outs(b), outs(b), outs(b)
            ix.search_among(Q, d_rows, k, out=o_dev)
            ix.search_among(Q, rows, k, out=o_host)
            torch.cuda.synchronize()
            st = ix.stats()
            same = {"among, host ids": equal(o_dev, o_host)}
            for name, eng in (("stream", amd.FLAT_STREAM), ("auto", amd.FLAT_AUTO)):
                ix.set_deleted(bits)
                ix.search(Q, k, out=o_flat, mode=amd.MODE_FLAT, flat_engine=eng)
                torch.cuda.synchronize()
                same["flat " + name] = equal(o_dev, o_flat)
            ix.set_deleted(None)
            assert all(same.values()), (base, same)
            ms, reps = timed(torch, lambda: ix.search_among(Q, d_rows, k, out=o_dev), a.reps)
            emit(route="search_among, device ids", ms=round(ms, 4), main_kernel_ms=round(ix.stats()["main_kernel_ms"], 4), dist_evals=st["dist_evals"], answers_equal=True, calls=reps, **base)
            ms, reps = timed(torch, lambda: ix.search_among(Q, rows, k, out=o_host), a.reps)
            emit(route="search_among, host ids", ms=round(ms, 4), answers_equal=True, calls=reps, **base)
            for name, eng in (("stream", amd.FLAT_STREAM), ("auto", amd.FLAT_AUTO)):
                def route():
                    ix.set_deleted(bits)
                    ix.search(Q, k, out=o_flat, mode=amd.MODE_FLAT, flat_engine=eng)
                ms, reps = timed(torch, route, a.reps)
                stf = ix.stats()
                emit(route="set_deleted + flat " + name, ms=round(ms, 4), main_kernel_bits=stf["main_kernel_bits"], one_pass=stf["one_pass"], answers_equal=True, calls=reps, **base)
            ix.set_deleted(None)

    # ---- one list per query
    m, b = 10_000, 64
    Q = Qall[:b].contiguous()
    lists = [rng.choice(n, size=m, replace=False).astype(np.int64) for _ in range(b)]
    cat = np.concatenate(lists)
    off = np.arange(b + 1, dtype=np.int64) * m
    d_cat = torch.from_numpy(cat).to(dev)
    bitsets = [complement(n, x) for x in lists]
    base = dict(form="per query", rows=n, dim=d, k=k, list=m, batch=b)
    o_dev, o_host, o_flat = outs(b), outs(b), outs(b)
    ix.search_among(Q, d_cat, k, offsets=off, out=o_dev)
    ix.search_among(Q, cat, k, offsets=off, out=o_host)
    torch.cuda.synchronize()
    st = ix.stats()
    assert equal(o_dev, o_host), base

    def per_query(eng):
        for j in range(b):
            ix.set_deleted(bitsets[j])
            ix.search(Q[j:j + 1], k, out=(o_flat[0][j:j + 1], o_flat[1][j:j + 1], o_flat[2][j:j + 1]), mode=amd.MODE_FLAT, flat_engine=eng)

    for name, eng in (("stream", amd.FLAT_STREAM), ("auto", amd.FLAT_AUTO)):
        per_query(eng)
        torch.cuda.synchronize()
        assert equal(o_dev, o_flat), (base, name)
    ix.set_deleted(None)
    ms, reps = timed(torch, lambda: ix.search_among(Q, d_cat, k, offsets=off, out=o_dev), a.reps)
    emit(route="search_among, device ids", ms=round(ms, 4), main_kernel_ms=round(ix.stats()["main_kernel_ms"], 4), dist_evals=st["dist_evals"], answers_equal=True, calls=reps, **base)
    ms, reps = timed(torch, lambda: ix.search_among(Q, cat, k, offsets=off, out=o_host), a.reps)
    emit(route="search_among, host ids", ms=round(ms, 4), answers_equal=True, calls=reps, **base)
    for name, eng in (("stream", amd.FLAT_STREAM), ("auto", amd.FLAT_AUTO)):
        ms, reps = timed(torch, lambda: per_query(eng), max(1, a.reps // 2))
        stf = ix.stats()
        emit(route="%d x (set_deleted + flat %s, one query)" % (b, name), ms=round(ms, 4), main_kernel_bits=stf["main_kernel_bits"], one_pass=stf["one_pass"], answers_equal=True, calls=reps, **base)
    ix.set_deleted(None)
    ix.close()
