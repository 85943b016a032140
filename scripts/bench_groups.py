"""Grouped search (GpuIndex.search_groups / eps_index_search_groups) against what a caller did before it existed: search(k'), ids to the host, drop
repeated groups there, and double k' while a query holds fewer than k groups and its answer was full.  Table: Gaussian rows, EUCLIDEAN, k = 10,
batch 1 / 64 / 1024.  Group layouts: 8 rows per group (consecutive rows), Zipf-sized groups, and the adversarial table - one group owns the
n - 100 closest rows of every query (rows scaled towards the origin; the 100 others are shifted away and are groups of their own).
Per (layout, batch), in one process: engine auto, pages (benign layouts only: on the adversarial table it is n / page_rows stream scans per call),
scan, and the caller's loop (adversarial table: batch 1 only - k' doubles up to n).  The answers of all routes are compared - ids, distance
bits, group keys, counts - BEFORE a time is taken; a mismatch ends the run.  Warm, device queries and results, wall time around a run of calls
with one synchronize at the end (at least `reps` calls and a quarter of a second).  The scan's algorithmic bytes - (n d 4 + n 4) per 4 queries
plus 16 G per query - over the call's time are reported as a fraction of 8 TB/s; set_groups' set-up time (host relabelling + upload) once per layout.
One JSON line per (layout, batch, route).  Usage: python scripts/bench_groups.py [--rows 1000000] [--dim 768] [--reps 5] [--out FILE]"""
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
    g = torch.Generator(device=dev).manual_seed(131)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 19):
        e = min(n, s + (1 << 19))
        X[s:e] = torch.randn((e - s, d), generator=g, device=dev, dtype=torch.float32)
    Qall = torch.randn((1024, d), generator=torch.Generator(device=dev).manual_seed(132), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix = amd.GpuIndex(d, "EUCLIDEAN", device=0).use_torch_stream()
    ix.attach_rows(X)
    rng = np.random.default_rng(133)
    far = min(100, n // 2)
    layouts = [("8 rows per group", np.arange(n, dtype=np.int64) // 8), ("zipf", np.minimum(rng.zipf(1.3, n), n // 2).astype(np.int64)),
               ("adversarial", np.where(np.arange(n) < n - far, -1, np.arange(n)).astype(np.int64))]

    def outs(b):
        return (torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b, k), dtype=torch.float32, device=dev),
                torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b,), dtype=torch.int32, device=dev))

    def equal(x, y):
        return bool(torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)) and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]))

    def caller_loop(Qh, keys):
        """what a caller does with the existing calls; returns the answer as numpy arrays and the last k'"""
        b = Qh.shape[0]
        kp = 4 * k
        while True:
            h_ids, h_dist, _ = ix.search(Qh, kp, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_AUTO)   # (host queries: the k' ids and distances come to the host)
            res = (np.full((b, k), -1, np.int64), np.full((b, k), np.inf, np.float32), np.zeros((b, k), np.int64), np.zeros(b, np.int32))
            short = False
            for q in range(b):
                valid = h_ids[q] >= 0
                gk = keys[h_ids[q][valid]]
                first = np.sort(np.unique(gk, return_index=True)[1])[:k]
                m = len(first)
                res[0][q, :m], res[1][q, :m], res[2][q, :m], res[3][q] = h_ids[q][valid][first], h_dist[q][valid][first], gk[first], m
                short = short or (m < k and valid.all())
            if not short or kp >= n:
                return res, kp
            kp = min(n, 2 * kp)

    for name, keys in layouts:
        if name == "adversarial":   # the same rows, pulled towards the origin / pushed away: every query's n - 100 closest rows are one group
            X[:n - far] *= 0.1
            X[n - far:] += 5.0
            torch.cuda.synchronize()
            ix.attach_rows(X)
        t0 = time.perf_counter()
        ix.set_groups(keys)
        setup_ms = (time.perf_counter() - t0) * 1e3
        info = ix.groups_info()
        G = info["n_groups"]
        emit(layout=name, route="set_groups", rows=n, ms=round(setup_ms, 2), n_groups=G, largest_group=info["largest_group"])
        for b in (1, 64, 1024):
            Q = Qall[:b].contiguous()
            Qh = Q.cpu().numpy()
            base = dict(layout=name, rows=n, dim=d, k=k, batch=b, n_groups=G)
            routes = ["auto", "scan"] + (["pages"] if name != "adversarial" else [])
            o = {r: outs(b) for r in routes}
            for r in routes:
                ix.search_groups(Q, k, engine=r, out=o[r])
            torch.cuda.synchronize()
            assert all(equal(o["auto"], o[r]) for r in routes), (base, "engines differ")
            loop = name != "adversarial" or b == 1
            if loop:
                res, kp = caller_loop(Qh, keys)
                got = [t.cpu().numpy() for t in o["auto"]]
                assert all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
                           for x, y in zip(got, res)), (base, "the caller's loop differs")
            for r in routes:
                ms, reps = timed(torch, lambda: ix.search_groups(Q, k, engine=r, out=o[r]), a.reps)
                st, gi = ix.stats(), ix.groups_info()
                line = dict(route="search_groups " + r, ms=round(ms, 4), engines=gi["last_engines"], scan_queries=gi["last_scan_queries"], answers_equal=True, calls=reps, **base)
                if r == "scan":
                    tiles = (b + 3) // 4
                    bytes_ = tiles * (n * d * 4 + n * 4) + 16 * G * b
                    line.update(scan_bytes=bytes_, fraction_of_8TBps=round(bytes_ / (ms * 1e-3) / 8e12, 4), last_chunk_scan_ms=round(st["main_kernel_ms"], 4),
                                last_chunk_queries=st["main_kernel_queries"])
                emit(**line)
            if loop:
                ms, reps = timed(torch, lambda: caller_loop(Qh, keys), 1 if name == "adversarial" else a.reps)
                emit(route="caller's loop: search(k') + host dedupe, k' doubling", ms=round(ms, 4), last_k_prime=kp, answers_equal=True, calls=reps, **base)
            else:
                emit(route="caller's loop: search(k') + host dedupe, k' doubling", ms=None, note="not measured: k' doubles up to n for every query of the batch", **base)
    ix.close()
