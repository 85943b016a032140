"""Radius search (GpuIndex.search_range / eps_index_search_range) against the only way the library had to the same rows: a flat search with
k = cap and a `@distance <= r` program, which runs the fp32 stream engine.  Table: unit-norm embedding-like rows (bench_legs.config_embedding_like's
recipe: Gaussian coordinates, the first 8 carry 4 x the scale), COSINE, one batch of queries; radii per query midway between its K-th and
(K + 1)-th neighbour for K = 10 and K = 500 (found by a flat search), so every query has K rows within its radius.  Three ways, warm, device
buffers, wall time around a run of calls with one synchronize at its end:
  1. search(k = cap) + program `@distance <= r` (one constant per call: the batch's median radius)      -> the stream engine
  2. search_range(flat_engine="stream")
  3. search_range(flat_engine="mfma_i8")   (the filter's operand width that served it is in main_kernel_bits)
One JSON line per (K, way).  Usage: python scripts/bench_range.py [--rows 10000000] [--dim 768] [--batch 1024] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def table(torch, amd, n, d, b, dev):
    scale = torch.ones((d,), dtype=torch.float32, device=dev)
    scale[:8] = 4.0
    g = torch.Generator(device=dev).manual_seed(77)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 19):
        e = min(n, s + (1 << 19))
        X[s:e] = torch.randn((e - s, d), generator=g, device=dev, dtype=torch.float32) * scale
    stream = torch.cuda.current_stream().cuda_stream
    amd.normalize_rows(X, only_if_nonzero=True, device=0, stream=stream)
    Q = torch.randn((b, d), generator=torch.Generator(device=dev).manual_seed(78), device=dev, dtype=torch.float32) * scale
    amd.normalize_rows(Q, only_if_nonzero=False, device=0, stream=stream)
    torch.cuda.synchronize()
    return X, Q


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import vectordb_amd as amd
    dev = torch.device("cuda:0")
    n, d, b = a.rows, a.dim, a.batch
    X, Q = table(torch, amd, n, d, b, dev)
    ix = amd.GpuIndex(d, "COSINE", device=0).use_torch_stream()
    ix.attach_rows(X)
    attr = np.zeros((n, 1), np.int32)   # (a program needs attribute rows; this one reads none of them)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def outs(k):
        return (torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b, k), dtype=torch.float32, device=dev),
                torch.empty((b,), dtype=torch.int32, device=dev))

    o = outs(512)
    ix.search(Q, 512, out=o, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_MFMA_I8)   # the neighbours the radii are taken from (and the mirror every later call finds built)
    torch.cuda.synchronize()
    dist = o[1].cpu().numpy()
    for K, cap in ((10, 64), (500, 1024)):
        radius = (0.5 * (dist[:, K - 1].astype(np.float64) + dist[:, K])).astype(np.float32)
        base = dict(rows=n, dim=d, batch=b, metric="COSINE", neighbours=K, cap=cap)
        # 1. the parent's way
        r_med = float(np.median(radius))
        ix.set_filter_program([("dist",), ("const", r_med), ("<=",)], attr.view(np.uint8), stride=4)
        os_ = outs(cap)
        ms = timed(torch, lambda: ix.search(Q, cap, out=os_, mode=amd.MODE_FLAT), a.reps)
        st = ix.stats()
        emit(way="search k=cap + @distance <= r", ms=round(ms, 3), main_kernel_bits=st["main_kernel_bits"], rows_per_query=float(os_[2].float().mean()), **base)
        ix.set_filter_program(None)
        # 2., 3.
        orr = (os_[0], os_[1], os_[2], torch.empty((b,), dtype=torch.int64, device=dev))
        for eng in ("stream", "mfma_i8"):
            ms = timed(torch, lambda: ix.search_range(Q, radius, cap, flat_engine=eng, out=orr), a.reps)
            st = ix.stats()
            tot = orr[3].cpu().numpy()
            emit(way="search_range " + eng, ms=round(ms, 3), main_kernel_bits=st["main_kernel_bits"], main_kernel_ms=round(st["main_kernel_ms"], 3),
                 rows_per_query=float(tot.mean()), candidates_per_query=round(st["rerank_rows"] / b, 1), overflow_queries=st["overflow_queries"],
                 i8_rotated=st["i8_rotated"], **base)
    ix.close()
