"""Radius search (GpuIndex.search_range / eps_index_search_range) against the only way the library had to the same rows: a flat search with
k = cap and a `@distance <= r` program, which runs the fp32 stream engine.  Table: unit-norm embedding-like rows (bench_legs.config_embedding_like's
recipe: Gaussian coordinates, the first 8 carry 4 x the scale), COSINE, one batch of queries; radii per query midway between its K-th and
(K + 1)-th neighbour for K = 10 and K = 500 (found by a flat search), so every query has K rows within its radius.  Three ways, warm, device
buffers, wall time around a run of calls with one synchronize at its end:
  1. search(k = cap) + program `@distance <= r` (one constant per call: the batch's median radius)      -> the stream engine
  2. search_range(flat_engine="stream")
  3. search_range(flat_engine="mfma_i8")   (the filter's operand width that served it is in main_kernel_bits)
One JSON line per (K, way).  Usage: python scripts/bench_range.py [--rows 10000000] [--dim 768] [--batch 1024] [--reps 3] [--out FILE]

--shards G: the merge step of a sharded radius search instead.  The table's rows i mod G go to G indices on device 0 (set_id_map(s, G)); per shape
(queries, cap) every shard answers the batch straight into its slot of one gathered buffer (the layout of eps_range_pack_bytes), then the merge
is timed on those bytes: eps_merge_range_packed (merge_rank_kernel) and, beside it, eps_merge_topk_packed with k = cap - the serial kernel, the
only earlier way to merge such lists; it computes no totals and no counts.  hipEvents around every call, device buffers, the two alternating,
median of --merge-reps warm calls.  Two fillings: "typical" - radii at every query's cap-th neighbour over the whole table, so the lists hold
about cap / G keys each - and "full" - an infinite radius, every list full.  One GPU only: the transport between GPUs is not part of this number.
One JSON line per (shape, filling)."""
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


def event_us(torch, fns, reps):
    """median device time of each fn in us: events around every call, the fns alternating inside one loop"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, fn in enumerate(fns):
            ev[i][r][0].record()
            fn()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) for a, b in e])) * 1e3 for e in ev]


def shards_mode(a, emit):
    import torch
    import vectordb_amd as amd
    dev = torch.device("cuda:0")
    n, d, G = a.rows, a.dim, a.shards
    X, Qall = table(torch, amd, n, d, max(a.batch, 16), dev)
    stream = torch.cuda.current_stream().cuda_stream
    whole = amd.GpuIndex(d, "COSINE", device=0).use_torch_stream()
    whole.attach_rows(X)
    parts = []
    for s in range(G):
        ix = amd.GpuIndex(d, "COSINE", device=0).use_torch_stream()
        ix.attach_rows(X[s::G].contiguous())
        ix.set_id_map(s, G)
        parts.append(ix)
    for b, cap in ((a.batch, 10), (a.batch, 64), (a.batch, 1024), (16, 8192)):
        Q = Qall[:b].contiguous()
        inf = np.full(b, np.inf, np.float32)
        top = whole.search_range(Q, inf, cap)   # the cap closest of the whole table
        torch.cuda.synchronize()
        kth = top[1][:, cap - 1].cpu().numpy()
        pack = amd.range_pack_bytes(b, cap)
        nk = b * cap
        buf = torch.zeros((G * pack,), dtype=torch.uint8, device=dev)

        def views(s):
            o = buf[s * pack:(s + 1) * pack]
            t0, d0, c0 = nk * 8, nk * 8 + b * 8, nk * 12 + b * 8   # ids | totals | distances | counts
            return (o[:t0].view(torch.int64).view(b, cap), o[d0:c0].view(torch.float32).view(b, cap), o[c0:c0 + b * 4].view(torch.int32),
                    o[t0:d0].view(torch.int64))

        out = (torch.empty((b, cap), dtype=torch.int64, device=dev), torch.empty((b, cap), dtype=torch.float32, device=dev),
               torch.empty((b,), dtype=torch.int32, device=dev), torch.empty((b,), dtype=torch.int64, device=dev))
        t_d, t_i = torch.empty((b, cap), dtype=torch.float32, device=dev), torch.empty((b, cap), dtype=torch.int64, device=dev)
        for filling, radius in (("typical", kth), ("full", inf)):
            def shard_calls():
                for s, ix in enumerate(parts):
                    ix.search_range(Q, radius, cap, out=views(s))
            shard_ms = timed(torch, shard_calls, a.reps) / G
            new_us, old_us = event_us(torch, [lambda: amd.merge_range_packed(buf, pack, G, b, cap, out=out, stream=stream),
                                              lambda: amd.merge_topk_packed(buf, pack, nk * 8 + b * 8, G, b, cap, t_d, t_i, stream=stream)], a.merge_reps)
            torch.cuda.synchronize()
            lens = torch.stack([views(s)[2] for s in range(G)]).float()
            unsharded = whole.search_range(Q, radius, cap)
            torch.cuda.synchronize()
            emit(shards=G, rows=n, dim=d, batch=b, cap=cap, filling=filling, keys_per_list=round(float(lens.mean()), 1), search_range_ms_per_shard=round(shard_ms, 3),
                 merge_range_us=round(new_us, 1), merge_topk_packed_us=round(old_us, 1), merge_reps=a.merge_reps,
                 equals_unsharded=bool(all(torch.equal(x, y) for x, y in zip(out, unsharded))), same_ids_as_topk_merge=bool(torch.equal(out[0], t_i)))
    whole.close()
    for ix in parts:
        ix.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shards", type=int, default=0, help="G > 0: time the merge of G shards' answers (see the module text)")
    ap.add_argument("--merge-reps", type=int, default=50)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.shards > 0:
        shards_mode(a, emit)
        sys.exit(0)
    import torch
    import vectordb_amd as amd
    dev = torch.device("cuda:0")
    n, d, b = a.rows, a.dim, a.batch
    X, Q = table(torch, amd, n, d, b, dev)
    ix = amd.GpuIndex(d, "COSINE", device=0).use_torch_stream()
    ix.attach_rows(X)
    attr = np.zeros((n, 1), np.int32)   # (a program needs attribute rows; this one reads none of them)

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
