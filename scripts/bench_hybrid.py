"""The hybrid search (GpuIndex.search_hybrid / eps_index_search_hybrid, csrc/hybrid.hip) on synthetic rows, beside the two things a caller can compare
it with.

Tables (seed 101, torch's device generator): n = 1M rows; the dense side 768 columns of N(0, 1); the sparse side bench_sparse.py's recipe - ~128
non-zeros per row over 30 522 columns, queries of ~32 non-zeros.  Both handles DOT_PRODUCT, k = 10, w_dense = 1, w_sparse = 0.5, device queries and
results, warm.  Per batch in {1, 64, 1024}, the median over `reps` calls of:
  hybrid       the call's hipEvent times read through stats(): kernel_ms (pass, merge, result conversion, the winners' terms) and main_kernel_ms (the
               fused pass alone); the pass's achieved bytes/s from its algorithmic row bytes (n * dim * 4 per tile of staged queries)
  torch        the same scores on the device by library calls: Q @ X.T, torch.sparse.mm on the CSR rows against the densified queries, the
               weighted add and topk - timed with device events around the four; it materialises two [batch][n] tables.  Its sums round
               differently, so the line reports how many top-1 ids agree with the hybrid call, not equality
  parts        a dense flat stream search and a sparse inverted-lists search of the same batch (k = 10 each): what the two terms cost apart - their
               two top-k lists do NOT answer the hybrid question
One JSON line per point.  Usage: python scripts/bench_hybrid.py [--rows 1000000] [--dim 768] [--sparse-dim 30522] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_sparse import HBM_PEAK, SEED, head, make_csr, median_ms

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--sparse-dim", type=int, default=30522)
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
    n, dim, sdim, k, wd, ws = a.rows, a.dim, a.sparse_dim, a.k, 1.0, 0.5
    gen = torch.Generator(device=dev).manual_seed(SEED)
    X = torch.randn((n, dim), generator=gen, device=dev)
    Q = torch.randn((1024, dim), generator=gen, device=dev)
    S = make_csr(torch, gen, n, sdim, 160, dev)
    SQ = make_csr(torch, gen, 1024, sdim, 40, dev)
    nnz = int(S[0][-1])
    torch.cuda.synchronize()
    ix = amd.GpuIndex(dim, "DOT_PRODUCT", device=0).use_torch_stream()
    ix.attach_rows(X)
    sx = amd.GpuSparseIndex(sdim, "DOT_PRODUCT").use_torch_stream()
    sx.attach_csr(*S)
    sx.build_inverted()
    S_torch = torch.sparse_csr_tensor(S[0], S[1].long(), S[2], size=(n, sdim))
    shape = dict(rows=n, dim=dim, sparse_dim=sdim, nnz_per_row=round(nnz / n, 1), k=k, w_dense=wd, w_sparse=ws, reps=a.reps)

    for b in (1, 64, 1024):
        q, sq = Q[:b].contiguous(), head(SQ, b)
        out = (torch.empty((b, k), dtype=torch.int64, device=dev),) + tuple(torch.empty((b, k), dtype=torch.float32, device=dev) for _ in range(3)) + \
              (torch.empty((b,), dtype=torch.int32, device=dev),)
        whole, main = median_ms(torch, ix, lambda: ix.search_hybrid(sx, q, sq, k, wd, ws, out=out), a.reps)
        tile = 1 if b == 1 else 4
        row_bytes = ((b + tile - 1) // tile) * n * dim * 4
        emit(route="hybrid", batch=b, kernel_ms=round(whole, 4), pass_ms=round(main, 4), queries_per_s=round(b / whole * 1e3, 1), row_bytes=row_bytes,
             row_bytes_per_s=round(row_bytes / main * 1e3, 0), hbm_fraction=round(row_bytes / main * 1e3 / HBM_PEAK, 4), nnz_per_query=round(int(SQ[0][b]) / b, 1),
             kernel="hybrid_tile_kernel: sparse terms into LDS accumulators per 512-row tile, dense rows through row_dists, one key per row", **shape)

        # ---- the torch route
        qd = torch.zeros((b, sdim), dtype=torch.float32, device=dev)
        qd[torch.repeat_interleave(torch.arange(b, device=dev), SQ[0][1:b + 1] - SQ[0][:b]), sq[1].long()] = sq[2]

        def torch_route():
            d = q @ X.T
            s = torch.sparse.mm(S_torch, qd.T).T
            return torch.topk(-wd * d - ws * s, k, dim=1, largest=False)
        try:
            torch_route()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                got = torch_route()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            t_ms = float(np.median(times))
            agree = float((got.indices[:, 0] == out[0][:, 0]).float().mean())
            emit(route="torch: Q @ X.T, torch.sparse.mm, add, topk", batch=b, ms=round(t_ms, 4), queries_per_s=round(b / t_ms * 1e3, 1),
                 hybrid_over_torch=round(whole / t_ms, 3), top1_ids_agree_with_hybrid=round(agree, 4), table_bytes=2 * b * n * 4, **shape)
        except Exception as e:   # (a torch build without sparse kernels for this device: said, not hidden)
            emit(route="torch: Q @ X.T, torch.sparse.mm, add, topk", batch=b, not_measured=repr(e)[:200], **shape)

        # ---- the parts
        o3 = (out[0], out[1], out[4])
        d_whole, d_main = median_ms(torch, ix, lambda: ix.search(q, k, out=o3, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM), a.reps)
        s_whole, s_main = median_ms(torch, sx, lambda: sx.search(sq, k, out=o3), a.reps)
        emit(route="parts: dense flat stream search + sparse inverted search", batch=b, dense_kernel_ms=round(d_whole, 4), dense_scan_ms=round(d_main, 4),
             sparse_kernel_ms=round(s_whole, 4), sparse_inverted_ms=round(s_main, 4), hybrid_over_parts=round(whole / (d_whole + s_whole), 3), **shape)
    ix.close()
    sx.close()
