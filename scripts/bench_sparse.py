"""The sparse-vector scan (GpuSparseIndex / eps_sparse_index_search, csrc/sparse.hip) on synthetic rows, and the route a caller had before it: the
same rows densified into a GpuIndex flat search.

Recipe (seed 101, torch's device generator): a vector over `dim` columns has `slots` candidate columns - sorted draws from [0, dim - slots) plus
0 .. slots - 1, so they are distinct and increasing - of which each is kept with probability 0.8, and values +-U[0.25, 4).  Rows: slots = 160
(~128 non-zeros), queries: slots = 40 (~32 non-zeros).  Default table: n = 1M rows, dim = 30 522 (a BERT vocabulary: SPLADE's column space).

Per nq in {1, 8, 64, 1024}, k = 10, EUCLIDEAN, device queries and results, warm: the median over `reps` calls of the call's hipEvent times read
through stats() - kernel_ms (scan, merge and result conversion) and main_kernel_ms (the scan launch alone).  One JSON line per point: queries/s
from kernel_ms, the scan's achieved bytes/s from its algorithmic bytes (8 * nnz + 8 * n per tile of staged queries; a tile is 4 queries, 2 for
nq = 2, 1 for nq = 1), and that as a fraction of the 8 TB/s HBM peak DESIGN quotes.

The dense route: eps_index_create takes dim <= 8192, so a 30 522-column field has NO dense route at all.  The comparison therefore runs on a second
table the dense index can hold: dim = 8192, n chosen so that n * dim * 4 bytes stay within --dense-gb (default 8 GB: n = 262 144), the same recipe,
served by both indices in the same run - GpuIndex flat search (EPS_FLAT_AUTO) on the densified rows beside the sparse scan on the CSR.  Their
distances differ in rounding (the dense kernels sum in another order, with fused multiply-adds), so the line reports how many top-1 ids agree, not
equality.

--engine scan|inverted|both and --metric EUCLIDEAN|COSINE|DOT_PRODUCT (one or more) pick what runs on the flagship table.  With `inverted` or `both`
the handle builds its inverted lists (GpuSparseIndex.build_inverted, csrc/sparse_inverted.hip; DOT_PRODUCT and COSINE only) - the line of the build
holds its wall time and the image's bytes - and the same batches run on them; with `both` the scan runs first on the same handle, before the
lists exist, and every inverted line says whether ids, distance bits and counts equal the scan's.  --skip-dense leaves the dense comparison out.

Usage: python scripts/bench_sparse.py [--rows 1000000] [--dim 30522] [--reps 7] [--dense-gb 8] [--engine scan] [--metric EUCLIDEAN] [--skip-dense]
                                      [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK = 8.0e12
SEED = 101


def make_csr(torch, gen, n, dim, slots, dev, keep=0.8):
    """(offsets int64[n + 1], indices int32[nnz], values float32[nnz]) on the device, by the recipe above"""
    offs, idxs, vals = [torch.zeros(1, dtype=torch.int64, device=dev)], [], []
    total = 0
    for s in range(0, n, 1 << 16):
        m = min(n, s + (1 << 16)) - s
        cols = torch.sort(torch.randint(0, dim - slots, (m, slots), generator=gen, device=dev), dim=1).values + torch.arange(slots, device=dev)
        mask = torch.rand((m, slots), generator=gen, device=dev) < keep
        v = (torch.rand((m, slots), generator=gen, device=dev) * 3.75 + 0.25) * (torch.randint(0, 2, (m, slots), generator=gen, device=dev) * 2 - 1)
        offs.append(torch.cumsum(mask.sum(1), 0) + total)
        total = int(offs[-1][-1])
        idxs.append(cols[mask].to(torch.int32))
        vals.append(v[mask].to(torch.float32))
    return torch.cat(offs).contiguous(), torch.cat(idxs).contiguous(), torch.cat(vals).contiguous()


def head(t, m):
    e = int(t[0][m])
    return t[0][:m + 1].cpu().numpy(), t[1][:e].contiguous(), t[2][:e].contiguous()


def median_ms(torch, ix, fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    whole, main = [], []
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        s = ix.stats()
        whole.append(s["kernel_ms"])
        main.append(s["main_kernel_ms"])
    return float(np.median(whole)), float(np.median(main))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=30522)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dense-gb", type=float, default=8.0)
    ap.add_argument("--engine", choices=("scan", "inverted", "both"), default="scan")
    ap.add_argument("--metric", nargs="+", choices=("EUCLIDEAN", "COSINE", "DOT_PRODUCT"), default=["EUCLIDEAN"])
    ap.add_argument("--skip-dense", action="store_true")
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
    k = a.k
    batches = (1, 8, 64, 1024)

    def outs(b):
        return (torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b, k), dtype=torch.float32, device=dev),
                torch.empty((b,), dtype=torch.int32, device=dev))

    def sparse_points(X, Q, n, dim, table, metric="EUCLIDEAN", engine="scan"):
        ix = amd.GpuSparseIndex(dim, metric).use_torch_stream()
        ix.attach_csr(*X)
        nnz = int(X[0][-1])
        res = {}
        if engine != "inverted" or metric == "EUCLIDEAN":   # (EUCLIDEAN has no inverted form: the scan is what there is to measure)
            for b in batches:   # (no inverted lists yet: the handle answers by the scan)
                q, o = head(Q, b), outs(b)
                whole, main = median_ms(torch, ix, lambda: ix.search(q, k, out=o), a.reps)
                tile = 1 if b == 1 else (2 if b == 2 else 4)
                scan_bytes = ((b + tile - 1) // tile) * (8 * nnz + 8 * n + (4 * n if metric == "COSINE" else 0))
                emit(route="sparse scan", metric=metric, table=table, rows=n, dim=dim, nnz=nnz, nnz_per_row=round(nnz / n, 1), nnz_per_query=round(int(Q[0][b]) / b, 1),
                     batch=b, k=k, kernel_ms=round(whole, 4), scan_ms=round(main, 4), queries_per_s=round(b / whole * 1e3, 1), scan_bytes=scan_bytes,
                     scan_bytes_per_s=round(scan_bytes / main * 1e3, 0), hbm_fraction=round(scan_bytes / main * 1e3 / HBM_PEAK, 4), reps=a.reps,
                     last_engine=ix.inverted_info()["last_engine"],
                     kernel="sparse_scan_kernel: one row per lane read straight from the CSR arrays, queries staged in LDS")
                res[b] = o
        if engine != "scan" and metric != "EUCLIDEAN":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.build_inverted()   # (synchronises)
            build_s = time.perf_counter() - t0
            info = ix.inverted_info()
            emit(route="inverted lists: build", metric=metric, table=table, rows=n, dim=dim, nnz=nnz, build_wall_ms=round(build_s * 1e3, 2),
                 image_bytes=8 * nnz + 8 * (dim + 1), csr_bytes=8 * nnz + 8 * (n + 1), longest_column=info["longest_column"], postings=info["postings"])
            for b in batches:
                q, o = head(Q, b), outs(b)
                whole, main = median_ms(torch, ix, lambda: ix.search(q, k, out=o), a.reps)
                same = None
                if b in res:
                    same = bool(torch.equal(o[0], res[b][0]) and torch.equal(o[1].view(torch.int32), res[b][1].view(torch.int32)) and torch.equal(o[2], res[b][2]))
                emit(route="inverted lists", metric=metric, table=table, rows=n, dim=dim, nnz=nnz, nnz_per_row=round(nnz / n, 1),
                     nnz_per_query=round(int(Q[0][b]) / b, 1), batch=b, k=k, kernel_ms=round(whole, 4), inverted_ms=round(main, 4),
                     queries_per_s=round(b / whole * 1e3, 1), reps=a.reps, last_engine=ix.inverted_info()["last_engine"], same_bits_as_scan=same,
                     kernel="sparse_inverted_kernel: term at a time on the postings, per-row fp32 accumulators in LDS")
                res[b] = o
        return ix, res

    # ---- the flagship shape
    gen = torch.Generator(device=dev).manual_seed(SEED)
    n, dim = a.rows, a.dim
    X = make_csr(torch, gen, n, dim, 160, dev)
    Q = make_csr(torch, gen, 1024, dim, 40, dev)
    torch.cuda.synchronize()
    for metric in a.metric:
        ix, _ = sparse_points(X, Q, n, dim, "flagship", metric, a.engine)
        ix.close()
    del X, Q, ix
    if a.skip_dense:
        sys.exit(0)

    # ---- beside the dense route, at a size the dense index holds
    dim2 = 8192
    n2 = 1 << int(np.floor(np.log2(a.dense_gb * 2 ** 30 / (dim2 * 4))))
    gen = torch.Generator(device=dev).manual_seed(SEED + 1)
    X = make_csr(torch, gen, n2, dim2, 160, dev)
    Q = make_csr(torch, gen, 1024, dim2, 40, dev)

    def densify(t, m):
        out = torch.zeros((m, dim2), dtype=torch.float32, device=dev)
        rows = torch.repeat_interleave(torch.arange(m, device=dev), t[0][1:m + 1] - t[0][:m])
        e = int(t[0][m])
        out[rows, t[1][:e].long()] = t[2][:e]
        return out

    Xd, Qd = densify(X, n2), densify(Q, 1024)
    torch.cuda.synchronize()
    sp, sparse_out = sparse_points(X, Q, n2, dim2, "dense-comparable: n * dim * 4 = %.1f GB" % (n2 * dim2 * 4 / 2 ** 30))
    dx = amd.GpuIndex(dim2, "EUCLIDEAN", device=0).use_torch_stream()
    dx.attach_rows(Xd)
    for b in batches:
        q, o = Qd[:b].contiguous(), outs(b)
        whole, main = median_ms(torch, dx, lambda: dx.search(q, k, out=o, mode=amd.MODE_FLAT, flat_engine=amd.FLAT_AUTO), a.reps)
        st = dx.stats()
        agree = float((o[0][:, 0] == sparse_out[b][0][:, 0]).float().mean())
        emit(route="densified rows, GpuIndex flat search (auto)", table="dense-comparable", rows=n2, dim=dim2, batch=b, k=k, kernel_ms=round(whole, 4),
             main_kernel_ms=round(main, 4), queries_per_s=round(b / whole * 1e3, 1), main_kernel_bits=st["main_kernel_bits"], one_pass=st["one_pass"],
             dense_bytes=n2 * dim2 * 4, top1_ids_agree_with_sparse=round(agree, 4), reps=a.reps)
    sp.close()
    dx.close()
