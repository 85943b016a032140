"""The half-vector scan (GpuHalfIndex / eps_half_index_search, csrc/half.hip) on random fp16 rows, and the route a caller had before it: the same
values as floats in a GpuIndex EUCLIDEAN flat search (MODE_FLAT).

Tables: 1M x 768 and 10M x 768 fp16, standard normal (seed 22, torch's device generator); k = 10; nq in {1, 8, 64, 1024}; device queries and
results, warm: the median over `reps` calls of the call's hipEvent times on the handle's stream, read through stats() - kernel_ms (query
preparation, seed pass, scan, merges and result conversion) and main_kernel_ms (the main scan launches alone).  Each line carries both floors of the
main scan - bytes: n * 2 d_pad per tile pass over the 8 TB/s HBM peak; matrix: 2 * n * nq * d_pad operations over 2.5 PFLOP/s - the scan's achieved
fraction of the larger one, and the share of the rounds of 64 rows that went through the hit path instead of ending at the vote: of the main launch,
whose slices start from the seed, and of the seed launch over the prefix, whose slices all start open - the scan without a seed, on the same call.
The dense route runs on the 1M table only (its floats are 3 GB; at 10M they are 30.7 GB); before anything is timed both routes answer a
100 000-row table of integers -8..8, where every fp32 distance is exact, and their ids, distances and counts are asserted equal.

Usage: python scripts/bench_half.py [--rows 1000000 10000000] [--reps 7] [--skip-dense] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK = 8.0e12
F16_PEAK = 2.5e15
SEED = 22
DIM = 768


def median_ms(torch, ix, fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    whole, main, s = [], [], None
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        s = ix.stats()
        whole.append(s["kernel_ms"])
        main.append(s["main_kernel_ms"])
    return float(np.median(whole)), float(np.median(main)), s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
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
    k, d_pad = a.k, (DIM + 31) // 32 * 32
    batches = (1, 8, 64, 1024)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    normal = lambda m: torch.randn((m, DIM), generator=gen, device=dev, dtype=torch.float32).to(torch.float16)
    ints = lambda m: torch.randint(-8, 9, (m, DIM), generator=gen, device=dev, dtype=torch.int32).to(torch.float16)
    floats = lambda t: torch.cat([t[s:s + 65536].to(torch.float32) for s in range(0, t.shape[0], 65536)])
    Q = normal(1024)

    def outs(b):
        return (torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b, k), dtype=torch.float32, device=dev), torch.empty((b,), dtype=torch.int32, device=dev))

    if not a.skip_dense:   # integers: both routes are exact, so they must agree to the last id
        Xs, Qs = ints(100_000), ints(64)
        hx, dx = amd.GpuHalfIndex(DIM, "EUCLIDEAN").use_torch_stream(), amd.GpuIndex(DIM, "EUCLIDEAN").use_torch_stream()
        torch.cuda.synchronize()   # (the index copies the table at attach, on its own stream: the producer must be done)
        hx.attach_rows(Xs)
        Xsf, Qsf = floats(Xs), floats(Qs)
        torch.cuda.synchronize()
        dx.attach_rows(Xsf)
        oh, od = outs(64), outs(64)
        hx.search(Qs, k, out=oh)
        dx.search(Qsf, k, out=od, mode=amd.MODE_FLAT)
        torch.cuda.synchronize()
        assert torch.equal(oh[0], od[0]) and torch.equal(oh[1], od[1]) and torch.equal(oh[2], od[2])
        emit(check="integers -8..8: half scan == fp32 flat search", rows=100_000, dim=DIM, batch=64, k=k, equal=True, seeded=hx.stats()["seeded"])
        hx.close()
        dx.close()
        del Xs, Xsf, hx, dx

    for n in a.rows:
        X = torch.cat([normal(min(1_000_000, n - s)) for s in range(0, n, 1_000_000)])
        ix = amd.GpuHalfIndex(DIM, "EUCLIDEAN").use_torch_stream()
        torch.cuda.synchronize()
        ix.attach_rows(X)
        for b in batches:
            q, o = Q[:b].contiguous(), outs(b)
            whole, main, s = median_ms(torch, ix, lambda: ix.search(q, k, out=o), a.reps)
            passes = (b + s["live_columns"] - 1) // s["live_columns"]
            floor_bytes_ms = n * 2 * d_pad * passes / HBM_PEAK * 1e3
            floor_mfma_ms = 2.0 * n * b * d_pad / F16_PEAK * 1e3
            floor = max(floor_bytes_ms, floor_mfma_ms)
            seed_rounds = (s["seed_rows"] + 63) // 64 * passes
            emit(route="half scan", rows=n, dim=DIM, batch=b, k=k, live_columns=s["live_columns"], kpl=s["kpl"], tile_passes=passes, kernel_ms=round(whole, 4),
                 scan_ms=round(main, 4), queries_per_s=round(b / whole * 1e3, 1), floor_bytes_ms=round(floor_bytes_ms, 4), floor_mfma_ms=round(floor_mfma_ms, 4),
                 bound="HBM" if floor_bytes_ms >= floor_mfma_ms else "MFMA", fraction_of_floor=round(floor / main, 4), seeded=s["seeded"], seed_rows=s["seed_rows"],
                 rounds=s["rounds"], hit_rounds=s["hit_rounds"], hit_share_seeded=round(s["hit_rounds"] / max(s["rounds"], 1), 4),
                 hit_share_unseeded_prefix=round(s["seed_hit_rounds"] / max(seed_rounds, 1), 4), table_bytes=(n + 63) // 64 * 64 * (2 * d_pad + 4), reps=a.reps,
                 kernel="half_scan_kernel: 4 wavefronts x 64-row rounds, v_mfma_f32_16x16x32_f16, query tile in LDS, lane-private seeded thresholds")
        if n == 1_000_000 and not a.skip_dense:
            dx = amd.GpuIndex(DIM, "EUCLIDEAN").use_torch_stream()
            Xf, Qf = floats(X), floats(Q)
            torch.cuda.synchronize()
            dx.attach_rows(Xf)
            for b in batches:
                q, o = Qf[:b].contiguous(), outs(b)
                whole, main, st = median_ms(torch, dx, lambda: dx.search(q, k, out=o, mode=amd.MODE_FLAT), a.reps)
                emit(route="the same values as floats, GpuIndex EUCLIDEAN flat search", rows=n, dim=DIM, batch=b, k=k, kernel_ms=round(whole, 4),
                     main_kernel_ms=round(main, 4), queries_per_s=round(b / whole * 1e3, 1), main_kernel_bits=st["main_kernel_bits"], one_pass=st["one_pass"],
                     table_bytes=n * DIM * 4, reps=a.reps)
            dx.close()
            del dx, Xf
        ix.close()
        del X, ix
