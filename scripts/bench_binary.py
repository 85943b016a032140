"""The binary-vector scan (GpuBinaryIndex / eps_binary_index_search, csrc/binary.hip) on random bits, and the route a caller had before it: the same
rows as +-1 floats in a GpuIndex EUCLIDEAN flat search (distance = 4 x Hamming).

Tables: 1M x 768 and 10M x 768 bits (seed 20, torch's device generator); k = 10; nq in {1, 8, 64, 1024}; device queries and results, warm: the
median over `reps` calls of the call's hipEvent times read through stats() - kernel_ms (scan, merge and result conversion) and main_kernel_ms (the
scan launches alone).  Each line carries both floors of the scan - bytes: n * W * 4 * tile passes over the 8 TB/s HBM peak; instructions:
2 * W * n * nq lane instructions over CUs x 64 lanes x the device's clock as the runtime reports it - and the scan's achieved fraction of the
larger one.  `split4` lines answer the same batch in calls of 4 queries (the 4-query form of the kernel) and sum the calls' kernel_ms: what a narrow
tile would cost, the gaps between calls left out.  The dense route runs on the 1M table only (its floats are 3 GB; at
10M they are 30.7 GB) and its answers are asserted equal to the binary ones first.

Usage: python scripts/bench_binary.py [--rows 1000000 10000000] [--reps 7] [--skip-dense] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK = 8.0e12
SEED = 20
DIM = 768


def tile_of(nq, k):
    """the query tile binary_plan gives the batch, from binary_host.hpp's own text: its budget, its narrowest tile and binary_kpl's steps"""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vectordb_amd", "csrc", "binary_host.hpp")).read()
    budget, narrow = (int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("BIN_TILE_BUDGET", "BIN_MIN_TILE"))
    body = re.search(r"inline int binary_kpl\(int32_t k\) \{ return (.*?); \}", src).group(1)
    steps, widest = re.findall(r"k <= (\d+) \? (\d+)", body), int(body.rsplit(":", 1)[1])
    assert steps and body.count("?") == len(steps)
    kpl = next((int(p) for limit, p in steps if k <= int(limit)), widest)
    cap, t = max(narrow, budget // kpl), narrow
    while t < cap and t < nq:
        t <<= 1
    return t


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
    import ctypes
    from vectordb_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    khz = ctypes.c_int(0)   # hipDeviceAttributeClockRate = 5: the peak clock in kHz, from the runtime the library itself is bound to
    assert ctypes.CDLL(_lib.LIB_PATH).hipDeviceGetAttribute(ctypes.byref(khz), 5, 0) == 0 and khz.value > 0
    clock_hz = khz.value * 1e3
    k, W = a.k, DIM // 32
    batches = (1, 8, 64, 1024)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    Q = torch.randint(-2 ** 31, 2 ** 31, (1024, W), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)

    def outs(b, dt=torch.int32):
        return (torch.empty((b, k), dtype=torch.int64, device=dev), torch.empty((b, k), dtype=dt, device=dev), torch.empty((b,), dtype=torch.int32, device=dev))

    for n in a.rows:
        X = torch.randint(-2 ** 31, 2 ** 31, (n, W), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
        ix = amd.GpuBinaryIndex(DIM).use_torch_stream()
        ix.attach_rows(X)
        answers = {}
        for b in batches:
            q, o = Q[:b].contiguous(), outs(b)
            whole, main = median_ms(torch, ix, lambda: ix.search(q, k, out=o), a.reps)
            answers[b] = o
            tile = tile_of(b, k)
            passes = (b + tile - 1) // tile
            floor_bytes_ms = n * W * 4 * passes / HBM_PEAK * 1e3
            floor_valu_ms = 2.0 * W * n * b / (cus * 64 * clock_hz) * 1e3
            floor = max(floor_bytes_ms, floor_valu_ms)
            emit(route="binary scan", rows=n, dim=DIM, batch=b, k=k, tile=tile, tile_passes=passes, kernel_ms=round(whole, 4), scan_ms=round(main, 4),
                 queries_per_s=round(b / whole * 1e3, 1), floor_bytes_ms=round(floor_bytes_ms, 4), floor_valu_ms=round(floor_valu_ms, 4),
                 bound="HBM" if floor_bytes_ms >= floor_valu_ms else "VALU", fraction_of_floor=round(floor / main, 4), cus=cus, clock_mhz=round(clock_hz / 1e6),
                 table_bytes=n * W * 4, reps=a.reps, kernel="binary_scan_kernel: one row per lane, per-lane 16-byte loads, query words as scalar operands")
        for b in (8, 64):   # the same batch in calls of 4 queries: the narrow form, one launch chain per call
            q4 = [Q[i:i + 4].contiguous() for i in range(0, b, 4)]
            o4 = [outs(4) for _ in q4]
            ms = []
            for rep in range(a.reps + 2):
                total = 0.0
                for q, o in zip(q4, o4):
                    ix.search(q, k, out=o)
                    total += ix.stats()["kernel_ms"]   # (waits for the call: the sum leaves the gaps between calls out)
                if rep >= 2:
                    ms.append(total)
            assert torch.equal(torch.cat([o[0] for o in o4]), answers[b][0])
            emit(route="binary scan, split4", rows=n, dim=DIM, batch=b, k=k, tile=4, calls=len(q4), sum_kernel_ms=round(float(np.median(ms)), 4), reps=a.reps)
        if n == 1_000_000 and not a.skip_dense:
            # (bit - 0.5) * 2 per word bit: the +-1 image, built on the device
            shifts = torch.arange(32, device=dev, dtype=torch.int32)
            img = lambda t: (((t.unsqueeze(-1) >> shifts) & 1).reshape(t.shape[0], DIM).to(torch.float32) * 2 - 1).contiguous()
            Xf = torch.cat([img(X[s:s + 65536]) for s in range(0, n, 65536)])
            Qf = img(Q)
            dx = amd.GpuIndex(DIM, "EUCLIDEAN").use_torch_stream()
            dx.attach_rows(Xf)
            for b in batches:
                q, o = Qf[:b].contiguous(), outs(b, torch.float32)
                whole, main = median_ms(torch, dx, lambda: dx.search(q, k, out=o, mode=amd.MODE_FLAT), a.reps)
                assert torch.equal(o[0], answers[b][0]) and torch.equal(o[1], answers[b][1].to(torch.float32) * 4) and torch.equal(o[2], answers[b][2])
                st = dx.stats()
                emit(route="+-1 floats, GpuIndex EUCLIDEAN flat search", rows=n, dim=DIM, batch=b, k=k, kernel_ms=round(whole, 4), main_kernel_ms=round(main, 4),
                     queries_per_s=round(b / whole * 1e3, 1), main_kernel_bits=st["main_kernel_bits"], one_pass=st["one_pass"], table_bytes=n * DIM * 4,
                     answers_equal_binary=True, reps=a.reps)
            dx.close()
            del Xf, dx
        ix.close()
        del X, ix
