"""Multi-vector queries (GpuIndex.search_multi / eps_index_search_multi) beside the two things a reader can hold them against.
 * The route a PyTorch-ROCm user writes today, on device tensors: Q @ X.T, scatter_reduce(amin) by label, a sum over the bag's vectors, topk.  Its
   distances are a GEMM's, its sum torch's: how its answer differs - group keys that differ, the largest relative score difference - is reported
   for the record, it is not a check.
 * search_groups(engine="scan") over the same vectors as plain queries, on the same handle in the same run: the same scan kernel without the
   t x G x 8 read-back of the table per bag, the sum and the matches.  The whole-table form may cost that read-back's bytes at the stream rate
   more, plus the run-to-run spread seen in this run; the script prints both and the difference.
Table: Gaussian rows, DOT_PRODUCT, k = 10, bags of 32 vectors, batch 1 / 16; the three group layouts of scripts/bench_groups.py; candidate lists
of 1 000 / 10 000 groups (one list for the batch, drawn once).  Before a time is taken the candidate form is compared with the whole-table form
where the list names every group of its answer.  Warm, device inputs and results; wall time around a run of calls with one synchronize at the
end (at least `reps` calls and a quarter of a second), the whole measurement repeated `rounds` times, routes alternating: min / median / max per
route give the spread.  One JSON line per (layout, batch, route).
Usage: python scripts/bench_multi.py [--rows 1000000] [--dim 768] [--bag 32] [--reps 5] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def timed(torch, fn, reps):
    """(ms per call, calls timed)"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = 2 if one > 0.5 else max(reps, min(2000, int(0.25 / one)))
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
    ap.add_argument("--bag", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--lists", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
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
    n, d, k, t = a.rows, a.dim, a.k, a.bag
    g = torch.Generator(device=dev).manual_seed(151)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 19):
        e = min(n, s + (1 << 19))
        X[s:e] = torch.randn((e - s, d), generator=g, device=dev, dtype=torch.float32)
    Qall = torch.randn((max(a.batches) * t, d), generator=torch.Generator(device=dev).manual_seed(152), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix = amd.GpuIndex(d, "DOT_PRODUCT", device=0).use_torch_stream()
    ix.attach_rows(X)
    rng = np.random.default_rng(153)
    far = min(100, n // 2)
    layouts = [("8 rows per group", np.arange(n, dtype=np.int64) // 8), ("zipf", np.minimum(rng.zipf(1.3, n), n // 2).astype(np.int64)),
               ("adversarial", np.where(np.arange(n) < n - far, -1, np.arange(n)).astype(np.int64))]

    for name, keys in layouts:
        ix.set_groups(keys)
        uniq, label = np.unique(keys, return_inverse=True)
        G = len(uniq)
        label_d = torch.from_numpy(label.astype(np.int64)).to(dev)
        uniq_d = torch.from_numpy(uniq).to(dev)

        def torch_route(Q, b):
            """(group keys [b][k], score [b][k]) the way a torch user writes it: GEMM, amin by label, sum over the bag, topk"""
            out_k, out_s = [], []
            for j in range(b):   # (a bag at a time: [t][n] floats of distances, not [b t][n])
                dist = -(Q[j * t:(j + 1) * t] @ X.T)
                best = torch.full((t, G), float("inf"), device=dev).scatter_reduce(1, label_d.expand(t, n), dist, "amin", include_self=True)
                s, lab = torch.topk(best.sum(0), min(k, G), largest=False)
                out_k.append(uniq_d[lab])
                out_s.append(s)
            return torch.stack(out_k), torch.stack(out_s)

        for b in a.batches:
            Q = Qall[:b * t].contiguous()
            off = np.arange(b + 1, dtype=np.int64) * t
            base = dict(layout=name, rows=n, dim=d, k=k, bag=t, batch=b, n_groups=G)
            whole = ix.search_multi((Q, off), k)
            torch.cuda.synchronize()
            routes = {"search_multi, whole table": lambda: ix.search_multi((Q, off), k),
                      "search_groups(engine=scan) over the same vectors": lambda: ix.search_groups(Q, k, engine="scan"),
                      "torch: Q @ X.T, scatter_reduce(amin), sum, topk": lambda: torch_route(Q, b)}
            lists = {}
            for m in a.lists:
                if m > G:
                    continue
                rest = np.setdiff1d(uniq, np.unique(whole[0].cpu().numpy()))
                cand = np.concatenate([np.unique(whole[0].cpu().numpy()), rng.choice(rest, size=max(0, m - (G - len(rest))), replace=False)])[:m]
                cand_d = torch.from_numpy(rng.permutation(cand).astype(np.int64)).to(dev)
                got = ix.search_multi((Q, off), k, cand_keys=cand_d)
                torch.cuda.synchronize()
                assert all(torch.equal(x, y) for x, y in zip(got, whole)), (base, m, "the candidate form differs from the whole-table form")
                lists[m] = cand_d
                routes["search_multi, %d candidate groups" % m] = (lambda c: lambda: ix.search_multi((Q, off), k, cand_keys=c))(cand_d)
            tk, ts = torch_route(Q, b)
            torch.cuda.synchronize()
            differ = int((tk != whole[0]).sum().item())
            rel = float(((ts - whole[1]).abs() / whole[1].abs().clamp_min(1e-30)).max().item())
            times = {r: [] for r in routes}
            calls = {}
            for _ in range(a.rounds):   # the routes alternate: what one round sees of the machine, every route sees
                for r, fn in routes.items():
                    ms, calls[r] = timed(torch, fn, a.reps)
                    times[r].append(ms)
            st_ms = {}
            for r, fn in routes.items():
                if r.startswith("search_"):
                    fn()
                    torch.cuda.synchronize()
                    st_ms[r] = ix.stats()["main_kernel_ms"]
            readback = 8 * t * G * b
            for r in routes:
                v = sorted(times[r])
                extra = {}
                if r == "search_multi, whole table":
                    gs = sorted(times["search_groups(engine=scan) over the same vectors"])
                    extra = dict(readback_bytes=readback, over_search_groups_ms=round(v[len(v) // 2] - gs[len(gs) // 2], 4),
                                 search_groups_spread_ms=round(gs[-1] - gs[0], 4), spread_ms=round(v[-1] - v[0], 4),
                                 readback_GBps_if_all_of_the_difference=round(readback / max(v[len(v) // 2] - gs[len(gs) // 2], 1e-6) / 1e6, 1))
                if r.startswith("torch"):
                    extra = dict(group_keys_that_differ=differ, of=int(whole[0].numel()), largest_relative_score_difference=rel)
                emit(route=r, ms_min=round(v[0], 4), ms_median=round(v[len(v) // 2], 4), ms_max=round(v[-1], 4), rounds=a.rounds, calls_per_round=calls[r],
                     last_main_kernel_ms=round(st_ms[r], 4) if r in st_ms else None, **extra, **base)
    ix.close()
