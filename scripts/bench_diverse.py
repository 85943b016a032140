"""Diverse search (GpuIndex.search_diverse / eps_index_search_diverse) beside the two routes a caller has without it, both on search(fetch_k):
 (a) the pool's rows copied to the host (fetch_k x dim x 4 bytes per query) and the greedy MMR loop in numpy;
 (b) the same greedy loop in torch on the device: index_select of the pool's rows, batched pair distances (|c|^2 + |s|^2 - 2 c.s by bmm), the
     scores and an argmin per step - no row leaves the device.  Route (b) is the yardstick.
Before a time is taken every route's selection must EQUAL the call's on a table of ties (small-integer coordinates: every route's arithmetic is
exact there), for both pool sizes.  On the timed Gaussian table the routes' pair distances are a GEMM's, not the flat scan's: how many selected
ids differ from the call's is reported for the record, it is not a check.
Table: Gaussian rows, EUCLIDEAN, k = 10, fetch_k = 100, lambda = 0.5, batch 1 / 64 / 1024, and fetch_k = 1024 at batch 64.  Warm, device queries
and results for the call and (b); wall time around a run of calls with one synchronize at the end (at least `reps` calls and a quarter of a
second), the whole measurement repeated `rounds` times, routes alternating: min / median / max per route give the spread.  The call's line also
carries the selection kernel's own time (main_kernel_ms) and the bytes per second it achieved against its (k - 1) x np x dim x 4 per query.
One JSON line per (batch, fetch_k, route).
Usage: python scripts/bench_diverse.py [--rows 1000000] [--dim 768] [--reps 5] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

F = np.float32


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


def greedy(xp, d, P, k, lam, first_min):
    """the rule's loop, batched, on numpy or torch (xp): d [b][F] pool distances, P [b][F][dim] pool rows; returns positions [b][k].  Pair
    distances as |c|^2 + |s|^2 - 2 c.s; m seeded by the first selection, then a minimum; ties to the smaller position (first_min)"""
    b, Fk = d.shape
    lam, mu = F(lam), F(1) - F(lam)
    pn = (P * P).sum(-1)
    if xp is np:
        rows, cur, taken = np.arange(b), np.zeros(b, np.int64), np.zeros((b, Fk), bool)
    else:
        rows, cur = xp.arange(b, device=d.device), xp.zeros(b, dtype=xp.int64, device=d.device)
        taken = xp.zeros((b, Fk), dtype=xp.bool, device=d.device)
    out = [cur]
    m = None
    for t in range(1, k):
        taken[rows, cur] = True
        s = P[rows, cur]                                              # [b][dim]
        D = pn + pn[rows, cur][:, None] - 2 * (P @ s[:, :, None])[:, :, 0]
        m = D if m is None else xp.minimum(m, D)
        score = xp.where(taken, xp.inf, float(lam) * d - float(mu) * m)
        cur = first_min(score)
        out.append(cur)
    return xp.stack(out, 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
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
    k, lam = a.k, a.lam

    def torch_first_min(score):
        at = torch.where(score == score.min(1, keepdim=True).values, torch.arange(score.shape[1], device=score.device), score.shape[1])
        return at.min(1).values

    def numpy_first_min(score):
        return np.argmin(score, axis=1)   # (numpy: the first minimum)

    def route_host(ix, X, Q, fetch_k):
        """(a): search(fetch_k) to the host, the pool's rows to the host, numpy"""
        ids, dist, _ = ix.search(Q.cpu().numpy(), fetch_k, mode=amd.MODE_FLAT)
        P = X.index_select(0, torch.from_numpy(ids.reshape(-1)).to(dev)).cpu().numpy().reshape(len(ids), fetch_k, -1)
        pos = greedy(np, dist, P, k, lam, numpy_first_min)
        return np.take_along_axis(ids, pos, 1)

    def route_device(ix, X, Q, fetch_k, bufs):
        """(b): search(fetch_k) into device tensors, the loop in torch"""
        ids, dist, _ = ix.search(Q, fetch_k, out=bufs, mode=amd.MODE_FLAT)
        P = X.index_select(0, ids.reshape(-1)).view(ids.shape[0], fetch_k, -1)
        pos = greedy(torch, dist, P, k, lam, torch_first_min)
        return torch.gather(ids, 1, pos)

    def search_bufs(b, fetch_k):
        return (torch.empty((b, fetch_k), dtype=torch.int64, device=dev), torch.empty((b, fetch_k), dtype=torch.float32, device=dev),
                torch.empty(b, dtype=torch.int32, device=dev))

    # ---- equality on a table of ties, before any time is taken
    rng = np.random.default_rng(161)
    Xt = torch.from_numpy(rng.integers(-8, 9, (3000, 16)).astype(F)).to(dev)
    Qt = torch.from_numpy(rng.integers(-8, 9, (8, 16)).astype(F)).to(dev)
    it = amd.GpuIndex(16, "EUCLIDEAN", device=0).use_torch_stream()
    it.attach_rows(Xt)
    for fetch_k in (100, 1024):
        mine = it.search_diverse(Qt, k, fetch_k, lam=lam)[0]
        torch.cuda.synchronize()
        head = it.search(Qt, k, out=search_bufs(8, k), mode=amd.MODE_FLAT)[0]
        torch.cuda.synchronize()
        assert not torch.equal(mine, head), "the ties table's selection is the pool's head: it would check nothing"
        assert np.array_equal(route_host(it, Xt, Qt, fetch_k), mine.cpu().numpy()), ("route (a) differs from the call on the ties table", fetch_k)
        assert torch.equal(route_device(it, Xt, Qt, fetch_k, search_bufs(8, fetch_k)), mine), ("route (b) differs from the call on the ties table", fetch_k)
    it.close()
    emit(check="routes (a) and (b) select the call's ids on a 3000 x 16 table of ties", fetch_k=[100, 1024], k=k, lam=lam, queries=8)

    # ---- the timed table
    n, d = a.rows, a.dim
    g = torch.Generator(device=dev).manual_seed(162)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 19):
        e = min(n, s + (1 << 19))
        X[s:e] = torch.randn((e - s, d), generator=g, device=dev, dtype=torch.float32)
    Qall = torch.randn((1024, d), generator=torch.Generator(device=dev).manual_seed(163), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix = amd.GpuIndex(d, "EUCLIDEAN", device=0).use_torch_stream()
    ix.attach_rows(X)

    for b, fetch_k in ((1, 100), (64, 100), (1024, 100), (64, 1024)):
        Q = Qall[:b].contiguous()
        bufs = search_bufs(b, fetch_k)
        base = dict(rows=n, dim=d, k=k, fetch_k=fetch_k, lam=lam, batch=b)
        mine = ix.search_diverse(Q, k, fetch_k, lam=lam)
        torch.cuda.synchronize()
        routes = {"search_diverse": lambda: ix.search_diverse(Q, k, fetch_k, lam=lam),
                  "search(fetch_k) alone, device results": lambda: ix.search(Q, fetch_k, out=bufs, mode=amd.MODE_FLAT),
                  "(b) search(fetch_k) + the greedy loop in torch on the device": lambda: route_device(ix, X, Q, fetch_k, bufs),
                  "(a) search(fetch_k) + rows to the host + numpy": lambda: route_host(ix, X, Q, fetch_k)}
        differ = {"(b) search(fetch_k) + the greedy loop in torch on the device": int((route_device(ix, X, Q, fetch_k, bufs) != mine[0]).sum().item()),
                  "(a) search(fetch_k) + rows to the host + numpy": int((route_host(ix, X, Q, fetch_k) != mine[0].cpu().numpy()).sum())}
        times = {r: [] for r in routes}
        calls = {}
        for _ in range(a.rounds):   # the routes alternate: what one round sees of the machine, every route sees
            for r, fn in routes.items():
                ms, calls[r] = timed(torch, fn, a.reps)
                times[r].append(ms)
        ix.search_diverse(Q, k, fetch_k, lam=lam)
        torch.cuda.synchronize()
        st = ix.stats()
        med = {r: sorted(v)[len(v) // 2] for r, v in times.items()}
        for r in routes:
            v = sorted(times[r])
            extra = {}
            if r == "search_diverse":
                sel_bytes = b * (k - 1) * fetch_k * d * 4
                extra = dict(selection_kernel_ms=round(st["main_kernel_ms"], 4), selection_row_bytes=sel_bytes,
                             selection_GBps=round(sel_bytes / max(st["main_kernel_ms"], 1e-6) / 1e6, 1),
                             over_search_alone_ms=round(med[r] - med["search(fetch_k) alone, device results"], 4),
                             speedup_over_b=round(med["(b) search(fetch_k) + the greedy loop in torch on the device"] / med[r], 3),
                             speedup_over_a=round(med["(a) search(fetch_k) + rows to the host + numpy"] / med[r], 3))
            if r in differ:
                extra = dict(selected_ids_that_differ_from_the_call=differ[r], of=b * k)
            emit(route=r, ms_min=round(v[0], 4), ms_median=round(v[len(v) // 2], 4), ms_max=round(v[-1], 4), rounds=a.rounds, calls_per_round=calls[r],
                 **extra, **base)
    ix.close()
