"""Grouped search with m rows per group (GpuIndex.search_group_rows / eps_index_search_group_rows) against what a caller did before it existed:
search_groups, the group keys to the host, one candidate list per (query, group) pair from the caller's own copy of the grouping (the rows sorted
by key, made once), and search_among over nq x k pseudo-queries - the queries replicated k times - with k = m.  search_groups alone is timed
beside them, so the second phase's cost is the difference.  Table: Gaussian rows, EUCLIDEAN, k = 10, m = 3 / 10, batch 1 / 64 / 1024; the three
group layouts of scripts/bench_groups.py.  Both routes' answers are compared - ids, distance bits, row counts - BEFORE a time is taken; a
mismatch ends the run.  The caller's route is not run where its lists exceed --max-cand entries (a huge group named by many queries).
Warm, device queries and results, wall time around a run of calls with one synchronize at the end (at least `reps` calls and a quarter of a
second; 2 calls where one takes over half a second).  The second phase's bytes are rows gathered x d x 4 (the rows of the winning groups: the sum
of group_sizes, no filter installed) over the difference of the two times.  One JSON line per (layout, batch, m, route).
Usage: python scripts/bench_group_rows.py [--rows 1000000] [--dim 768] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--ms", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-cand", type=int, default=1 << 25)
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
    Qall = torch.randn((max(a.batches), d), generator=torch.Generator(device=dev).manual_seed(132), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix = amd.GpuIndex(d, "EUCLIDEAN", device=0).use_torch_stream()
    ix.attach_rows(X)
    rng = np.random.default_rng(133)
    far = min(100, n // 2)
    layouts = [("8 rows per group", np.arange(n, dtype=np.int64) // 8), ("zipf", np.minimum(rng.zipf(1.3, n), n // 2).astype(np.int64)),
               ("adversarial", np.where(np.arange(n) < n - far, -1, np.arange(n)).astype(np.int64))]

    for name, keys in layouts:
        if name == "adversarial":   # the same rows, pulled towards the origin / pushed away: every query's n - 100 closest rows are one group
            X[:n - far] *= 0.1
            X[n - far:] += 5.0
            torch.cuda.synchronize()
            ix.attach_rows(X)
        ix.set_groups(keys)
        # the caller's own copy of the grouping, made once: the rows sorted by key
        order = np.argsort(keys, kind="stable").astype(np.int64)
        uniq, start = np.unique(keys[order], return_index=True)
        end = np.append(start[1:], n)
        t0 = time.perf_counter()
        ix.search_group_rows(Qall[:1].contiguous(), k, 1)   # the first call builds the rows by group
        torch.cuda.synchronize()
        info = ix.groups_info()
        G = info["n_groups"]
        emit(layout=name, route="first call (builds the rows by group)", rows=n, ms=round((time.perf_counter() - t0) * 1e3, 2), n_groups=G,
             largest_group=info["largest_group"])

        def callers_route(Q, m):
            """returns (ids [b * k][m], dist, counts [b * k]) as device tensors, or None where the lists are too long"""
            b = Q.shape[0]
            _, _, gk, cnt = ix.search_groups(Q, k)
            gk_h, cnt_h = gk.cpu().numpy().reshape(-1), cnt.cpu().numpy()
            valid = (np.arange(k)[None, :] < cnt_h[:, None]).reshape(-1)
            pos = np.searchsorted(uniq, gk_h)
            pos[~valid] = 0
            lens = np.where(valid, end[pos] - start[pos], 0)
            offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            if offsets[-1] > a.max_cand:
                return None
            cand = np.concatenate([order[start[p]:end[p]] for p, v in zip(pos, valid) if v]) if valid.any() else np.zeros(0, np.int64)
            return ix.search_among(Q.repeat_interleave(k, dim=0), cand, m, offsets=offsets)

        for b in a.batches:
            Q = Qall[:b].contiguous()
            tg, _ = timed(torch, lambda: ix.search_groups(Q, k), a.reps)
            for m in a.ms:
                base = dict(layout=name, rows=n, dim=d, k=k, m=m, batch=b, n_groups=G)
                new = ix.search_group_rows(Q, k, m)
                old = callers_route(Q, m)
                torch.cuda.synchronize()
                if old is not None:
                    same = (torch.equal(new[0].reshape(b * k, m), old[0]) and torch.equal(new[1].reshape(b * k, m).view(torch.int32), old[1].view(torch.int32))
                            and torch.equal(new[3].reshape(-1), old[2]))
                    assert same, (base, "the two routes differ")
                gathered = int(new[4].sum().item())
                tn, reps = timed(torch, lambda: ix.search_group_rows(Q, k, m), a.reps)
                st = ix.stats()
                second = max(tn - tg, 1e-6)
                emit(route="search_group_rows", ms=round(tn, 4), search_groups_alone_ms=round(tg, 4), second_phase_ms=round(second, 4), rows_gathered=gathered,
                     second_phase_bytes=gathered * d * 4, second_phase_TBps=round(gathered * d * 4 / (second * 1e-3) / 1e12, 4),
                     last_gather_kernel_ms=round(st["main_kernel_ms"], 4), answers_equal=True if old is not None else "not compared: the caller's route was not run", calls=reps, **base)
                if old is not None:
                    to, reps = timed(torch, lambda: callers_route(Q, m), a.reps)
                    emit(route="caller: search_groups + keys to host + lists + search_among", ms=round(to, 4), ratio_caller_over_new=round(to / tn, 3), answers_equal=True,
                         calls=reps, **base)
                else:
                    emit(route="caller: search_groups + keys to host + lists + search_among", ms=None, note="not run: its lists exceed %d entries" % a.max_cand, **base)
    ix.close()
