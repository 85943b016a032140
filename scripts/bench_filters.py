"""Search under per-query filters (GpuIndex.search_filters / eps_index_search_filters) beside the route a caller has without it on the same build:
per program, set_filter_program(append_only) + search(MODE_FLAT) over that program's queries.

Table n x dim (default 1M x 768, U[0, 1)), k = 10, batch 64 and 1024, P programs `tenant == j` of which every query names one, per-program
selectivity s: a row carries tenant j < P with probability s each (tenants overlap: the column is a set of P flag bytes), so every program shows
s x n rows whatever P is.  Per point: warm-up calls, then `reps` timed calls each ended by a stream sync; the median and the spread
(max - min) / median over the timed calls are reported, for the two engines forced and for the loop.  One JSON line per (point, route) to stdout
and to --out.

    python scripts/bench_filters.py --out profiles/r18_search_filters.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vectordb_amd as amd  # noqa: E402


def timed(ix, call, warm, reps):
    for _ in range(warm):
        call()
    ix.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ix.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    return float(np.median(ms)), float((ms.max() - ms.min()) / np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--programs", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--selectivity", type=float, nargs="+", default=[0.001, 0.01, 0.1, 0.5])
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = rng.random((a.n, a.dim), dtype=np.float32)
    ix = amd.GpuIndex(a.dim, "EUCLIDEAN", device=0)
    ix.attach_rows(X)
    out = open(a.out, "a") if a.out else None

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for s in a.selectivity:
        rows = (rng.random((a.n, 64)) < s).astype(np.uint8)   # flag byte j: the row belongs to tenant j
        for P in a.programs:
            progs = [[("bool", j)] for j in range(P)]
            for b in a.batches:
                Q = rng.random((b, a.dim), dtype=np.float32)
                qp = (np.arange(b) % P).astype(np.int32)
                base = dict(n=a.n, dim=a.dim, k=a.k, batch=b, programs=P, selectivity=s, warm=a.warm, reps=a.reps)

                def loop():
                    for j in range(P):
                        ix.set_filter_program(progs[j], rows, append_only=True)
                        ix.search(Q[qp == j], a.k, mode=amd.MODE_FLAT)
                    ix.set_filter_program(None)

                want = None
                for engine in ("lists", "planes"):   # (AUTO is the list engine while its lists fit the scratch cap)
                    got = ix.search_filters(Q, a.k, progs, qp, rows, append_only=True, engine=engine)
                    want = got if want is None else want
                    equal = all(np.array_equal(x, y) for x, y in zip(got, want))
                    ms, spread = timed(ix, lambda: ix.search_filters(Q, a.k, progs, qp, rows, append_only=True, engine=engine), a.warm, a.reps)
                    st = ix.stats()
                    emit(route="search_filters " + engine, ms=round(ms, 4), spread=round(spread, 3), main_kernel_ms=round(st["main_kernel_ms"], 4),
                         dist_evals=st["dist_evals"], engines=np.bincount(ix.filters_info()[0], minlength=3).tolist(), answers_equal=bool(equal), **base)
                ms, spread = timed(ix, loop, a.warm, a.reps)
                emit(route="loop: set_filter_program + search per program", ms=round(ms, 4), spread=round(spread, 3), **base)
    ix.close()


if __name__ == "__main__":
    main()
