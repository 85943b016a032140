"""Filter-only gets (DBServer::Project -> VecSearchExecutor::SearchByAttribute, full-scan branch) through the drop-in DBServer: the host loop
against eps_index_select on the same table, per table size - the measurement behind the adapter's crossover (kSelectMinRows in
dropin/vec_search_executor.cpp; EPS_DROPIN_SELECT_MIN_ROWS picks the side here, it is read on every call).  Filter `ID < n / 2`; the window
lies beyond the last visible row (skip = n), so both sides judge every row and the answer carries no records: the time is the scan's, not the
JSON's.  A second pair (skip = 0, limit = 10) shows the case the host loop leaves after a handful of rows.
Then the library call alone (GpuIndex.select, device outputs, hipEvents around a run of calls) with its HBM bytes per second.
Usage: python scripts/bench_select.py [--sizes 1000,10000,100000,1000000] [--reps 9] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def timed_get(db, reps, **kw):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rc, res = db.get("T", fields=("ID",), **kw)
        ts.append(time.perf_counter() - t0)
        assert rc == 0, res
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, len(res)


def dropin_pair(n, reps):
    from oracle.pyoracle import DROPIN_SO, Ref
    lib = Ref(DROPIN_SO)
    db = lib.db(os.path.join(tempfile.mkdtemp(), "db"), scale=n + 1000, wal=False)
    X = np.random.default_rng(5).random((n, 4), dtype=np.float32)
    schema = {"name": "T", "fields": [{"name": "ID", "dataType": "INT", "primaryKey": True},
                                       {"name": "V", "dataType": "VECTOR_FLOAT", "dimensions": 4, "metricType": "EUCLIDEAN"}]}
    assert db.create_table(schema) == 0
    for s in range(0, n, 20000):
        assert db.insert("T", [{"ID": int(i), "V": X[i].tolist()} for i in range(s, min(n, s + 20000))]) == 0
        if s and s % 200000 == 0:
            print("# %d of %d rows inserted" % (s, n), file=sys.stderr, flush=True)
    flt = "ID < %d" % (n // 2)
    out = {"rows": n, "filter": flt}
    for window, kw in (("beyond", dict(skip=n, limit=10)), ("head", dict(skip=0, limit=10))):
        for side, env in (("device", "0"), ("host", str(1 << 62))):
            os.environ["EPS_DROPIN_SELECT_MIN_ROWS"] = env
            timed_get(db, 2, flt=flt, **kw)   # (warm-up: row and attribute upload, scratch)
            med, best, got = timed_get(db, reps, flt=flt, **kw)
            out["%s_%s_ms" % (window, side)] = round(med, 4)
            out["%s_%s_best_ms" % (window, side)] = round(best, 4)
            out["%s_records" % window] = got
    db.close()
    return out


def library_call(n, reps):
    import torch
    import vectordb_amd as amd
    ix = amd.GpuIndex(4, "EUCLIDEAN", device=0).use_torch_stream()
    ix.attach_rows(np.zeros((n, 4), np.float32))
    ids_col = np.arange(n, dtype=np.int32)
    ix.set_filter_program([("i32", 0), ("const", n // 2), ("<",)], ids_col.reshape(n, 1).view(np.uint8), stride=4)
    out = {"rows": n}
    for name, skip, limit in (("all_ids", 0, n), ("window_10", n // 4, 10)):
        ids = torch.empty(limit, dtype=torch.int64, device="cuda")
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        for _ in range(5):
            ix.select(skip, limit, out=(ids, counts))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ix.select(skip, limit, out=(ids, counts))
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        count, total = (int(x) for x in counts.cpu())
        assert total == n // 2 and count == min(limit, total - skip)
        blocks = (n + 1023) // 1024
        nbytes = 4 * n + 2 * (blocks * 128) + 12 * blocks + 8 * (blocks + 1) + 8 * count   # attribute rows, bitset out and in, counts out and in + offsets out, offsets in, ids
        out[name] = {"ms_per_call": round(ms, 5), "bytes": nbytes, "GB_per_s": round(nbytes / ms / 1e6, 2), "fraction_of_8TBps": round(nbytes / ms / 1e6 / 8000, 5)}
    ix.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in (int(x) for x in a.sizes.split(",")):
        r = dropin_pair(n, a.reps)
        lines.append(json.dumps({"leg": "dropin_get", **r}))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    for n in (int(x) for x in a.sizes.split(",")):
        r = library_call(n, 200)
        lines.append(json.dumps({"leg": "eps_index_select", **r}))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
