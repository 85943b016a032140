"""Host-side mirror of the reference's operator surface for the ANN path, over the C ABI.

  GpuIndex           batch-native handle (one per vector field / shard)
  ANNGraphSegment    same public members and method names as engine/db/ann_graph_segment.hpp:22-55
  VecSearchExecutor  same constructor argument order and result members as
                     engine/db/execution/vec_search_executor.hpp:61-74, 51-52
  GetDistFunc        metric dispatch of engine/db/index/index.cpp:10-35 (returns the metric code the
                     device kernels take; the arithmetic itself lives in csrc/device_common.hpp)

numpy arrays are host buffers; anything exposing `data_ptr()` (a torch tensor on the GPU) is passed as a
device pointer and used in place.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as lib
from ._lib import (EpsillaError, SearchParams, BuildParams, SearchStats, MODE_REFERENCE, MODE_FLAT, MODE_GRAPH,
                   FLAT_AUTO, FLAT_STREAM, FLAT_MFMA, FLAT_MFMA_I8, METRIC_EUCLIDEAN, METRIC_COSINE, METRIC_DOT_PRODUCT, OPS)

METRICS = {"EUCLIDEAN": 0, "COSINE": 1, "DOT_PRODUCT": 2, "L2": 0, "IP": 2, 0: 0, 1: 1, 2: 2}
BruteforceThreshold = 512  # vec_search_executor.hpp:28


def _ptr(a):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _is_dev(a):
    return hasattr(a, "data_ptr")


def GetDistFunc(field_type="VECTOR_FLOAT", metric_type="EUCLIDEAN"):
    """index.cpp:10-35: unknown metrics fall back to L2Sqr."""
    return METRICS.get(metric_type, 0)


class GpuIndex:
    def __init__(self, dim, metric="EUCLIDEAN", device=0, devices=None):
        """devices = [d0, d1, ...]: a hash-sharded index over those GPUs of this process (eps_index_create_sharded; host buffers,
        or device rows per shard / device queries and results on a device of the group); otherwise one index on `device`."""
        self.L = lib.load()
        self.dim = int(dim)
        self.metric = METRICS[metric]
        self.device = device if devices is None else devices[0]
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = self.L.eps_index_create_sharded(self.dim, self.metric, arr, len(devices), C.byref(h))
        else:
            rc = self.L.eps_index_create(self.dim, self.metric, device, C.byref(h))
        if rc != 0:
            raise EpsillaError(rc, "eps_index_create failed (no gfx950 device? there is no CPU fallback)")
        self.h = h
        self._keep = {}

    def _check(self, rc):
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_index_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.eps_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data
    def attach_rows(self, rows):
        if not _is_dev(rows):
            rows = np.ascontiguousarray(rows, np.float32)
        assert rows.shape[1] == self.dim
        self._keep["rows"] = rows
        self._check(self.L.eps_index_attach_rows(self.h, _ptr(rows), rows.shape[0]))

    def attach_shard_rows(self, shard, rows):
        """rows of ONE shard of a sharded index (local row l = global row l * shards + shard): numpy, or a tensor on the shard's own
        device (borrowed).  eps_index_attach_shard_rows."""
        if not _is_dev(rows):
            rows = np.ascontiguousarray(rows, np.float32)
        assert rows.shape[1] == self.dim
        self._keep["rows%d" % shard] = rows
        self._check(self.L.eps_index_attach_shard_rows(self.h, int(shard), _ptr(rows), rows.shape[0]))

    def append_rows(self, rows):
        if not _is_dev(rows):
            rows = np.ascontiguousarray(rows, np.float32)
        self._check(self.L.eps_index_append_rows(self.h, _ptr(rows), rows.shape[0]))

    def clone_rows(self, src, n=None):
        """eps_index_clone_rows: this index takes a device-side copy of the first n rows of `src` (None: all of them) - another index of the same
        kind, dimension and device(s): a plain index from a plain one, a shard group from a group with as many shards.  Later appends to either side
        leave the other unchanged."""
        n = src.row_count if n is None else int(n)
        self._check(self.L.eps_index_clone_rows(self.h, src.h, n))

    def load_table(self, path, primitive_offset, var_len_attrs, dense_dims, field):
        """eps_index_load_table: the reference's data_mvp.bin straight into HBM; returns the record count"""
        dims = (C.c_int64 * len(dense_dims))(*dense_dims)
        lay = lib.TableLayout(primitive_offset, var_len_attrs, len(dense_dims), dims, field, 0)
        n = C.c_int64()
        self._check(self.L.eps_index_load_table(self.h, path.encode(), C.byref(lay), C.byref(n)))
        return n.value

    @property
    def row_count(self):
        return self.L.eps_index_row_count(self.h)

    def set_id_map(self, base, stride):
        self._check(self.L.eps_index_set_id_map(self.h, base, stride))

    def set_deleted(self, bits):
        if bits is None:
            self._check(self.L.eps_index_set_deleted(self.h, None, 0))
            return
        if not _is_dev(bits):
            bits = np.ascontiguousarray(bits, np.uint8)
        self._keep["deleted"] = bits
        nbytes = bits.numel() if _is_dev(bits) else bits.size
        self._check(self.L.eps_index_set_deleted(self.h, _ptr(bits), nbytes))

    def set_int_filter(self, column, op, value, stride=None, width=None, offset=0):
        """column: numpy array / device tensor holding the attribute rows; the value of row i is the signed
        `width`-byte integer at byte `offset + i*stride` (TableSegmentMVP::attribute_table_ layout)."""
        if column is None or not OPS[op]:
            self._check(self.L.eps_index_set_int_filter(self.h, None, 0, 0, 0, 0))
            return
        if not _is_dev(column):
            column = np.ascontiguousarray(column)
            stride = stride or column.strides[0]
            width = width or column.dtype.itemsize
        else:
            stride = stride or column.element_size()
            width = width or column.element_size()
        self._keep["fcol"] = column
        base = C.c_void_p(_ptr(column).value + offset)
        self._check(self.L.eps_index_set_int_filter(self.h, base, stride, width, OPS[op], int(value)))

    def set_filter_program(self, program, rows=None, stride=None, append_only=False):
        """program: postfix list of ("const", x) | ("dist",) | ("i8"|"i16"|"i32"|"i64"|"f32"|"f64"|"bool", byte_offset) |
        (operator,) with operators + - * / % < <= = <> >= > and or not =b <>b (see eps_filter_op); rows: the packed
        attribute rows (numpy structured/2-D uint8 array or device tensor), row i at i*stride bytes.  None / [] clears.
        Host rows are uploaded in full on every call (edit the array in place and call again to refresh);
        append_only=True promises that rows handed over earlier from the same array are unchanged, so only the new tail is
        uploaded (EPS_FILTER_ROWS_APPEND_ONLY)."""
        if not program:
            self._check(self.L.eps_index_set_filter_program(self.h, None, 0, None, 0, 0))
            return
        ops = (lib.FilterOp * len(program))()
        for i, ins in enumerate(program):
            ops[i].op = lib.FOP[ins[0]]
            if ins[0] == "const":
                ops[i].dval = float(ins[1])
            elif len(ins) > 1:
                ops[i].arg = int(ins[1])
        if rows is None:   # the attribute rows eps_index_load_table kept on the device
            self._check(self.L.eps_index_set_filter_program(self.h, ops, len(program), None, 0, 0))
            return
        if not _is_dev(rows):
            rows = np.ascontiguousarray(rows)
            stride = stride or rows.strides[0]
        n_rows = rows.shape[0]
        self._keep["prog_rows"] = rows
        self._check(self.L.eps_index_set_filter_program_ex(self.h, ops, len(program), _ptr(rows), stride, n_rows,
                                                           lib.FILTER_ROWS_APPEND_ONLY if append_only else 0))

    def search_walk(self, queries, limit, cap, **kw):
        """eps_index_search_walk: the <= cap candidates the reference's post-filter loop would walk (host queries)"""
        p = self.params(**kw)
        queries = np.ascontiguousarray(queries, np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.empty((nq, cap), np.int64)
        dist = np.empty((nq, cap), np.float32)
        counts = np.empty(nq, np.int32)
        self._check(self.L.eps_index_search_walk(self.h, _ptr(queries), nq, limit, cap, C.byref(p), _ptr(ids), _ptr(dist), _ptr(counts)))
        return ids, dist, counts

    def set_stream(self, stream_ptr):
        """stream_ptr: a hipStream_t as an integer (torch: `torch.cuda.current_stream().cuda_stream`).  0 is
        torch's default stream = HIP's legacy null stream and is passed as hipStreamLegacy; None gives the index
        its own non-blocking stream again.  Device buffers handed to the index must be ready on ITS stream:
        share the producer's stream (this call) or synchronise the producer first."""
        if stream_ptr is None:
            self._check(self.L.eps_index_set_stream(self.h, None))
        else:
            self._check(self.L.eps_index_set_stream(self.h, C.c_void_p(stream_ptr if stream_ptr else 1)))

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream().cuda_stream)
        return self

    def synchronize(self):
        self._check(self.L.eps_index_synchronize(self.h))

    # ---- graph
    def set_graph(self, off, nbr, nav):
        off = np.ascontiguousarray(off, np.int64)
        nbr = np.ascontiguousarray(nbr, np.int64)
        self._check(self.L.eps_index_set_graph(self.h, len(off) - 1, _ptr(off), _ptr(nbr), int(nav)))

    def graph_info(self):
        n, e, nav = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.L.eps_index_graph_info(self.h, C.byref(n), C.byref(e), C.byref(nav)))
        return n.value, e.value, nav.value

    def get_graph(self):
        n, e, nav = self.graph_info()
        off = np.zeros(n + 1, np.int64)
        nbr = np.zeros(max(e, 1), np.int64)
        self._check(self.L.eps_index_get_graph(self.h, _ptr(off), _ptr(nbr)))
        return off, nbr[:e], nav

    def build(self, n=None, **kw):
        bp = BuildParams()
        self.L.eps_default_build_params(C.byref(bp))
        for k_, v in kw.items():
            setattr(bp, k_, v)
        self._check(self.L.eps_index_build(self.h, self.row_count if n is None else n, C.byref(bp)))

    def knn_graph(self, n=None, **kw):
        """the kNN-graph stage of the build alone (eps_index_knn_graph): ids [n][min(knng, n-1)], closest first, -1 padded"""
        bp = BuildParams()
        self.L.eps_default_build_params(C.byref(bp))
        for k_, v in kw.items():
            setattr(bp, k_, v)
        n = self.row_count if n is None else n
        out = np.empty((n, min(int(bp.knng), n - 1)), np.int64)
        self._check(self.L.eps_index_knn_graph(self.h, n, C.byref(bp), _ptr(out)))
        return out

    def link(self, knn=None, nav=-1, n=None, **kw):
        """the Link stage alone (eps_index_link) on the kNN graph `knn` [n][K] (None: the device's own) from navigation node `nav`
        (-1: the closest row to the centroid); returns (ids [n][out_degree] -1 padded, deg [n], nav)"""
        bp = BuildParams()
        self.L.eps_default_build_params(C.byref(bp))
        for k_, v in kw.items():
            setattr(bp, k_, v)
        n = self.row_count if n is None else n
        if knn is not None:
            knn = np.ascontiguousarray(knn, np.int64)
            assert knn.shape == (n, min(int(bp.knng), n - 1)), knn.shape
        out = np.empty((n, int(bp.out_degree)), np.int64)
        deg = np.empty(n, np.int32)
        nav_out = C.c_int64(-1)
        self._check(self.L.eps_index_link(self.h, n, _ptr(knn), int(nav), C.byref(bp), _ptr(out), _ptr(deg), C.byref(nav_out)))
        return out, deg, int(nav_out.value)

    def mirror_view(self, bits, queries=None):
        """eps_index_mirror_view: what the kernels of the flat matrix engine read, as a dict of numpy arrays - the mirror of width `bits`
        (8 | 16; built or extended as a search would) and `queries` prepared as the staged chain prepares them.  Per-row arrays hold n_pad
        rows.  8-bit: x8 [n_pad][d_pad8] int8, acc0, erow, hrow, mu8, sp8 (rotated frame), scal8, scal8f, q8, qstat, and - when the table
        folds per-row margins - acc0b, qmax; fp16: xh, xn, start, scal, qh, qstat.  Scalars under their own names."""
        q = None if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = 0 if q is None else len(q)
        v = lib.MirrorView()
        self._check(self.L.eps_index_mirror_view(self.h, int(bits), None, 0, C.byref(v)))   # the sizes (no buffer, no query)
        out = {name: getattr(v, name) for name in ("n", "n_pad", "forced_rows", "extended_rows", "d_pad", "usable", "rot", "rot_w", "fold", "step", "slack")}
        out["bits"], out["metric"], out["dim"] = int(bits), self.metric, self.dim
        if not v.usable:
            return out
        n_pad, d_pad = v.n_pad, v.d_pad
        if bits == 8:
            bufs = dict(x=("x8", (n_pad, d_pad), np.int8), acc0=("acc0", (n_pad,), np.int32), erow=("erow", (n_pad,), np.float32),
                        hrow=("hrow", (n_pad,), np.float32), mu=("mu8", (d_pad,), np.float32), scal=("scal8", (8,), np.float32),
                        scalf=("scal8f", (8,), np.float32))
            if v.rot:
                bufs["sp"] = ("sp8", (d_pad,), np.int32)
            if nq:
                bufs.update(q=("q8", (nq, d_pad), np.int8), qstat=("qstat", (nq, 4), np.float32))
                if v.fold:
                    bufs.update(acc0b=("acc0b", (n_pad,), np.int32), qmax=("qmax", (2,), np.uint32))
        else:
            bufs = dict(x=("xh", (n_pad, d_pad), np.float16), xn=("xn", (n_pad,), np.float32), start=("start", (n_pad,), np.float32),
                        scal=("scal", (4,), np.float32))
            if nq:
                bufs.update(q=("qh", (nq, d_pad), np.float16), qstat=("qstat", (nq, 4), np.float32))
        for field, (name, shape, dt) in bufs.items():
            out[name] = np.zeros(shape, dt)
            setattr(v, field, out[name].ctypes.data)
        self._check(self.L.eps_index_mirror_view(self.h, int(bits), _ptr(q), nq, C.byref(v)))
        out["version"] = v.version
        return out

    def filter_pass(self, queries, bits, lo, hi, cap, thr, mode="ids", thr_is_distance=False):
        """eps_index_filter_pass: ONE launch of the filter kernel over rows [lo, hi) with imposed thresholds `thr` [nq] (raw: int32 for
        bits = 8, float32 for 16; or distances, turned into T by the device).  Returns (cnt [nq] rows that passed, lists, T [nq] used):
        lists = per query the min(cnt, cap) row ids (mode "ids"), or (distances, rows) of the approximate keys ("keys", "dense": slot
        = row - lo, every row of the range)."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = len(q)
        m = {"ids": lib.PASS_IDS, "keys": lib.PASS_KEYS, "dense": lib.PASS_DENSE}[mode]
        tdt = np.float32 if (thr_is_distance or bits == 16) else np.int32
        t_in = None if thr is None else np.ascontiguousarray(np.broadcast_to(np.asarray(thr, tdt), (nq,)))
        T = np.zeros(nq, np.int32 if bits == 8 else np.float32)
        cnt = np.zeros(nq, np.uint32)
        cand = np.zeros((nq, int(cap)), np.uint32 if m == lib.PASS_IDS else np.uint64)
        self._check(self.L.eps_index_filter_pass(self.h, _ptr(q), nq, int(bits), int(lo), int(hi), int(cap), m,
                                                 lib.THR_DISTANCE if thr_is_distance else lib.THR_RAW, _ptr(t_in), _ptr(T), _ptr(cnt), _ptr(cand)))
        cnt = cnt.astype(np.int64)
        lists = []
        for j in range(nq):
            c = cand[j, :min(int(cnt[j]), int(cap))]
            if m == lib.PASS_IDS:
                lists.append(c.astype(np.int64))
            else:   # key = order-preserving image of the fp32 distance << 32 | row (device_common.hpp, make_key); ~0 = a NaN key of the dense form
                o = (c >> np.uint64(32)).astype(np.uint32)
                u = np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o)
                lists.append((u.view(np.float32), (c & np.uint64(0xFFFFFFFF)).astype(np.int64)))
        return cnt, lists, T

    def one_pass_probe(self, queries, k):
        """eps_index_one_pass_probe: what the next flat 8-bit search of `queries` with this k would do up to and including the one-pass search's
        pass, and what that pass left behind - a dict: form (the eps_one_pass_form fields), raw_cnt [nq][waves] int64, raw [nq][waves][wave_cap]
        uint64 ((accumulator << 32) | row as stored), table [nq][slots] int32, qstat [nq][4], kth [nq], T_final [nq] int32.  Raises
        EpsillaError 50002 where that search would not take the one-pass form."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = len(q)
        form = lib.OnePassForm()
        room = min(max(nq, 1), 32)   # (more than 32 queries are refused before anything is written)
        raw_cnt = np.empty(room * lib.ONE_PASS_MAX_WAVES, np.uint32)
        raw = np.empty(room * lib.ONE_PASS_MAX_WAVES * lib.ONE_PASS_WAVE_CAP, np.uint64)
        table = np.empty(room * lib.ONE_PASS_MAX_SLOTS, np.int32)
        qstat = np.zeros((nq, 4), np.float32)
        kth, T = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
        self._check(self.L.eps_index_one_pass_probe(self.h, _ptr(q), nq, int(k), C.byref(form), _ptr(raw_cnt), _ptr(raw), _ptr(table), _ptr(qstat), _ptr(kth), _ptr(T)))
        f = {name: int(getattr(form, name)) for name, _ in lib.OnePassForm._fields_}
        W, cap, S = f["waves"], f["wave_cap"], f["slots"]
        return dict(form=f, k=int(k), raw_cnt=raw_cnt[:nq * W].reshape(nq, W).astype(np.int64), raw=raw[:nq * W * cap].reshape(nq, W, cap).copy(),
                    table=table[:nq * S].reshape(nq, S).copy(), qstat=qstat, kth=kth, T_final=T)

    def select_edges(self, nodes, cands, depth=300, out_degree=50):
        """SyncPrune's sort + SelectEdge for given candidate lists (eps_index_select_edges); returns (ids [m][R] -1 padded, deg [m])"""
        nodes = np.ascontiguousarray(nodes, np.int64)
        cands = np.ascontiguousarray(cands, np.int64)
        out = np.empty((len(nodes), out_degree), np.int64)
        deg = np.empty(len(nodes), np.int32)
        self._check(self.L.eps_index_select_edges(self.h, _ptr(nodes), len(nodes), _ptr(cands), cands.shape[1], depth, out_degree, _ptr(out), _ptr(deg)))
        return out, deg

    def inter_insert(self, ids, deg, out_degree):
        """The InterInsert stage on given edge lists ids [n][R] / deg [n] (eps_index_inter_insert); returns (ids [n][R] -1 padded, deg [n])"""
        ids = np.ascontiguousarray(ids, np.int64)
        deg = np.ascontiguousarray(deg, np.int32)
        out = np.empty_like(ids)
        od = np.empty(len(deg), np.int32)
        self._check(self.L.eps_index_inter_insert(self.h, _ptr(ids), _ptr(deg), len(deg), out_degree, _ptr(out), _ptr(od)))
        return out, od

    def save_graph(self, path):
        self._check(self.L.eps_index_save_graph(self.h, path.encode()))

    def load_graph(self, path):
        self._check(self.L.eps_index_load_graph(self.h, path.encode()))

    # ---- search
    def params(self, **kw):
        p = SearchParams()
        self.L.eps_default_search_params(C.byref(p))
        for k_, v in kw.items():
            setattr(p, k_, v)
        return p

    def search(self, queries, k, out=None, **kw):
        """Returns (ids int64[nq,k], dist float32[nq,k], counts int32[nq]); numpy for host queries, or the
        caller-provided device tensors `out=(ids, dist, counts)`."""
        p = self.params(**kw)
        assert out is not None or not _is_dev(queries), "device queries need device output tensors: out=(ids, dist, counts)"
        queries, nq = _queries_2d(queries, self.dim)
        # (caller-provided buffers may be host or device whichever side the queries are on: the C ABI takes either, and refuses a mixed set itself)
        ids, dist, counts = _results("search", (("ids", (nq, k), "int64"), ("dist", (nq, k), "float32"), ("counts", (nq,), "int32")), out, queries,
                                     one_kind=False)
        self._check(self.L.eps_index_search(self.h, _ptr(queries), nq, k, C.byref(p), _ptr(ids), _ptr(dist), _ptr(counts)))
        return ids, dist, counts

    def select(self, skip=0, limit=None, out=None):
        """eps_index_select (SearchByAttribute's full scan, vec_search_executor.cpp:1016-1029): the rows that are not deleted and pass the
        filter installed last, in ascending row order, ranks [skip, skip + limit) of them (limit=None: all rows).  Returns (ids, total):
        the window's ids (row * stride + base) and the number of visible rows in the whole table.  out=(ids int64[limit], counts int64[2]):
        caller-provided buffers, both numpy or both device tensors; counts receives [count, total].  Device buffers are returned as they
        are - (ids, counts), ids[:counts[0]] valid - and the call is asynchronous on the index's stream."""
        skip = int(skip)
        limit = int(self.row_count if limit is None else limit)
        if out is not None:
            ids, counts = out
            _check_select_out(ids, counts, limit)
        else:
            ids = np.empty(max(limit, 0), np.int64)
            counts = np.zeros(2, np.int64)
        total_ptr = C.c_void_p(_ptr(counts).value + 8)
        self._check(self.L.eps_index_select(self.h, skip, limit, _ptr(ids), _ptr(counts), total_ptr))
        if _is_dev(counts):
            return ids, counts
        return ids[:int(counts[0])], int(counts[1])

    def search_range(self, queries, radius, cap, flat_engine="auto", out=None):
        """eps_index_search_range: per query the visible rows whose exact fp32 distance is <= its radius (a scalar, or one per query).  Returns
        (ids int64[nq, cap], dist float32[nq, cap], counts int32[nq], totals int64[nq]): totals = how many such rows there are, counts =
        min(totals, cap), and the counts closest in ascending (distance, id) order, the rest -1 / +inf.  flat_engine: "auto" | "stream" | "mfma" |
        "mfma_i8" (or a FLAT_* value): the same bits from all of them.  NumPy queries give NumPy results; device queries give device tensors and
        the call is asynchronous on the index's stream.  out=(ids, dist, counts, totals): caller-provided buffers, all NumPy or all device."""
        engine = RANGE_ENGINES[flat_engine]
        cap = int(cap)
        queries, nq = _queries_2d(queries, self.dim)
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), (nq,)))
        ids, dist, counts, totals = _results("search_range", _range_spec(nq, cap), out, queries)
        p = self.params(flat_engine=engine)
        self._check(self.L.eps_index_search_range(self.h, _ptr(queries), nq, _ptr(radius), cap, C.byref(p), _ptr(ids), _ptr(dist), _ptr(counts),
                                                  _ptr(totals)))
        return ids, dist, counts, totals

    def search_among(self, queries, ids, k, offsets=None, out=None):
        """eps_index_search_among: per query the k closest VISIBLE rows among the ids the caller names (global ids, eps_index_set_id_map; an id
        that names no row is ignored, a row named several times counts once).  ids: int64, NumPy or a device tensor - offsets None: ONE list for
        every query; else any integer sequence of nq + 1 non-decreasing positions, offsets[0] = 0, offsets[nq] = len(ids): query j's list is
        ids[offsets[j]:offsets[j + 1]].  Returns (ids int64[nq, k], dist float32[nq, k], counts int32[nq]) in ascending (distance, id) order, the
        rest -1 / +inf; the distances are a flat search's, bit for bit.  NumPy queries give NumPy results; device queries give device tensors
        and the call is asynchronous on the index's stream.  out=(ids, dist, counts): caller-provided buffers, all NumPy or all device."""
        k = int(k)
        queries, nq = _queries_2d(queries, self.dim)
        if _is_dev(ids):
            if str(ids.dtype) != "torch.int64" or ids.dim() != 1 or not ids.is_contiguous():
                raise ValueError("search_among: device ids must be a contiguous 1-D int64 tensor, got %s %s" % (ids.dtype, tuple(ids.shape)))
            n_cand = ids.numel()
        else:
            ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
            n_cand = ids.size
        if offsets is not None:
            offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if _is_dev(offsets) else offsets), np.int64).reshape(-1)
            if offsets.size != nq + 1:
                raise ValueError("search_among: offsets must hold nq + 1 = %d entries, got %d" % (nq + 1, offsets.size))
        out_ids, dist, counts = _results("search_among", (("ids", (nq, k), "int64"), ("dist", (nq, k), "float32"), ("counts", (nq,), "int32")), out, queries)
        self._keep["among"] = (queries, ids, offsets)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_index_search_among(self.h, _ptr(queries), nq, _ptr(ids) if n_cand else None, _ptr(offsets), n_cand, k, _ptr(out_ids),
                                                  _ptr(dist), _ptr(counts)))
        return out_ids, dist, counts

    def search_diverse(self, queries, k, fetch_k, lam=0.5, ids=None, offsets=None, flat_engine="auto", out=None):
        """eps_index_search_diverse: per query k rows of its pool by greedy maximal marginal relevance - step 1 takes the closest row, every later
        step the unselected row with the smallest lam * d(row, query) - (1 - lam) * min over the selected rows s of D(row, s), ties to the earlier pool
        position.  The pool is search(k=fetch_k)'s answer (flat mode, flat_engine as for search_range: the same bits from all of them) or, with ids
        given, search_among(ids, fetch_k, offsets)'s - ids and offsets as search_among takes them.  Returns (ids int64[nq, k], dist float32[nq, k],
        score float32[nq, k], counts int32[nq]) in SELECTION order, counts = min(k, pool size), the rest -1 / +inf / +inf; dist are a flat search's
        bits, lam = 1 returns the pool's first k.  1 <= k <= fetch_k <= 1024; the selection reads (k - 1) x pool x dim x 4 bytes per query: quadratic
        when k follows fetch_k.  NumPy queries give NumPy results; device queries give device tensors and the call is asynchronous on the index's
        stream.  out=(ids, dist, score, counts): caller-provided buffers, all NumPy or all device."""
        k, fetch_k = int(k), int(fetch_k)
        queries, nq = _queries_2d(queries, self.dim)
        n_cand = 0
        if ids is None:
            if offsets is not None:
                raise ValueError("search_diverse: offsets without ids")
        elif _is_dev(ids):
            if str(ids.dtype) != "torch.int64" or ids.dim() != 1 or not ids.is_contiguous():
                raise ValueError("search_diverse: device ids must be a contiguous 1-D int64 tensor, got %s %s" % (ids.dtype, tuple(ids.shape)))
            n_cand = ids.numel()
        else:
            ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
            n_cand = ids.size
        if ids is not None and n_cand == 0:
            ids = np.zeros(1, np.int64)   # (an empty list is still a list: a non-null pointer that is never read)
        if offsets is not None:
            offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if _is_dev(offsets) else offsets), np.int64).reshape(-1)
            if offsets.size != nq + 1:
                raise ValueError("search_diverse: offsets must hold nq + 1 = %d entries, got %d" % (nq + 1, offsets.size))
        out_ids, dist, score, counts = _results("search_diverse", (("ids", (nq, k), "int64"), ("dist", (nq, k), "float32"), ("score", (nq, k), "float32"),
                                                                   ("counts", (nq,), "int32")), out, queries)
        p = self.params(flat_engine=RANGE_ENGINES[flat_engine])
        self._keep["diverse"] = (queries, ids, offsets)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_index_search_diverse(self.h, _ptr(queries), nq, k, fetch_k, float(lam), _ptr(ids), _ptr(offsets), n_cand, C.byref(p),
                                                    _ptr(out_ids), _ptr(dist), _ptr(score), _ptr(counts)))
        return out_ids, dist, score, counts

    def set_groups(self, keys):
        """eps_index_set_groups: one int64 key per row (NumPy, or a contiguous 1-D int64 device tensor); rows with equal keys form a group.  None
        forgets the groups.  After attach_rows / append_rows the keys must be set again."""
        if keys is None:
            self._check(self.L.eps_index_set_groups(self.h, None, 0))
            return
        if _is_dev(keys):
            if str(keys.dtype) != "torch.int64" or keys.dim() != 1 or not keys.is_contiguous():
                raise ValueError("set_groups: device keys must be a contiguous 1-D int64 tensor, got %s %s" % (keys.dtype, tuple(keys.shape)))
            n = keys.numel()
        else:
            keys = np.ascontiguousarray(keys, np.int64).reshape(-1)
            n = keys.size
        self._check(self.L.eps_index_set_groups(self.h, _ptr(keys), n))   # (the library copies the keys before it returns)

    def search_groups(self, queries, k, engine="auto", page_rows=0, scratch_bytes=0, flat_engine="auto", out=None):
        """eps_index_search_groups: per query the k closest GROUPS (set_groups), each represented by its closest visible row.  Returns
        (ids int64[nq, k], dist float32[nq, k], group_keys int64[nq, k], counts int32[nq]) in ascending (distance, id) order of the
        representatives; counts = min(k, groups with a visible row), the rest -1 / +inf / key 0.  The distances are a flat search's, bit for bit.
        engine: "auto" | "pages" | "scan" (or a GROUPS_* value), flat_engine as for search_range: the same bits from all of them.  page_rows: keys per
        page (0: the library's rule of k); scratch_bytes: a cap on the scan engine's table (0: the default).  NumPy queries give NumPy results; device
        queries give device tensors and the call is asynchronous on the index's stream.  out=(ids, dist, group_keys, counts): caller-provided
        buffers, all NumPy or all device."""
        k = int(k)
        engine, flat_engine = GROUPS_ENGINES[engine], RANGE_ENGINES[flat_engine]
        queries, nq = _queries_2d(queries, self.dim)
        ids, dist, gkeys, counts = _results("search_groups", (("ids", (nq, k), "int64"), ("dist", (nq, k), "float32"), ("group_keys", (nq, k), "int64"),
                                                              ("counts", (nq,), "int32")), out, queries)
        p = self.params(flat_engine=flat_engine)
        self._keep["groups"] = (queries,)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_index_search_groups(self.h, _ptr(queries), nq, k, C.byref(p), engine, int(page_rows), int(scratch_bytes),
                                                   _ptr(ids), _ptr(dist), _ptr(gkeys), _ptr(counts)))
        return ids, dist, gkeys, counts

    def search_group_rows(self, queries, k, m, engine="auto", page_rows=0, scratch_bytes=0, flat_engine="auto", out=None):
        """eps_index_search_group_rows: per query the k closest GROUPS as search_groups returns them, and of each its m closest visible rows.  Returns
        (ids int64[nq, k, m], dist float32[nq, k, m], group_keys int64[nq, k], row_counts int32[nq, k], group_sizes int64[nq, k], counts int32[nq]):
        the rows of a group in ascending (distance, id) order, slot 0 the representative of search_groups; row_counts = min(m, visible rows of the
        group), group_sizes = its visible rows for this query, counts = min(k, groups with a visible row); unused row slots -1 / +inf, unused group
        slots key 0, row count 0, size 0.  engine, page_rows, scratch_bytes, flat_engine: as for search_groups.  NumPy queries give NumPy results;
        device queries give device tensors and the call is asynchronous on the index's stream.  out=(ids, dist, group_keys, row_counts, group_sizes,
        counts): caller-provided buffers, all NumPy or all device."""
        k, m = int(k), int(m)
        engine, flat_engine = GROUPS_ENGINES[engine], RANGE_ENGINES[flat_engine]
        queries, nq = _queries_2d(queries, self.dim)
        ids, dist, gkeys, rcounts, gsizes, counts = _results("search_group_rows", (
            ("ids", (nq, k, m), "int64"), ("dist", (nq, k, m), "float32"), ("group_keys", (nq, k), "int64"), ("row_counts", (nq, k), "int32"),
            ("group_sizes", (nq, k), "int64"), ("counts", (nq,), "int32")), out, queries)
        p = self.params(flat_engine=flat_engine)
        self._keep["group_rows"] = (queries,)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_index_search_group_rows(self.h, _ptr(queries), nq, k, m, C.byref(p), engine, int(page_rows), int(scratch_bytes),
                                                       _ptr(ids), _ptr(dist), _ptr(gkeys), _ptr(rcounts), _ptr(gsizes), _ptr(counts)))
        return ids, dist, gkeys, rcounts, gsizes, counts

    def search_multi(self, bags, k, cand_keys=None, cand_offsets=None, scratch_bytes=0, out=None):
        """eps_index_search_multi: every query is a BAG of vectors; a group (set_groups) scores by the sum, over the bag's vectors in order, of the
        distance to its closest visible row, and the k groups with the smallest sums are returned.  bags: a sequence of 2-D arrays, or a pair
        (vectors [T, dim] - NumPy or a device tensor -, offsets: nq + 1 non-decreasing positions, offsets[0] = 0).  cand_keys None: every group is
        considered; else only the groups whose int64 keys are named (NumPy or a device tensor) - one list for every bag, or with cand_offsets
        (nq + 1 positions) bag j's list cand_keys[cand_offsets[j]:cand_offsets[j + 1]]; unknown keys are ignored, repeated ones count once.
        Returns (group_keys int64[nq, k], score float32[nq, k], counts int32[nq], match_ids int64[k * T], match_dist float32[k * T]): ascending
        (score, group key), counts = min(k, groups with a visible row for EVERY vector of the bag), the rest key 0 / +inf; the matches - the row
        each vector met in each returned group, -1 / +inf where unused - are flat: multi_matches(match_ids, offsets, k, j) is bag j's [k, t_j] view.
        scratch_bytes: a cap on the tables of one pass (0: the default).  NumPy vectors give NumPy results; device vectors give device tensors and
        the call is asynchronous on the index's stream.  out=(group_keys, score, counts, match_ids, match_dist): caller-provided buffers, all NumPy
        or all device."""
        k = int(k)
        vectors, offsets = _bags(bags, self.dim)
        nq, T = offsets.size - 1, int(offsets[-1])
        n_cand = 0
        if cand_keys is not None:
            if _is_dev(cand_keys):
                if str(cand_keys.dtype) != "torch.int64" or cand_keys.dim() != 1 or not cand_keys.is_contiguous():
                    raise ValueError("search_multi: device cand_keys must be a contiguous 1-D int64 tensor, got %s %s" % (cand_keys.dtype, tuple(cand_keys.shape)))
                n_cand = cand_keys.numel()
            else:
                cand_keys = np.ascontiguousarray(cand_keys, np.int64).reshape(-1)
                n_cand = cand_keys.size
                if n_cand == 0:
                    cand_keys = np.zeros(1, np.int64)   # (an empty list is still a list: the pointer says which form is meant)
        if cand_offsets is not None:
            if cand_keys is None:
                raise ValueError("search_multi: cand_offsets without cand_keys")
            cand_offsets = np.ascontiguousarray(np.asarray(cand_offsets.cpu() if _is_dev(cand_offsets) else cand_offsets), np.int64).reshape(-1)
            if cand_offsets.size != nq + 1:
                raise ValueError("search_multi: cand_offsets must hold nq + 1 = %d entries, got %d" % (nq + 1, cand_offsets.size))
        gkeys, score, counts, mids, mdist = _results("search_multi", (("group_keys", (nq, k), "int64"), ("score", (nq, k), "float32"), ("counts", (nq,), "int32"),
                                                                     ("match_ids", (k * T,), "int64"), ("match_dist", (k * T,), "float32")), out, vectors)
        self._keep["multi"] = (vectors, offsets, cand_keys, cand_offsets)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_index_search_multi(self.h, _ptr(vectors) if T else None, _ptr(offsets), nq, _ptr(cand_keys), _ptr(cand_offsets), n_cand, k,
                                                  int(scratch_bytes), _ptr(gkeys), _ptr(score), _ptr(counts), _ptr(mids), _ptr(mdist)))
        return gkeys, score, counts, mids, mdist

    def groups_info(self):
        """eps_index_groups_info: {"n_groups", "largest_group", "last_engines": the engines the last search_groups ran, as names, "last_scan_queries"}"""
        g, big, scanned, engines = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._check(self.L.eps_index_groups_info(self.h, C.byref(g), C.byref(big), C.byref(engines), C.byref(scanned)))
        return {"n_groups": g.value, "largest_group": big.value, "last_scan_queries": scanned.value,
                "last_engines": tuple(name for name, bit in (("pages", GROUPS_PAGES), ("scan", GROUPS_SCAN)) if engines.value >> bit & 1)}

    def kernel_times(self, cap=64):
        """main-kernel ms of the most recent search calls (oldest first); synchronises the index's stream"""
        buf = (C.c_double * cap)()
        n = self.L.eps_index_kernel_times(self.h, buf, cap)
        return [buf[i] for i in range(n)]

    def stats(self):
        s = SearchStats()
        self._check(self.L.eps_index_last_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in SearchStats._fields_}


def _queries_2d(queries, dim):
    """(queries, nq) as the C ABI reads them: a device tensor as it is, anything else as C-contiguous float32 - one query per row, a single vector as one row"""
    if not _is_dev(queries):
        queries = np.ascontiguousarray(queries, np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
    assert queries.shape[1] == dim
    return queries, queries.shape[0]


def _bags(bags, dim):
    """(vectors [T, dim], offsets int64[nq + 1]) as eps_index_search_multi reads them, from a pair (vectors, offsets) or a sequence of 2-D arrays"""
    if isinstance(bags, tuple) and len(bags) == 2 and (_is_dev(bags[0]) or np.ndim(bags[1]) == 1 and np.ndim(bags[0]) == 2):
        vectors, offsets = bags
        offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if _is_dev(offsets) else offsets), np.int64).reshape(-1)
        if not _is_dev(vectors):
            vectors = np.ascontiguousarray(vectors, np.float32).reshape(-1, dim)
    else:
        parts = [np.ascontiguousarray(b, np.float32).reshape(-1, dim) for b in bags]
        offsets = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([p.shape[0] for p in parts], out=offsets[1:])
        vectors = np.concatenate(parts) if parts else np.zeros((0, dim), np.float32)
    if offsets.size < 1 or offsets[0] != 0 or np.any(np.diff(offsets) < 0):
        raise ValueError("search_multi: offsets must start at 0 and not decrease")
    if tuple(vectors.shape) != (int(offsets[-1]), dim) or (_is_dev(vectors) and (str(vectors.dtype) != "torch.float32" or not vectors.is_contiguous())):
        raise ValueError("search_multi: vectors must be a C-contiguous float32 array of shape (%d, %d), got %s" % (int(offsets[-1]), dim, tuple(vectors.shape)))
    return vectors, offsets


def multi_matches(flat, offsets, k, j):
    """bag j's [k, t_j] view of search_multi's flat match_ids / match_dist (slot s, vector u of the bag at k * offsets[j] + s * t_j + u)"""
    lo, t = int(offsets[j]), int(offsets[j + 1]) - int(offsets[j])
    return flat[k * lo:k * (lo + t)].reshape(k, t)


def _check_bufs(who, bufs, one_kind=True, label="%s"):
    """the one check of arrays the C ABI reads or writes through raw pointers.  bufs: (array, name, shape, dtype) - each C-contiguous, of that dtype
    and shape, and (one_kind) all of them NumPy arrays or all device tensors; or a ValueError that names the call and the array (as label % name)
    instead of an out-of-bounds access"""
    if one_kind and len({_is_dev(a) for a, _, _, _ in bufs}) != 1:
        names = [label % name for _, name, _, _ in bufs]
        each = "both" if len(bufs) == 2 else "all"
        raise ValueError("%s: %s and %s must %s be NumPy arrays or %s be device tensors" % (who, ", ".join(names[:-1]), names[-1], each, each))
    for a, name, shape, dtype in bufs:
        got_dtype = str(a.dtype).replace("torch.", "")
        contiguous = a.is_contiguous() if hasattr(a, "is_contiguous") else bool(a.flags["C_CONTIGUOUS"])
        if got_dtype != dtype or tuple(a.shape) != tuple(shape) or not contiguous:
            raise ValueError("%s: %s must be a C-contiguous %s array of shape %s, got %s %s%s"
                             % (who, label % name, dtype, tuple(shape), got_dtype, tuple(a.shape), "" if contiguous else " (not contiguous)"))


def _results(who, spec, out, like, one_kind=True):
    """a call's result arrays from its spec - (name, shape, dtype) per result.  out given: the caller's buffers, checked against the spec (_check_bufs);
    else new ones of the kind `like` is - NumPy arrays, or tensors on like's device"""
    if out is None:
        return tuple(_empty_like_kind(like, tuple(max(int(v), 0) for v in shape), dtype) for _, shape, dtype in spec)
    out = tuple(out)
    if len(out) != len(spec):
        raise ValueError("%s: out must hold %d buffers (%s), got %d" % (who, len(spec), ", ".join(name for name, _, _ in spec), len(out)))
    _check_bufs(who, tuple((a,) + tuple(s) for a, s in zip(out, spec)), one_kind, "out[%s]")
    return out


def _check_out(a, name, shape, dtype, who="search"):
    """one caller-provided result buffer of the call `who`"""
    _check_bufs(who, ((a, name, shape, dtype),), one_kind=False, label="out[%s]")


RANGE_ENGINES = {"auto": FLAT_AUTO, "stream": FLAT_STREAM, "mfma": FLAT_MFMA, "mfma_i8": FLAT_MFMA_I8,
                 FLAT_AUTO: FLAT_AUTO, FLAT_STREAM: FLAT_STREAM, FLAT_MFMA: FLAT_MFMA, FLAT_MFMA_I8: FLAT_MFMA_I8}


GROUPS_AUTO, GROUPS_PAGES, GROUPS_SCAN = 0, 1, 2
GROUPS_ENGINES = {"auto": GROUPS_AUTO, "pages": GROUPS_PAGES, "scan": GROUPS_SCAN, GROUPS_AUTO: GROUPS_AUTO, GROUPS_PAGES: GROUPS_PAGES, GROUPS_SCAN: GROUPS_SCAN}


def _range_spec(nq, cap):
    return (("ids", (nq, cap), "int64"), ("dist", (nq, cap), "float32"), ("counts", (nq,), "int32"), ("totals", (nq,), "int64"))


def _check_range_out(ids, dist, counts, totals, nq, cap):
    """search_range's caller-provided buffers (and the range merges'): ids int64 [nq, cap], dist float32 [nq, cap], counts int32 [nq], totals int64 [nq]"""
    _results("search_range", _range_spec(nq, cap), (ids, dist, counts, totals), None)


def _check_select_out(ids, counts, limit):
    """select's caller-provided buffers (and merge_select's): ids int64 [limit] and counts int64 [2]"""
    _results("select", (("ids", (limit,), "int64"), ("counts", (2,), "int64")), (ids, counts), None)


def traversal_gather_bytes(stats, dim, avg_degree, seed_evals=0):
    """Algorithmic bytes the traversal kernel gathers for the search `stats` describes: adjacency lists X*(8 + 4*deg); rows
    E*(4d + 4) when every evaluation reads its fp32 row; with the 8-bit prefilter (stats["rerank_rows"] > 0: fp32 rows read in
    step d) the seed evaluations and the survivors read 4d bytes, every neighbour evaluation its mirror row (d rounded up to 16
    bytes) + the 4-byte row constant.  seed_evals: SearchQueueSize x queries (seeds are always evaluated in fp32)."""
    e, x, f = float(stats["dist_evals"]), float(stats["expansions"]), float(stats["rerank_rows"])
    adj = x * (8 + 4.0 * avg_degree)
    if f <= 0:
        return e * (4.0 * dim + 4) + adj
    q8 = (dim + 15) // 16 * 16
    return (seed_evals + f) * 4.0 * dim + (e - seed_evals) * (q8 + 4.0) + e * 4 + adj


def merge_topk_packed(gathered, shard_stride_bytes, dist_offset_bytes, shards, nq, k, out_dist, out_ids, device=0, stream=None):
    """gathered: one device buffer = the all-gather of every rank's packed [ids int64[nq][k] | dist float[nq][k]]."""
    L = lib.load()
    rc = L.eps_merge_topk_packed(_ptr(gathered), shard_stride_bytes, dist_offset_bytes, shards, nq, k, _ptr(out_dist), _ptr(out_ids),
                                 device, C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise EpsillaError(rc, "eps_merge_topk_packed failed")
    return out_dist, out_ids


class Exchange:
    """eps_exchange (include/epsilla_gfx950.h): the sharded path's one exchange step - an RCCL all-gather of every rank's packed top-k lists and
    the k-way merge - on a communicator the library owns.  Bootstrap: rank 0 calls Exchange.unique_id(), the 128 bytes reach every rank by the
    caller's means, every rank constructs Exchange(rank, world, id_bytes, device) (collective)."""

    @staticmethod
    def unique_id():
        L = lib.load()
        buf = C.create_string_buffer(128)
        rc = L.eps_exchange_unique_id(buf)
        if rc != 0:
            raise EpsillaError(rc, "eps_exchange_unique_id failed (RCCL not loadable?)")
        return buf.raw

    def __init__(self, rank, world, id_bytes, device=0):
        self.L = lib.load()
        assert len(id_bytes) == 128
        self.h = C.c_void_p()
        self.device = device
        rc = self.L.eps_exchange_create(rank, world, C.c_char_p(bytes(id_bytes)), device, C.byref(self.h))
        if rc != 0:
            msg = self.L.eps_exchange_last_error(self.h).decode() if self.h else "eps_exchange_create failed"
            if self.h:
                self.L.eps_exchange_destroy(self.h)
                self.h = None
            raise EpsillaError(rc, msg)

    @classmethod
    def direct(cls, rank, world, device=0):
        """an exchange WITHOUT a communicator: the b = 1 form only (mailbox_export / mailbox_connect / direct_merge); ranks may share a device"""
        self = cls.__new__(cls)
        self.L = lib.load()
        self.h = C.c_void_p()
        self.device = device
        self.world = world
        rc = self.L.eps_exchange_create_direct(rank, world, device, C.byref(self.h))
        if rc != 0:
            msg = self.L.eps_exchange_last_error(self.h).decode() if self.h else "eps_exchange_create_direct failed"
            if self.h:
                self.L.eps_exchange_destroy(self.h)
                self.h = None
            raise EpsillaError(rc, msg)
        return self

    def mailbox_export(self):
        """64 bytes: this rank's mailbox for its peers (hipIpc handle); gather all ranks' handles by your own means and pass them to mailbox_connect"""
        buf = C.create_string_buffer(64)
        rc = self.L.eps_exchange_mailbox_export(self.h, buf)
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_exchange_last_error(self.h).decode())
        return buf.raw

    def mailbox_connect(self, handles):
        """handles: every rank's 64 bytes, in rank order"""
        blob = b"".join(bytes(h) for h in handles)
        assert len(blob) == 64 * len(handles)
        rc = self.L.eps_exchange_mailbox_connect(self.h, C.c_char_p(blob))
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_exchange_last_error(self.h).decode())

    def direct_merge(self, ids, dist, out_ids, out_dist, stream=None):
        """the exchange step without a collective (<= 16 KB of lists per rank): peer stores + flag, device-side wait, merge"""
        nq, k = ids.shape
        rc = self.L.eps_exchange_direct_merge(self.h, _ptr(ids), _ptr(dist), nq, k, _ptr(out_ids), _ptr(out_dist), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_exchange_last_error(self.h).decode())
        return out_ids, out_dist

    def allgather_merge(self, ids, dist, out_ids, out_dist, stream=None):
        """ids int64 [nq][k], dist float32 [nq][k] (this rank's lists, device tensors) -> out_ids / out_dist: the merged global top-k, on every rank"""
        nq, k = ids.shape
        rc = self.L.eps_exchange_allgather_merge(self.h, _ptr(ids), _ptr(dist), nq, k, _ptr(out_ids), _ptr(out_dist), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_exchange_last_error(self.h).decode())
        return out_ids, out_dist

    def allgather_merge_range(self, ids, dist, counts, totals, out=None, stream=None):
        """this rank's answer of GpuIndex.search_range over its shard (device tensors: ids int64 / dist float32 [nq, cap], counts int32 [nq], totals
        int64 [nq]) -> (ids, dist, counts, totals) of the unsharded table, on every rank; out=: caller-provided device tensors of those shapes"""
        nq, cap = (int(v) for v in ids.shape)
        _check_range_out(ids, dist, counts, totals, nq, cap)
        if out is None:
            import torch
            out = (torch.empty_like(ids), torch.empty_like(dist), torch.empty_like(counts), torch.empty_like(totals))
        _check_range_out(*out, nq, cap)
        rc = self.L.eps_exchange_allgather_merge_range(self.h, _ptr(ids), _ptr(dist), _ptr(counts), _ptr(totals), nq, cap, _ptr(out[0]), _ptr(out[1]),
                                                       _ptr(out[2]), _ptr(out[3]), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_exchange_last_error(self.h).decode())
        return tuple(out)

    def times_us(self, max_calls=64):
        """[(all-gather us, merge us)] of the last calls, oldest first (waits for them)"""
        buf = (C.c_double * (2 * max_calls))()
        got = self.L.eps_exchange_times(self.h, buf, max_calls)
        if got < 0:
            raise EpsillaError(-1, "eps_exchange_times failed")
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(got)]

    def info(self):
        r, w, v = C.c_int32(), C.c_int32(), C.c_int32()
        path = C.create_string_buffer(512)
        self.L.eps_exchange_info(self.h, C.byref(r), C.byref(w), C.byref(v), path, 512)
        return {"rank": r.value, "world": w.value, "rccl_version": v.value, "rccl_library": path.value.decode()}

    def close(self):
        if self.h:
            self.L.eps_exchange_destroy(self.h)
            self.h = None


def normalize_rows(rows, only_if_nonzero=True, device=0, stream=None):
    """Normalize (db/vector.cpp:60-69) / insert-time normalisation (table_segment_mvp.cpp:574-587), in place."""
    L = lib.load()
    n, d = rows.shape
    rc = L.eps_normalize_rows(_ptr(rows), n, d, int(only_if_nonzero), device, C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise EpsillaError(rc, "eps_normalize_rows failed")
    return rows


def merge_topk(dist, ids, out_dist, out_ids, device=0, stream=None):
    """dist/ids: [shards, nq, k] (all device tensors or all numpy)."""
    L = lib.load()
    shards, nq, k = dist.shape
    rc = L.eps_merge_topk(_ptr(dist), _ptr(ids), shards, nq, k, _ptr(out_dist), _ptr(out_ids), device,
                          C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise EpsillaError(rc, "eps_merge_topk failed")
    return out_dist, out_ids


# ---- radius search and ordered select across shards (eps_merge_range, eps_merge_range_packed, eps_merge_select; csrc/merge_lists.hip)
MERGE_MAX_SHARDS, MERGE_MAX_CAP = 16, 8192


def _empty_like_kind(like, shape, dtype):
    """a result buffer of the kind `like` is: a NumPy array, or a tensor on like's device"""
    if _is_dev(like):
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)
    return np.empty(shape, dtype)


def _merge_refusal(shards, cap=1, nq=0, length=0, skip=0, limit=0):
    """why the library refused a merge (it has no handle to leave a message in)"""
    why = []
    if not 1 <= shards <= MERGE_MAX_SHARDS:
        why.append("shards = %d, must be in 1 .. %d" % (shards, MERGE_MAX_SHARDS))
    if not 1 <= cap <= MERGE_MAX_CAP:
        why.append("cap = %d, must be in 1 .. %d" % (cap, MERGE_MAX_CAP))
    if nq < 0 or length < 0 or skip < 0 or limit < 0:
        why.append("negative nq, len, skip or limit")
    elif length < skip + limit:
        why.append("len = %d < skip + limit = %d: a shard's list must reach as far as the window" % (length, skip + limit))
    return "; ".join(why) or "refused (a null or mixed host / device buffer?)"


def range_pack_bytes(nq, cap):
    """eps_range_pack_bytes: one shard's packed radius answer, ids i64[nq][cap] | totals i64[nq] | dist f32[nq][cap] | counts i32[nq], rounded up to 8"""
    return int(lib.load().eps_range_pack_bytes(nq, cap))


def merge_range(ids, dist, counts, totals, out=None, device=0, stream=None):
    """eps_merge_range: ids int64 / dist float32 [shards, nq, cap], counts int32 [shards, nq], totals int64 [shards, nq] - every shard's answer of
    search_range to the same queries, global ids - all NumPy or all device tensors.  Returns (ids [nq, cap], dist [nq, cap], counts [nq], totals [nq])
    of the unsharded table, of the same kind (out=: caller-provided buffers of that kind).  Device tensors: asynchronous on `stream`."""
    L = lib.load()
    if len(ids.shape) != 3:
        raise ValueError("merge_range: ids must have shape [shards, nq, cap], got %s" % (tuple(ids.shape),))
    shards, nq, cap = (int(v) for v in ids.shape)
    _check_bufs("merge_range", ((ids, "ids", (shards, nq, cap), "int64"), (dist, "dist", (shards, nq, cap), "float32"),
                                (counts, "counts", (shards, nq), "int32"), (totals, "totals", (shards, nq), "int64")))
    if out is None:
        out = _results("merge_range", _range_spec(nq, cap), None, ids)
    _check_range_out(*out, nq, cap)
    if _is_dev(out[0]) != _is_dev(ids):
        raise ValueError("merge_range: lists and out= must all be NumPy arrays or all be device tensors")
    rc = L.eps_merge_range(_ptr(ids), _ptr(dist), _ptr(counts), _ptr(totals), shards, nq, cap, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
                           device, C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise EpsillaError(rc, "eps_merge_range: " + _merge_refusal(shards, cap, nq))
    return tuple(out)


def merge_range_packed(gathered, shard_stride_bytes, shards, nq, cap, out=None, device=0, stream=None):
    """eps_merge_range_packed: gathered = one device buffer in which shard s's packed answer (range_pack_bytes) starts at s * shard_stride_bytes"""
    L = lib.load()
    shards, nq, cap = int(shards), int(nq), int(cap)
    if not _is_dev(gathered):
        raise ValueError("merge_range_packed: gathered must be a device tensor")
    if 1 <= shards <= MERGE_MAX_SHARDS and gathered.numel() * gathered.element_size() < shards * int(shard_stride_bytes):
        raise ValueError("merge_range_packed: gathered holds %d bytes, %d shards of %d bytes are needed"
                         % (gathered.numel() * gathered.element_size(), shards, shard_stride_bytes))
    if out is None:
        out = _results("merge_range_packed", _range_spec(nq, cap), None, gathered)
    _check_range_out(*out, nq, cap)
    rc = L.eps_merge_range_packed(_ptr(gathered), int(shard_stride_bytes), shards, nq, cap, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
                                  device, C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise EpsillaError(rc, "eps_merge_range_packed: " + (_merge_refusal(shards, cap, nq) if not (1 <= shards <= MERGE_MAX_SHARDS and 1 <= cap <= MERGE_MAX_CAP)
                                                             else "shard_stride_bytes must be a multiple of 8 and at least range_pack_bytes; device buffers only"))
    return tuple(out)


def merge_select(ids, counts, totals, skip=0, limit=None, out=None, device=0, stream=None):
    """eps_merge_select: ids int64 [shards, len], counts int64 [shards], totals int64 [shards] - every shard's answer of select(0, len), global ids -
    all NumPy or all device tensors.  Ranks [skip, skip + limit) of the merged ascending ids (limit=None: len - skip) and the total, as
    GpuIndex.select returns them: NumPy -> (ids of the window, total); device -> (ids [limit], counts [2] = count, total), asynchronous on `stream`.
    out=(ids int64 [limit], counts int64 [2]) of the lists' kind."""
    L = lib.load()
    if len(ids.shape) != 2:
        raise ValueError("merge_select: ids must have shape [shards, len], got %s" % (tuple(ids.shape),))
    shards, length = (int(v) for v in ids.shape)
    skip = int(skip)
    limit = max(length - skip, 0) if limit is None else int(limit)
    _check_bufs("merge_select", ((ids, "ids", (shards, length), "int64"), (counts, "counts", (shards,), "int64"), (totals, "totals", (shards,), "int64")))
    if out is None:
        out = (_empty_like_kind(ids, (max(limit, 0),), "int64"), _empty_like_kind(ids, (2,), "int64"))
    out_ids, out_counts = out
    _check_select_out(out_ids, out_counts, max(limit, 0))
    if _is_dev(out_ids) != _is_dev(ids):
        raise ValueError("merge_select: lists and out= must all be NumPy arrays or all be device tensors")
    total_ptr = C.c_void_p(_ptr(out_counts).value + 8)
    rc = L.eps_merge_select(_ptr(ids), _ptr(counts), _ptr(totals), shards, length, skip, limit, _ptr(out_ids), _ptr(out_counts), total_ptr, device,
                            C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise EpsillaError(rc, "eps_merge_select: " + _merge_refusal(shards, 1, 0, length, skip, limit))
    if _is_dev(out_counts):
        return out_ids, out_counts
    return out_ids[:int(out_counts[0])], int(out_counts[1])


def _check_shards(what, shards):
    shards = list(shards)
    if not 1 <= len(shards) <= MERGE_MAX_SHARDS:
        raise EpsillaError(lib.EPS_USER_ERROR, "%s: %d shards, must be 1 .. %d" % (what, len(shards), MERGE_MAX_SHARDS))
    return shards


def search_range_shards(shards, queries, radius, cap, flat_engine="auto"):
    """GpuIndex.search_range of a table held by G single-device indices, shard s holding the rows i with i mod G = s and set_id_map(s, G): every
    shard answers the whole batch over its rows, merge_range joins the answers.  Returns what GpuIndex.search_range returns for the whole table, bit
    for bit: NumPy queries give NumPy arrays; device queries give tensors on the queries' device (the shards' calls are waited for, the merge is
    asynchronous on the null stream: synchronise the device before reading)."""
    shards = _check_shards("search_range_shards", shards)
    G, cap = len(shards), int(cap)
    dev = _is_dev(queries)
    if not dev:
        queries = np.ascontiguousarray(queries, np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
    nq = int(queries.shape[0])
    c = max(cap, 0)
    ids = _empty_like_kind(queries, (G, nq, c), "int64")
    dist = _empty_like_kind(queries, (G, nq, c), "float32")
    counts = _empty_like_kind(queries, (G, nq), "int32")
    totals = _empty_like_kind(queries, (G, nq), "int64")
    for s, ix in enumerate(shards):
        ix.search_range(queries, radius, cap, flat_engine=flat_engine, out=(ids[s], dist[s], counts[s], totals[s]))
    if dev:
        for ix in shards:
            ix.synchronize()
    return merge_range(ids, dist, counts, totals, device=shards[0].device)


def select_shards(shards, skip=0, limit=None):
    """GpuIndex.select of a table held by G single-device indices (as search_range_shards): every shard lists its first skip + limit visible rows,
    merge_select cuts the window out of their merged order.  Returns (ids of the window, total) as GpuIndex.select does; limit=None: all rows."""
    shards = _check_shards("select_shards", shards)
    G = len(shards)
    rows = int(sum(ix.row_count for ix in shards))
    skip = int(skip)
    limit = rows if limit is None else int(limit)
    if skip < 0 or limit < 0:
        raise EpsillaError(lib.EPS_USER_ERROR, "select_shards: negative skip or limit")
    skip = min(skip, rows)               # (no rank reaches the number of rows: the window is cut to what can exist,
    window = min(limit, rows - skip)     #  and a shard's list reaches as far as it: skip + window ids at the most)
    length = skip + window
    ids = np.empty((G, length), np.int64)
    counts = np.zeros((G, 2), np.int64)
    for s, ix in enumerate(shards):
        ix.select(0, length, out=(ids[s], counts[s]))
    got, total = merge_select(ids, np.ascontiguousarray(counts[:, 0]), np.ascontiguousarray(counts[:, 1]), skip, window, device=shards[0].device)
    return got, total


# ---------------------------------------------------------------------------------------------------------
class ANNGraphSegment:
    """engine/db/ann_graph_segment.hpp:22-55.  Public members keep the reference's names."""

    def __init__(self, db_catalog_path=None, table_id=None, field_id=None, skip_sync_disk=True):
        self.skip_sync_disk_ = skip_sync_disk if db_catalog_path is None else False
        self.first_record_id_ = 0
        self.record_number_ = 0
        self.offset_table_ = np.zeros(1, np.int64)
        self.neighbor_list_ = np.zeros(0, np.int64)
        self.navigation_point_ = 0
        self._index = None
        if db_catalog_path is not None:  # file ctor, ann_graph_segment.cpp:39-98
            path = self._path(db_catalog_path, table_id, field_id)
            if os.path.exists(path):
                with open(path, "rb") as f:
                    hdr = np.fromfile(f, np.int64, 2)
                    self.record_number_, self.first_record_id_ = int(hdr[0]), int(hdr[1])
                    self.offset_table_ = np.fromfile(f, np.int64, self.record_number_ + 1)
                    self.neighbor_list_ = np.fromfile(f, np.int64, int(self.offset_table_[-1]))
                    self.navigation_point_ = int(np.fromfile(f, np.int64, 1)[0])
            else:
                os.makedirs(os.path.dirname(path), exist_ok=True)
                self.SaveANNGraph(db_catalog_path, table_id, field_id)

    @staticmethod
    def _path(db_catalog_path, table_id, field_id):
        return os.path.join(db_catalog_path, str(table_id), "ann_graph_%d.bin" % field_id)

    def BuildFromVectorTable(self, vector_column, n, dim, metricType, device=0, **build_kw):
        """ann_graph_segment.cpp:201-242, on the device: kNN graph -> NSG -> CSR."""
        ix = GpuIndex(dim, metricType, device)
        ix.attach_rows(vector_column[:n] if not hasattr(vector_column, "data_ptr") else vector_column)
        ix.build(n, **build_kw)
        self.offset_table_, self.neighbor_list_, self.navigation_point_ = ix.get_graph()
        self.record_number_ = n
        self._index = ix
        return self

    def SaveANNGraph(self, db_catalog_path, table_id, field_id, force=False):
        """ann_graph_segment.cpp:156-199 (tmp + fsync + rename); returns a status code."""
        if self.skip_sync_disk_ and not force:
            return 0
        path = self._path(db_catalog_path, table_id, field_id)
        tmp = path + ".tmp"
        try:
            with open(tmp, "wb") as f:
                np.array([self.record_number_, self.first_record_id_], np.int64).tofile(f)
                np.ascontiguousarray(self.offset_table_, np.int64).tofile(f)
                np.ascontiguousarray(self.neighbor_list_, np.int64).tofile(f)
                np.array([self.navigation_point_], np.int64).tofile(f)
                f.flush()
                os.fsync(f.fileno())
            os.rename(tmp, path)
        except OSError:
            return lib.EPS_DB_UNEXPECTED_ERROR
        return 0


class VecSearchExecutor:
    """engine/db/execution/vec_search_executor.hpp:30-74.  One query per Search() call like the reference;
    SearchBatch() is the additive batched entry."""

    def __init__(self, dimension, start_search_point, ann_index, offset_table, neighbor_list, vector_column,
                 fstdistfunc, dist_func_param=None, num_threads=4, L_master=500, L_local=500,
                 subsearch_iterations=15, prefilter_enabled=False, device=0):
        self.ann_index_ = ann_index
        self.total_indexed_vector_ = int(ann_index.record_number_)
        self.dimension_ = int(dimension)
        self.start_search_point_ = int(start_search_point)
        self.num_threads_, self.L_master_, self.L_local_ = num_threads, L_master, L_local
        self.subsearch_iterations_, self.prefilter_enabled_ = subsearch_iterations, prefilter_enabled
        self.brute_force_search_ = self.total_indexed_vector_ < BruteforceThreshold
        self.search_result_ = np.zeros(L_master, np.int64)
        self.distance_ = np.zeros(L_master, np.float64)
        self._ix = GpuIndex(dimension, fstdistfunc, device)
        self._rows = vector_column
        self._attached = -1
        self._graph = (np.asarray(offset_table, np.int64), np.asarray(neighbor_list, np.int64))

    def _sync(self, total_vector, deleted, filter_spec):
        if total_vector != self._attached:
            self._ix.attach_rows(self._rows[:total_vector])
            if self.total_indexed_vector_ > 0:
                self._ix.set_graph(self._graph[0], self._graph[1], self.start_search_point_)
            self._attached = total_vector
        self._ix.set_deleted(deleted)
        if filter_spec:
            self._ix.set_int_filter(*filter_spec)
        else:
            self._ix.set_int_filter(None, None, 0)

    def SearchBatch(self, queries, total_vector, limit, deleted=None, filter_spec=None):
        self._sync(total_vector, deleted, filter_spec)
        ids, dist, counts = self._ix.search(queries, limit, mode=MODE_REFERENCE, prefilter=int(self.prefilter_enabled_),
                                            intra_threads=self.num_threads_, master_queue=self.L_master_,
                                            local_queue=self.L_local_, sync_interval=self.subsearch_iterations_)
        return ids, dist, counts

    def Search(self, query_data, total_vector, limit, deleted=None, filter_spec=None):
        """Status Search(query, table_segment, limit, filter_nodes, result_size): returns (status, result_size);
        results land in search_result_ / distance_ (double), vec_search_executor.cpp:833-935."""
        ids, dist, counts = self.SearchBatch(np.asarray(query_data, np.float32)[None, :], total_vector, limit, deleted,
                                             filter_spec)
        n = int(counts[0])
        if n > len(self.search_result_):
            self.search_result_ = np.zeros(n, np.int64)
            self.distance_ = np.zeros(n, np.float64)
        self.search_result_[:n] = ids[0, :n]
        self.distance_[:n] = dist[0, :n].astype(np.float64)
        return 0, n

    def SearchByAttribute(self, total_vector, skip, limit, deleted=None, filter_spec=None):
        """Status SearchByAttribute(schema, table_segment, skip, limit, primary_keys, filter_nodes, result_size) without a primary-key
        list (vec_search_executor.cpp:937-1033, full-scan branch :1016-1029): returns (status, result_size); the row ids land in
        search_result_, in ascending row order."""
        self._sync(total_vector, deleted, filter_spec)
        limit = min(int(limit), int(total_vector))   # (:958-961)
        ids, _ = self._ix.select(skip, limit)
        n = len(ids)
        if n > len(self.search_result_):   # (:962-964)
            self.search_result_ = np.zeros(n, np.int64)
        self.search_result_[:n] = ids
        return 0, n
