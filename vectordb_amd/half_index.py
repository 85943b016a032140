"""GpuHalfIndex: a half-precision field, fp16 or bf16, over the C ABI's eps_half_index_* - a table of halves in HBM and its fp32 top-k on the
matrix cores (csrc/half.hip), EUCLIDEAN, COSINE (normalising is the caller's job) or DOT_PRODUCT.  Device tensors are torch.float16 /
torch.bfloat16 and are passed as device pointers; host arrays are np.float16 for an fp16 index and np.uint16 bit patterns for a bf16 index (NumPy
has no bf16).  The index always keeps its own copy of the table, in its stored form.  Every dtype, shape and contiguity is checked here, before a
pointer reaches the library."""
import ctypes as C

import numpy as np

from . import _lib as lib
from ._lib import EpsillaError, SearchStats
from .index import METRICS, _is_dev, _ptr, _results

MAX_K = 1024
MAX_DIM = 4096
DTYPES = {"float16": ("float16", "float16"), "bfloat16": ("bfloat16", "uint16")}   # name -> (device dtype, host dtype)


def _dtype(a):
    return str(a.dtype).replace("torch.", "")


def _rows(a, name, dim, dev_dtype, host_dtype, who, strided=False):
    """a [m, dim] array, rows contiguous: a device tensor of `dev_dtype` as it is (or a ValueError), anything else as a C-contiguous array of
    `host_dtype`.  strided: a device tensor's rows may lie `stride(0) >= dim` elements apart.  Returns (array, rows, stride in elements)"""
    if _is_dev(a):
        ok = _dtype(a) == dev_dtype and a.dim() == 2 and a.shape[1] == dim
        if ok and a.shape[0] > 0:
            ok = a.stride(1) == 1 and (a.stride(0) >= dim if strided else a.stride(0) == dim)
        if not ok:
            raise ValueError("%s: device %s must be a %s tensor of shape [m, %d] with contiguous rows, got %s %s" % (who, name, dev_dtype, dim, _dtype(a), tuple(a.shape)))
        return a, int(a.shape[0]), int(a.stride(0)) if a.shape[0] > 0 else dim
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError("%s: %s must have shape [m, %d], got %s" % (who, name, dim, a.shape))
    if a.dtype != np.dtype(host_dtype):
        raise ValueError("%s: %s must be %s%s, got %s" % (who, name, host_dtype, " bit patterns of bfloat16" if dev_dtype == "bfloat16" and host_dtype == "uint16" else "", a.dtype))
    return np.ascontiguousarray(a), int(a.shape[0]), dim


class GpuHalfIndex:
    def __init__(self, dim, metric="EUCLIDEAN", dtype="float16", device=0):
        self.dim = int(dim)
        if not 1 <= self.dim <= MAX_DIM:
            raise ValueError("GpuHalfIndex: dim must be in [1, %d], got %d" % (MAX_DIM, self.dim))
        if dtype not in DTYPES:
            raise ValueError("GpuHalfIndex: dtype must be 'float16' or 'bfloat16', got %r" % (dtype,))
        self.metric = METRICS[metric]
        self.dtype = dtype
        self.dev_dtype, self.host_dtype = DTYPES[dtype]
        self.L = lib.load()
        self.device = device
        h = C.c_void_p()
        rc = self.L.eps_half_index_create(self.dim, self.metric, int(dtype == "bfloat16"), device, C.byref(h))
        if rc != 0:
            raise EpsillaError(rc, "eps_half_index_create failed (no gfx950 device? there is no CPU fallback)")
        self.h = h
        self._keep = {}

    def _check(self, rc):
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_half_index_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.eps_half_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach_rows(self, rows):
        """eps_half_index_attach_rows: [n, dim] halves - np.float16 / np.uint16 bf16 patterns, or a device tensor (its rows may be a strided view,
        stride(0) >= dim); copied into the index's stored form either way"""
        rows, n, stride = _rows(rows, "rows", self.dim, self.dev_dtype, self.host_dtype, "attach_rows", strided=True)
        self._check(self.L.eps_half_index_attach_rows(self.h, _ptr(rows) if n else None, n, stride))
        self._keep.pop("deleted", None)

    def attach_floats(self, rows):
        """eps_half_index_attach_floats: [n, dim] float32, host or device, each element rounded to the index's type (nearest, ties to even)"""
        rows, n, _ = _rows(rows, "rows", self.dim, "float32", "float32", "attach_floats")
        self._check(self.L.eps_half_index_attach_floats(self.h, _ptr(rows) if n else None, n))
        self._keep.pop("deleted", None)

    def convert_floats(self, x):
        """eps_half_index_convert_floats: [m, dim] float32 -> halves of the index's type with attach_floats' rounding: a device tensor gives a
        device tensor (asynchronous on the index's stream), a NumPy array np.float16 or np.uint16 bf16 patterns"""
        x, m, _ = _rows(x, "x", self.dim, "float32", "float32", "convert_floats")
        if _is_dev(x):
            import torch
            out = torch.empty((m, self.dim), dtype=getattr(torch, self.dev_dtype), device=x.device)
        else:
            out = np.empty((m, self.dim), self.host_dtype)
        self._keep["convert"] = (x, out)
        if m:
            self._check(self.L.eps_half_index_convert_floats(self.h, _ptr(x), m, _ptr(out)))
        return out

    @property
    def row_count(self):
        return self.L.eps_half_index_row_count(self.h)

    def set_id_map(self, base, stride):
        self._check(self.L.eps_half_index_set_id_map(self.h, int(base), int(stride)))

    def set_deleted(self, bits):
        if bits is None:
            self._check(self.L.eps_half_index_set_deleted(self.h, None, 0))
            return
        if _is_dev(bits):
            if _dtype(bits) != "uint8" or bits.dim() != 1 or not bits.is_contiguous():
                raise ValueError("set_deleted: device bits must be a contiguous 1-D uint8 tensor, got %s %s" % (_dtype(bits), tuple(bits.shape)))
            size = bits.numel()
        else:
            bits = np.asarray(bits)
            if bits.ndim != 1 or bits.dtype != np.uint8:
                raise ValueError("set_deleted: bits must be a 1-D uint8 array, got %s %s" % (bits.dtype, bits.shape))
            bits = np.ascontiguousarray(bits)
            size = bits.size
        self._check(self.L.eps_half_index_set_deleted(self.h, _ptr(bits), size))
        self._keep["deleted"] = bits

    def search(self, queries, k, out=None):
        """eps_half_index_search.  queries: [nq, dim] halves of the index's type.  Returns (ids int64[nq, k], dist float32[nq, k], counts
        int32[nq]) in ascending (distance, id) order, the rest -1 / +inf.  Device queries give device results and the call is asynchronous on the
        index's stream; out=(ids, dist, counts): caller-provided buffers of the kind the queries are."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("search: k must be in [1, %d], got %d" % (MAX_K, k))
        queries, nq, _ = _rows(queries, "queries", self.dim, self.dev_dtype, self.host_dtype, "search")
        ids, dist, counts = _results("search", (("ids", (nq, k), "int64"), ("dist", (nq, k), "float32"), ("counts", (nq,), "int32")), out, queries)
        if _is_dev(ids) != _is_dev(queries):
            raise ValueError("search: queries and out must all be NumPy arrays or all be device tensors")
        self._keep["queries"] = (queries, ids, dist, counts)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_half_index_search(self.h, _ptr(queries) if nq else None, nq, k, _ptr(ids), _ptr(dist), _ptr(counts)))
        return ids, dist, counts

    def stats(self):
        """eps_half_index_last_stats, and the scan's form spelt out: live_columns, kpl, rounds, hit_rounds, seeded, seed_rows, seed_hit_rounds"""
        s = SearchStats()
        self._check(self.L.eps_half_index_last_stats(self.h, C.byref(s)))
        d = {f: getattr(s, f) for f, _ in SearchStats._fields_}
        d.update(live_columns=d["expansions"] // 100, kpl=d["expansions"] % 100, rounds=d["filter_rows_all"], hit_rounds=d["rerank_rows"],
                 seeded=bool(d["overflow_queries"]), seed_rows=d["i8_folded"], seed_hit_rounds=d["i8_declined"])
        return d

    def synchronize(self):
        self._check(self.L.eps_half_index_synchronize(self.h))

    def use_torch_stream(self, stream=None):
        """run on a torch stream (None: torch's current one), so that device tensors produced on it need no extra synchronisation"""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        self._keep["stream"] = s
        self._check(self.L.eps_half_index_set_stream(self.h, C.c_void_p(s.cuda_stream)))
        return self
