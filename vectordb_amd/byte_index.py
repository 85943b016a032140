"""GpuByteIndex: a one-byte-per-dimension field, int8 or uint8, over the C ABI's eps_byte_index_* - a table of bytes in HBM and its exact int32 top-k
on the matrix cores (csrc/byte.hip).  EUCLIDEAN distances are sum (x - q)^2, DOT_PRODUCT distances -sum x q; COSINE is not an integer rule and is
refused.  numpy arrays are host buffers; anything exposing `data_ptr()` (a torch tensor on the GPU) is passed as a device pointer.  The index always
keeps its own copy of the table, in its stored form.  Every dtype, shape and contiguity is checked here, before a pointer reaches the library."""
import ctypes as C

import numpy as np

from . import _lib as lib
from ._lib import EpsillaError, SearchStats
from .index import METRICS, _is_dev, _ptr, _results

MAX_K = 1024
MAX_DIM = 4096


def _dtype(a):
    return str(a.dtype).replace("torch.", "")


def _bytes(a, name, dim, dtype, who, strided=False):
    """a [m, dim] array of `dtype` bytes, rows contiguous: a device tensor as it is (or a ValueError), anything else as a C-contiguous array.
    strided: a device tensor's rows may lie `stride(0) >= dim` bytes apart.  Returns (array, rows, stride in bytes)"""
    if _is_dev(a):
        ok = _dtype(a) == dtype and a.dim() == 2 and a.shape[1] == dim
        if ok and a.shape[0] > 0:
            ok = a.stride(1) == 1 and (a.stride(0) >= dim if strided else a.stride(0) == dim)
        if not ok:
            raise ValueError("%s: device %s must be an %s tensor of shape [m, %d] with contiguous rows, got %s %s" % (who, name, dtype, dim, _dtype(a), tuple(a.shape)))
        return a, int(a.shape[0]), int(a.stride(0)) if a.shape[0] > 0 else dim
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError("%s: %s must have shape [m, %d], got %s" % (who, name, dim, a.shape))
    if a.dtype != np.dtype(dtype):
        raise ValueError("%s: %s must be %s bytes, got %s" % (who, name, dtype, a.dtype))
    return np.ascontiguousarray(a), int(a.shape[0]), dim


class GpuByteIndex:
    def __init__(self, dim, metric="EUCLIDEAN", unsigned=False, device=0):
        self.dim = int(dim)
        if not 1 <= self.dim <= MAX_DIM:
            raise ValueError("GpuByteIndex: dim must be in [1, %d], got %d" % (MAX_DIM, self.dim))
        self.metric = METRICS[metric]
        if self.metric == METRICS["COSINE"]:
            raise ValueError("GpuByteIndex: COSINE is not an integer rule; byte fields serve EUCLIDEAN and DOT_PRODUCT")
        self.unsigned = bool(unsigned)
        self.dtype = "uint8" if self.unsigned else "int8"
        self.L = lib.load()
        self.device = device
        h = C.c_void_p()
        rc = self.L.eps_byte_index_create(self.dim, self.metric, int(self.unsigned), device, C.byref(h))
        if rc != 0:
            raise EpsillaError(rc, "eps_byte_index_create failed (no gfx950 device? there is no CPU fallback)")
        self.h = h
        self._keep = {}

    def _check(self, rc):
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_byte_index_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.eps_byte_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach_rows(self, rows):
        """eps_byte_index_attach_rows: [n, dim] int8 / uint8 - NumPy or a device tensor (its rows may be a strided view, stride(0) >= dim); copied
        into the index's stored form either way"""
        rows, n, stride = _bytes(rows, "rows", self.dim, self.dtype, "attach_rows", strided=True)
        self._check(self.L.eps_byte_index_attach_rows(self.h, _ptr(rows) if n else None, n, stride))
        self._keep.pop("deleted", None)

    @property
    def row_count(self):
        return self.L.eps_byte_index_row_count(self.h)

    def set_id_map(self, base, stride):
        self._check(self.L.eps_byte_index_set_id_map(self.h, int(base), int(stride)))

    def set_deleted(self, bits):
        if bits is None:
            self._check(self.L.eps_byte_index_set_deleted(self.h, None, 0))
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
        self._check(self.L.eps_byte_index_set_deleted(self.h, _ptr(bits), size))
        self._keep["deleted"] = bits

    def search(self, queries, k, out=None):
        """eps_byte_index_search.  queries: [nq, dim] bytes of the index's signedness.  Returns (ids int64[nq, k], dist int32[nq, k], counts
        int32[nq]) in ascending (distance, id) order, the rest -1 / INT32_MAX.  Device queries give device results and the call is asynchronous on
        the index's stream; out=(ids, dist, counts): caller-provided buffers of the kind the queries are."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("search: k must be in [1, %d], got %d" % (MAX_K, k))
        queries, nq, _ = _bytes(queries, "queries", self.dim, self.dtype, "search")
        ids, dist, counts = _results("search", (("ids", (nq, k), "int64"), ("dist", (nq, k), "int32"), ("counts", (nq,), "int32")), out, queries)
        if _is_dev(ids) != _is_dev(queries):
            raise ValueError("search: queries and out must all be NumPy arrays or all be device tensors")
        self._keep["queries"] = (queries, ids, dist, counts)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_byte_index_search(self.h, _ptr(queries) if nq else None, nq, k, _ptr(ids), _ptr(dist), _ptr(counts)))
        return ids, dist, counts

    def stats(self):
        """eps_byte_index_last_stats, and the scan's form spelt out: live_columns, kpl, rounds and hit_rounds"""
        s = SearchStats()
        self._check(self.L.eps_byte_index_last_stats(self.h, C.byref(s)))
        d = {f: getattr(s, f) for f, _ in SearchStats._fields_}
        d.update(live_columns=d["expansions"] // 100, kpl=d["expansions"] % 100, rounds=d["filter_rows_all"], hit_rounds=d["rerank_rows"])
        return d

    def synchronize(self):
        self._check(self.L.eps_byte_index_synchronize(self.h))

    def use_torch_stream(self, stream=None):
        """run on a torch stream (None: torch's current one), so that device tensors produced on it need no extra synchronisation"""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        self._keep["stream"] = s
        self._check(self.L.eps_byte_index_set_stream(self.h, C.c_void_p(s.cuda_stream)))
        return self
