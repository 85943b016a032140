"""GpuBinaryIndex: a 1-bit-per-dimension field over the C ABI's eps_binary_index_* - a table of packed bits in HBM and its exact Hamming scan
(csrc/binary.hip).  A vector of `dim` bits is W = ceil(dim / 32) words; bit j is bit j % 32 of word j / 32 - np.packbits(bits, axis=-1,
bitorder="little") viewed as uint32 on a little-endian host; the pad bits of the last word may hold anything.  numpy arrays are host buffers;
anything exposing `data_ptr()` (a torch tensor on the GPU) is passed as a device pointer and used in place - device words are int32 or uint32
tensors (the same 32 bits).  Every dtype, shape and contiguity is checked here, before a pointer reaches the library."""
import ctypes as C

import numpy as np

from . import _lib as lib
from ._lib import EpsillaError, SearchStats
from .index import _empty_like_kind, _is_dev, _ptr, _results

MAX_K = 1024
MAX_DIM = 65536


def words_per_vector(dim):
    return (int(dim) + 31) // 32


def _dtype(a):
    return str(a.dtype).replace("torch.", "")


def _words(a, name, W, who, strided=False):
    """a [m, W] array of packed words, rows contiguous: a device tensor as it is (or a ValueError), anything else as a C-contiguous uint32 array.
    strided: a device tensor's rows may lie `stride(0) >= W` words apart.  Returns (array, rows, stride in words)"""
    if _is_dev(a):
        ok = _dtype(a) in ("int32", "uint32") and a.dim() == 2 and a.shape[1] == W
        if ok and a.shape[0] > 0:
            ok = a.stride(1) == 1 and (a.stride(0) >= W if strided else a.stride(0) == W)
        if not ok:
            raise ValueError("%s: device %s must be an int32 / uint32 tensor of shape [m, %d] with contiguous rows, got %s %s" % (who, name, W, _dtype(a), tuple(a.shape)))
        return a, int(a.shape[0]), int(a.stride(0)) if a.shape[0] > 0 else W
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != W:
        raise ValueError("%s: %s must have shape [m, %d] (ceil(dim / 32) words per vector), got %s" % (who, name, W, a.shape))
    if a.dtype not in (np.uint32, np.int32):
        raise ValueError("%s: %s must be uint32 words, got %s" % (who, name, a.dtype))
    return np.ascontiguousarray(a).view(np.uint32), int(a.shape[0]), W


def _floats(a, name, dim, who):
    """a C-contiguous float32 [m, dim] array or device tensor"""
    if _is_dev(a):
        if _dtype(a) != "float32" or a.dim() != 2 or a.shape[1] != dim or not a.is_contiguous():
            raise ValueError("%s: device %s must be a contiguous float32 tensor of shape [m, %d], got %s %s" % (who, name, dim, _dtype(a), tuple(a.shape)))
        return a
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError("%s: %s must have shape [m, %d], got %s" % (who, name, dim, a.shape))
    if a.dtype.kind not in "iuf":
        raise ValueError("%s: %s must be numeric (float32), got %s" % (who, name, a.dtype))
    return np.ascontiguousarray(a, np.float32)


class GpuBinaryIndex:
    def __init__(self, dim, device=0):
        self.dim = int(dim)
        if not 1 <= self.dim <= MAX_DIM:
            raise ValueError("GpuBinaryIndex: dim must be in [1, %d], got %d" % (MAX_DIM, self.dim))
        self.W = words_per_vector(self.dim)
        self.L = lib.load()
        self.device = device
        h = C.c_void_p()
        rc = self.L.eps_binary_index_create(self.dim, device, C.byref(h))
        if rc != 0:
            raise EpsillaError(rc, "eps_binary_index_create failed (no gfx950 device? there is no CPU fallback)")
        self.h = h
        self._keep = {}

    def _check(self, rc):
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_binary_index_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.eps_binary_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach_rows(self, words):
        """eps_binary_index_attach_rows: [n, W] packed words - NumPy (copied) or a device tensor (borrowed, kept alive here; its rows may be a
        strided view, stride(0) >= W)"""
        words, n, stride = _words(words, "words", self.W, "attach_rows", strided=True)
        self._check(self.L.eps_binary_index_attach_rows(self.h, _ptr(words) if n else None, n, stride))
        self._keep["rows"] = words if _is_dev(words) else None
        self._keep.pop("deleted", None)

    def attach_signs(self, rows):
        """eps_binary_index_attach_signs: float32 [n, dim], NumPy or device; bit j of row r = rows[r, j] > 0, packed on the device into a table the
        index owns"""
        rows = _floats(rows, "rows", self.dim, "attach_signs")
        n = int(rows.shape[0])
        self._check(self.L.eps_binary_index_attach_signs(self.h, _ptr(rows) if n else None, n))
        self._keep["rows"] = None
        self._keep.pop("deleted", None)

    def pack_signs(self, x, out=None):
        """eps_binary_index_pack_signs: float32 [m, dim] -> words [m, W] of the kind x is (uint32 array / int32 device tensor), pad bits clear"""
        x = _floats(x, "x", self.dim, "pack_signs")
        m = int(x.shape[0])
        if out is None:
            out = _empty_like_kind(x, (m, self.W), "int32" if _is_dev(x) else "uint32")
        elif _is_dev(out) != _is_dev(x):
            raise ValueError("pack_signs: x and out must both be NumPy arrays or both be device tensors")
        else:
            if not _is_dev(out) and (out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"]):
                raise ValueError("pack_signs: out must be a C-contiguous uint32 array of shape (%d, %d), got %s" % (m, self.W, out.dtype))
            out, rows, _ = _words(out, "out", self.W, "pack_signs")
            if rows != m:
                raise ValueError("pack_signs: out must have shape (%d, %d), got %s" % (m, self.W, tuple(out.shape)))
        self._keep["pack"] = (x, out)   # (device buffers: the call is still running when this returns)
        self._check(self.L.eps_binary_index_pack_signs(self.h, _ptr(x) if m else None, m, _ptr(out) if m else None))
        return out

    @property
    def row_count(self):
        return self.L.eps_binary_index_row_count(self.h)

    def set_id_map(self, base, stride):
        self._check(self.L.eps_binary_index_set_id_map(self.h, int(base), int(stride)))

    def set_deleted(self, bits):
        if bits is None:
            self._check(self.L.eps_binary_index_set_deleted(self.h, None, 0))
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
        self._check(self.L.eps_binary_index_set_deleted(self.h, _ptr(bits), size))
        self._keep["deleted"] = bits

    def search(self, queries, k, out=None):
        """eps_binary_index_search.  queries: [nq, W] packed words.  Returns (ids int64[nq, k], dist int32[nq, k], counts int32[nq]) in ascending
        (Hamming distance, id) order, the rest -1 / INT32_MAX.  Device queries give device results and the call is asynchronous on the index's
        stream; out=(ids, dist, counts): caller-provided buffers of the kind the queries are."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("search: k must be in [1, %d], got %d" % (MAX_K, k))
        queries, nq, _ = _words(queries, "queries", self.W, "search")
        ids, dist, counts = _results("search", (("ids", (nq, k), "int64"), ("dist", (nq, k), "int32"), ("counts", (nq,), "int32")), out, queries)
        if _is_dev(ids) != _is_dev(queries):
            raise ValueError("search: queries and out must all be NumPy arrays or all be device tensors")
        self._keep["queries"] = (queries, ids, dist, counts)   # (device results: the call is still running when this returns)
        self._check(self.L.eps_binary_index_search(self.h, _ptr(queries) if nq else None, nq, k, _ptr(ids), _ptr(dist), _ptr(counts)))
        return ids, dist, counts

    def stats(self):
        s = SearchStats()
        self._check(self.L.eps_binary_index_last_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in SearchStats._fields_}

    def synchronize(self):
        self._check(self.L.eps_binary_index_synchronize(self.h))

    def use_torch_stream(self, stream=None):
        """run on a torch stream (None: torch's current one), so that device tensors produced on it need no extra synchronisation"""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        self._keep["stream"] = s
        self._check(self.L.eps_binary_index_set_stream(self.h, C.c_void_p(s.cuda_stream)))
        return self
