"""GpuSparseIndex: a sparse-vector field (SPARSE_VECTOR_FLOAT) over the C ABI's eps_sparse_index_* - a CSR table in HBM and its exact scan
(csrc/sparse.hip), optionally its inverted lists for dot and cosine (csrc/sparse_inverted.hip).  numpy arrays are host buffers; anything exposing `data_ptr()` (a torch tensor on the GPU) is passed as a device pointer and
used in place.  Every dtype, shape and contiguity is checked here, before a pointer reaches the library."""
import ctypes as C

import numpy as np

from . import _lib as lib
from ._lib import EpsillaError, SearchStats
from .index import METRICS, _is_dev, _ptr, _results

MAX_K = 1024


def _dtype(a):
    return str(a.dtype).replace("torch.", "")


def _flat(a, name, dtype, who):
    """a 1-D C-contiguous array of `dtype`: a device tensor as it is (or a ValueError), anything else converted to NumPy"""
    if _is_dev(a):
        if _dtype(a) != dtype or a.dim() != 1 or not a.is_contiguous():
            raise ValueError("%s: device %s must be a contiguous 1-D %s tensor, got %s %s" % (who, name, dtype, _dtype(a), tuple(a.shape)))
        return a
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError("%s: %s must be 1-D, got shape %s" % (who, name, a.shape))
    if a.size and a.dtype.kind not in ("iu" if dtype.startswith("int") else "iuf"):
        raise ValueError("%s: %s must be numeric (%s), got %s" % (who, name, dtype, a.dtype))
    return np.ascontiguousarray(a, getattr(np, dtype))


def _size(a):
    return a.numel() if _is_dev(a) else a.size


def _csr(offsets, indices, values, who):
    """(offsets, indices, values, rows): dtypes and lengths agree; the offsets' LAST entry is checked against the arrays where it is on the host"""
    offsets = _flat(offsets, "offsets", "int64", who)
    indices = _flat(indices, "indices", "int32", who)
    values = _flat(values, "values", "float32", who)
    if _size(offsets) < 1:
        raise ValueError("%s: offsets must hold rows + 1 entries, got none" % who)
    if _size(indices) != _size(values):
        raise ValueError("%s: indices and values differ in length (%d, %d)" % (who, _size(indices), _size(values)))
    if not _is_dev(offsets) and int(offsets[-1]) != _size(indices):
        raise ValueError("%s: offsets[-1] = %d, but indices and values hold %d entries" % (who, int(offsets[-1]), _size(indices)))
    return offsets, indices, values, _size(offsets) - 1


def queries_from_dicts(queries):
    """[{"indices": [...], "values": [...]}, ...] - the client's JSON shape of a sparse vector - as an (offsets, indices, values) triple"""
    off, idx, val = [0], [], []
    for j, q in enumerate(queries):
        qi, qv = list(q["indices"]), list(q["values"])
        if len(qi) != len(qv):
            raise ValueError("search: query %d has %d indices and %d values" % (j, len(qi), len(qv)))
        idx += qi
        val += qv
        off.append(len(idx))
    return np.asarray(off, np.int64), np.asarray(idx, np.int64).astype(np.int32), np.asarray(val, np.float32)


class GpuSparseIndex:
    def __init__(self, dim, metric="EUCLIDEAN", device=0):
        self.L = lib.load()
        self.dim = int(dim)
        self.metric = METRICS[metric]
        self.device = device
        h = C.c_void_p()
        rc = self.L.eps_sparse_index_create(self.dim, self.metric, device, C.byref(h))
        if rc != 0:
            raise EpsillaError(rc, "eps_sparse_index_create failed (no gfx950 device? there is no CPU fallback)")
        self.h = h
        self._keep = {}

    def _check(self, rc):
        if rc != 0:
            raise EpsillaError(rc, self.L.eps_sparse_index_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.eps_sparse_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach_csr(self, offsets, indices, values):
        """eps_sparse_index_attach_csr: all NumPy (copied) or all device tensors (borrowed, kept alive here)"""
        offsets, indices, values, n = _csr(offsets, indices, values, "attach_csr")
        self._check(self.L.eps_sparse_index_attach_csr(self.h, _ptr(offsets), _ptr(indices) if _size(indices) else None,
                                                       _ptr(values) if _size(values) else None, n))
        self._keep["csr"] = (offsets, indices, values)
        self._keep.pop("deleted", None)

    @property
    def row_count(self):
        return self.L.eps_sparse_index_row_count(self.h)

    def set_id_map(self, base, stride):
        self._check(self.L.eps_sparse_index_set_id_map(self.h, int(base), int(stride)))

    def set_deleted(self, bits):
        if bits is None:
            self._check(self.L.eps_sparse_index_set_deleted(self.h, None, 0))
            return
        bits = _flat(bits, "bits", "uint8", "set_deleted")
        self._check(self.L.eps_sparse_index_set_deleted(self.h, _ptr(bits), _size(bits)))
        self._keep["deleted"] = bits

    def search(self, queries, k, out=None):
        """eps_sparse_index_search.  queries: an (offsets, indices, values) triple - offsets on the host, indices / values NumPy or device
        tensors - or a list of {"indices": [...], "values": [...]} dicts.  Returns (ids int64[nq, k], dist float32[nq, k], counts int32[nq]) in
        ascending (distance, id) order, the rest -1 / +inf.  Device indices / values give device results and the call is asynchronous on the
        index's stream; out=(ids, dist, counts): caller-provided buffers, all NumPy or all device."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("search: k must be in [1, %d], got %d" % (MAX_K, k))
        if isinstance(queries, (list,)) and (not queries or isinstance(queries[0], dict)):
            queries = queries_from_dicts(queries)
        q_off, q_idx, q_val = queries
        if _is_dev(q_off):
            q_off = q_off.cpu().numpy()
        if _is_dev(q_idx) != _is_dev(q_val):
            raise ValueError("search: the queries' indices and values must both be NumPy arrays or both be device tensors")
        q_off, q_idx, q_val, nq = _csr(q_off, q_idx, q_val, "search")
        ids, dist, counts = _results("search", (("ids", (nq, k), "int64"), ("dist", (nq, k), "float32"), ("counts", (nq,), "int32")), out, q_idx)
        self._keep["queries"] = (q_off, q_idx, q_val)   # (device results: the call is still running when this returns)
        nnz = _size(q_idx)
        self._check(self.L.eps_sparse_index_search(self.h, _ptr(q_off), _ptr(q_idx) if nnz else None, _ptr(q_val) if nnz else None, nq, k, _ptr(ids),
                                                   _ptr(dist), _ptr(counts)))
        return ids, dist, counts

    def build_inverted(self):
        """eps_sparse_index_build_inverted: the attached table by column (8 * nnz + 8 * (dim + 1) bytes of device memory); DOT_PRODUCT and COSINE
        searches then sum term at a time on it and return the scan's bits.  attach_csr forgets it."""
        self._check(self.L.eps_sparse_index_build_inverted(self.h))

    def drop_inverted(self):
        self._check(self.L.eps_sparse_index_drop_inverted(self.h))

    def inverted_info(self):
        """{"built", "columns", "postings", "longest_column", "last_engine"}; last_engine: 0 none yet, 1 scan, 2 inverted lists"""
        cols, post, longest, engine = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.L.eps_sparse_index_inverted_info(self.h, C.byref(cols), C.byref(post), C.byref(longest), C.byref(engine)))
        return {"built": cols.value > 0, "columns": cols.value, "postings": post.value, "longest_column": longest.value, "last_engine": engine.value}

    def inverted_arrays(self):
        """eps_sparse_index_get_inverted: host copies (col_offsets int64[dim + 1], rows int32[nnz], values float32[nnz])"""
        info = self.inverted_info()
        if not info["built"]:
            raise ValueError("inverted_arrays: no inverted lists (build_inverted first)")
        off = np.empty(self.dim + 1, np.int64)
        rows, values = np.empty(info["postings"], np.int32), np.empty(info["postings"], np.float32)
        self._check(self.L.eps_sparse_index_get_inverted(self.h, off.ctypes.data, rows.ctypes.data if rows.size else None,
                                                         values.ctypes.data if values.size else None))
        return off, rows, values

    def stats(self):
        s = SearchStats()
        self._check(self.L.eps_sparse_index_last_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in SearchStats._fields_}

    def synchronize(self):
        self._check(self.L.eps_sparse_index_synchronize(self.h))

    def use_torch_stream(self, stream=None):
        """run on a torch stream (None: torch's current one), so that device tensors produced on it need no extra synchronisation"""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        self._keep["stream"] = s
        self._check(self.L.eps_sparse_index_set_stream(self.h, C.c_void_p(s.cuda_stream)))
        return self
