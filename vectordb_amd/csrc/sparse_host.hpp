// Host side of the sparse-vector index (eps_sparse_index_*; kernels: sparse.hip, host state: sparse_index.cpp): the limits, the validation of CSR
// offsets and of host-resident indices, and the launch plan of the scan - how many queries a workgroup stages, how many wavefronts share the table
// and which rows each of them takes.  Plain C++ with no device type in it: tests/native/sparse_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"
#include "among_host.hpp"

namespace eps {

constexpr int32_t SPARSE_MAX_K = 1024;                         // the widest WaveTopK (KPL = 16)
constexpr int64_t SPARSE_MAX_ROWS = ((int64_t)1 << 31) - 1;    // rows of one table (a key carries a 32-bit row)
constexpr int64_t SPARSE_MAX_DIM = ((int64_t)1 << 31) - 1;     // indices are int32
constexpr int SPARSE_BLOCK_WAVES = 4;                          // wavefronts of a scan workgroup (launch_among_merge wants a multiple of 4 lists)
constexpr int SPARSE_WAVE_ROWS = 64;                           // rows of one round of a wavefront: one per lane
// CSR elements the first kernel form staged in LDS per wavefront and step (sparse.hip says why it went).  No length is special to the kernel
// now; the tests keep probing row lengths around this one and its double, where that form had its edges.
constexpr int SPARSE_PIECE = 512;
constexpr int64_t SPARSE_STATIC_LDS = 64;                      // per staged query its length and v2_prod
constexpr int64_t SPARSE_LDS_BUDGET = 65536;                   // per workgroup, all of it staged queries: two workgroups fit a CU's 160 KB
// non-zeros of one query: its (index, value) pairs are staged in LDS.  (65536 - 64) / 8 = 8184 fit; the power of two below it is the limit
constexpr int64_t SPARSE_MAX_QUERY_NNZ = 4096;
constexpr int64_t SPARSE_MAX_BLOCKS = 2048;                    // scan workgroups of one launch in x times query tiles (among_plan's figure)
constexpr int64_t SPARSE_GRID_Y = 32768;                       // query tiles of one launch; longer batches run in slices

enum : int32_t { SPARSE_BAD_NONE = 0, SPARSE_BAD_FIRST = 1, SPARSE_BAD_OFFSETS = 2, SPARSE_BAD_RANGE = 3, SPARSE_BAD_ORDER = 4 };
inline const char* sparse_bad_text(int32_t kind) {
  switch (kind) {
    case SPARSE_BAD_FIRST: return "offsets[0] must be 0";
    case SPARSE_BAD_OFFSETS: return "offsets must be non-decreasing";
    case SPARSE_BAD_RANGE: return "an index outside [0, dim)";
    case SPARSE_BAD_ORDER: return "indices must be strictly increasing inside a row";
  }
  return "";
}

// offsets[0 .. n]: EPS_OK and *nnz = offsets[n], *longest = the longest row - or EPS_USER_ERROR with the first offending row and the kind.
inline int32_t sparse_offsets_check(const int64_t* offsets, int64_t n, int64_t* nnz, int64_t* longest, int64_t* bad_row, int32_t* kind) {
  *nnz = 0;
  *longest = 0;
  *bad_row = -1;
  *kind = SPARSE_BAD_NONE;
  if (n < 0 || !offsets) return *kind = SPARSE_BAD_OFFSETS, EPS_USER_ERROR;
  if (offsets[0] != 0) return *bad_row = 0, *kind = SPARSE_BAD_FIRST, EPS_USER_ERROR;
  int64_t most = 0;
  for (int64_t r = 0; r < n; ++r) {
    if (offsets[r + 1] < offsets[r]) return *bad_row = r, *kind = SPARSE_BAD_OFFSETS, EPS_USER_ERROR;
    const int64_t len = offsets[r + 1] - offsets[r];
    most = len > most ? len : most;
  }
  *nnz = offsets[n];
  *longest = most;
  return EPS_OK;
}

// the row checks of the reference's insert path (table_segment_mvp.cpp:526-550) on host arrays whose offsets passed sparse_offsets_check: every
// index inside [0, dim), strictly increasing inside a row.  An empty row is accepted.
inline int32_t sparse_rows_check(const int64_t* offsets, const int32_t* indices, int64_t n, int64_t dim, int64_t* bad_row, int32_t* kind) {
  *bad_row = -1;
  *kind = SPARSE_BAD_NONE;
  for (int64_t r = 0; r < n; ++r) {
    int64_t prev = -1;
    for (int64_t e = offsets[r]; e < offsets[r + 1]; ++e) {
      const int64_t c = indices[e];
      if (c < 0 || c >= dim) return *bad_row = r, *kind = SPARSE_BAD_RANGE, EPS_USER_ERROR;
      if (c <= prev) return *bad_row = r, *kind = SPARSE_BAD_ORDER, EPS_USER_ERROR;
      prev = c;
    }
  }
  return EPS_OK;
}

struct SparsePlan {
  int nq_tile;            // queries staged per workgroup: 1, 2 or 4
  int64_t tiles;          // workgroups in y over the whole batch (launched in slices of SPARSE_GRID_Y)
  int W;                  // wavefronts = partial lists per query, a multiple of SPARSE_BLOCK_WAVES
  int64_t rows_per_wave;  // a multiple of SPARSE_WAVE_ROWS: wavefront w takes rows [w * rows_per_wave, (w + 1) * rows_per_wave) of the table
  int64_t qcap;           // LDS slots per staged query (>= the batch's longest query)
  int64_t lds_dynamic;    // bytes: nq_tile * qcap * 8
};
// n rows, nq queries of at most `longest_query` <= SPARSE_MAX_QUERY_NNZ non-zeros, 1 <= k <= SPARSE_MAX_K
inline SparsePlan sparse_plan(int64_t n, int64_t nq, int32_t k, int64_t longest_query) {
  SparsePlan p;
  p.qcap = (longest_query + 3) / 4 * 4;
  if (p.qcap < 4) p.qcap = 4;
  p.nq_tile = k > 128 ? 1 : (nq >= 3 ? 4 : (nq == 2 ? 2 : 1));   // (pick_nq's rule: the wide lists keep one query's registers)
  while (p.nq_tile > 1 && p.nq_tile * p.qcap * 8 + SPARSE_STATIC_LDS > SPARSE_LDS_BUDGET) p.nq_tile >>= 1;
  p.lds_dynamic = p.nq_tile * p.qcap * 8;
  p.tiles = (nq + p.nq_tile - 1) / p.nq_tile;
  int64_t gx = (n + (int64_t)SPARSE_WAVE_ROWS * SPARSE_BLOCK_WAVES - 1) / ((int64_t)SPARSE_WAVE_ROWS * SPARSE_BLOCK_WAVES);   // >= one round per wavefront
  int64_t cap = SPARSE_MAX_BLOCKS / (p.tiles > 0 ? p.tiles : 1);   // many queries fill the chip by themselves
  const int64_t cap_merge = AMONG_MERGE_KEYS / ((int64_t)k * SPARSE_BLOCK_WAVES);   // launch_among_merge: W * k <= AMONG_MERGE_KEYS where W > 4
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  p.W = (int)(gx * SPARSE_BLOCK_WAVES);
  const int64_t per = (n + p.W - 1) / p.W;
  p.rows_per_wave = (per + SPARSE_WAVE_ROWS - 1) / SPARSE_WAVE_ROWS * SPARSE_WAVE_ROWS;
  if (p.rows_per_wave < SPARSE_WAVE_ROWS) p.rows_per_wave = SPARSE_WAVE_ROWS;
  return p;
}
// rows [*begin, *end) of wavefront w (those beyond the table: begin = end = n); the kernel calls it too
EPS_AMONG_HD inline void sparse_wave_rows(const SparsePlan& p, int64_t n, int64_t w, int64_t* begin, int64_t* end) {
  const int64_t b = w * p.rows_per_wave < n ? w * p.rows_per_wave : n;   // (w < 2^13, rows_per_wave < 2^31: no overflow)
  *begin = b;
  *end = n - b < p.rows_per_wave ? n : b + p.rows_per_wave;
}

}  // namespace eps
