// Host side of the hybrid search (eps_index_search_hybrid; kernels: hybrid.hip): the limits, the checks of the call's scalar arguments, the launch
// plan - how many queries a workgroup stages, how many wavefronts share the table and which rows each of them takes - and the layout of the
// workgroup's dynamic LDS.  Plain C++ with no device type in it: the launcher and the kernel read the same plan, and
// tests/native/hybrid_host_check.cpp runs it under a sanitizer.
//
// The LDS of one workgroup of hybrid_tile_kernel, in this order (every part starts on a multiple of 16 bytes):
//   [nq_tile][qstride] float      the dense queries, qstride = dim rounded up to 4
//   [nq_tile][qcap] int32         the sparse queries' indices, qcap = the batch's longest query rounded up to 4 (at least 4)
//   [nq_tile][qcap] float         ... and their values
//   [HYB_BLOCK_WAVES][nq_tile][HYB_TILE_ROWS] float   per wavefront one accumulator per (query, row of its tile)
// dim 768, four queries of 1024 terms: 12 + 32 + 32 = 76 KB - above the budget, so such a batch runs two queries per workgroup (6 + 16 + 16 KB);
// at the 128 terms of a SPLADE-like query four queries take 12 + 4 + 32 = 48 KB.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sparse_inv_host.hpp"

namespace eps {

constexpr int32_t HYB_MAX_K = 1024;                       // the widest WaveTopK (KPL = 16)
constexpr int HYB_BLOCK_WAVES = 4;                        // wavefronts of a workgroup (launch_among_merge wants a multiple of 4 lists)
constexpr int HYB_TILE_ROWS = 512;                        // rows whose sparse sums a wavefront holds in LDS at once, per staged query
constexpr int64_t HYB_MAX_QUERY_NNZ = 1024;               // non-zeros of one sparse query: its pairs are staged in LDS next to the dense queries
constexpr int64_t HYB_LDS_BUDGET = 65536;                 // per workgroup, all of it dynamic: two workgroups fit a CU's 160 KB
constexpr int64_t HYB_STATIC_LDS = 0;                     // the kernels declare none
constexpr int64_t HYB_MIN_BLOCKS = 256;                   // workgroups wanted before a wavefront is given a whole tile of rows
constexpr int64_t HYB_MAX_BLOCKS = 2048;                  // workgroups of one launch in x times query tiles (among_plan's figure)
constexpr int64_t HYB_GRID_Y = 32768;                     // query tiles of one launch; longer batches run in slices
constexpr int64_t HYB_PARTS_LDS_BUDGET = 65536;           // hybrid_parts_kernel: one dense and one sparse query

// EPS_OK, or EPS_USER_ERROR with the reason in *why: what the call refuses before it looks at a buffer
inline int32_t hybrid_args_check(int64_t nq, int32_t k, float w_dense, float w_sparse, const char** why) {
  *why = "";
  if (k < 1 || k > HYB_MAX_K) return *why = "k must be in [1, 1024]", EPS_USER_ERROR;
  if (nq < 0) return *why = "nq must be >= 0", EPS_USER_ERROR;
  if (nq > SPARSE_MAX_ROWS) return *why = "more than 2^31 - 1 queries", EPS_USER_ERROR;
  // (x - x is 0 for a finite x and NaN for +-inf and NaN: no <math.h> needed)
  if (!(w_dense - w_dense == 0.0f) || !(w_sparse - w_sparse == 0.0f)) return *why = "w_dense and w_sparse must be finite", EPS_USER_ERROR;
  return EPS_OK;
}

// bytes of dynamic LDS of a workgroup that stages nq_tile queries of `dim` columns and `qcap` sparse slots
inline int64_t hybrid_lds_bytes(int nq_tile, int64_t dim, int64_t qcap) {
  const int64_t qstride = (dim + 3) / 4 * 4;
  return (int64_t)nq_tile * qstride * 4 + (int64_t)nq_tile * qcap * 8 + (int64_t)HYB_BLOCK_WAVES * nq_tile * HYB_TILE_ROWS * 4;
}
// the widest dense row one staged query of `qcap` sparse slots leaves room for
inline int64_t hybrid_max_dim(int64_t qcap) { return (HYB_LDS_BUDGET - HYB_STATIC_LDS - qcap * 8 - (int64_t)HYB_BLOCK_WAVES * HYB_TILE_ROWS * 4) / 4 / 4 * 4; }

struct HybridPlan {
  SparsePlan rows;        // nq_tile in {1, 2, 4}, tiles; W, rows_per_wave (a multiple of SPARSE_WAVE_ROWS) for sparse_wave_rows; qcap; lds_dynamic
  int qstride;            // floats per staged dense query
  int64_t idx_offset;     // byte offsets of the parts in dynamic LDS
  int64_t val_offset;
  int64_t acc_offset;
};
// n rows of `dim` columns, nq queries whose sparse sides hold at most `longest_query` <= HYB_MAX_QUERY_NNZ non-zeros, 1 <= k <= HYB_MAX_K.
// false: even one staged query does not fit HYB_LDS_BUDGET (dim > hybrid_max_dim) - nothing is launched.  The outer plan is sparse_inv_plan's: a
// wavefront gets whole tiles of rows unless that leaves the chip short of workgroups, then half a tile, and so on down to 64 rows.
inline bool hybrid_plan(int64_t n, int64_t nq, int32_t k, int64_t dim, int64_t longest_query, HybridPlan* p) {
  SparsePlan& r = p->rows;
  r.qcap = (longest_query + 3) / 4 * 4;
  if (r.qcap < 4) r.qcap = 4;
  r.nq_tile = k > 128 ? 1 : (nq >= 3 ? 4 : (nq == 2 ? 2 : 1));   // (pick_nq's rule: the wide lists keep one query's registers)
  while (r.nq_tile > 1 && HYB_STATIC_LDS + hybrid_lds_bytes(r.nq_tile, dim, r.qcap) > HYB_LDS_BUDGET) r.nq_tile >>= 1;
  if (dim < 1 || HYB_STATIC_LDS + hybrid_lds_bytes(r.nq_tile, dim, r.qcap) > HYB_LDS_BUDGET) return false;
  r.tiles = (nq + r.nq_tile - 1) / r.nq_tile;
  r.lds_dynamic = hybrid_lds_bytes(r.nq_tile, dim, r.qcap);
  p->qstride = (int)((dim + 3) / 4 * 4);
  p->idx_offset = (int64_t)r.nq_tile * p->qstride * 4;
  p->val_offset = p->idx_offset + (int64_t)r.nq_tile * r.qcap * 4;
  p->acc_offset = p->val_offset + (int64_t)r.nq_tile * r.qcap * 4;
  int64_t per_wave = HYB_TILE_ROWS;
  const int64_t tiles = r.tiles > 0 ? r.tiles : 1;
  while (per_wave > SPARSE_WAVE_ROWS && (n + per_wave * HYB_BLOCK_WAVES - 1) / (per_wave * HYB_BLOCK_WAVES) * tiles < HYB_MIN_BLOCKS) per_wave >>= 1;
  int64_t gx = (n + per_wave * HYB_BLOCK_WAVES - 1) / (per_wave * HYB_BLOCK_WAVES);
  int64_t cap = HYB_MAX_BLOCKS / tiles;   // many queries fill the chip by themselves
  const int64_t cap_merge = AMONG_MERGE_KEYS / ((int64_t)k * HYB_BLOCK_WAVES);   // launch_among_merge: W * k <= AMONG_MERGE_KEYS where W > 4
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  r.W = (int)(gx * HYB_BLOCK_WAVES);
  const int64_t per = (n + r.W - 1) / r.W;
  r.rows_per_wave = (per + SPARSE_WAVE_ROWS - 1) / SPARSE_WAVE_ROWS * SPARSE_WAVE_ROWS;
  if (r.rows_per_wave < SPARSE_WAVE_ROWS) r.rows_per_wave = SPARSE_WAVE_ROWS;
  return true;
}

// hybrid_parts_kernel stages ONE dense query and ONE sparse query: [qstride] float, [qcap] int32, [qcap] float
inline int64_t hybrid_parts_lds_bytes(int64_t dim, int64_t qcap) { return (dim + 3) / 4 * 4 * 4 + qcap * 8; }

}  // namespace eps
