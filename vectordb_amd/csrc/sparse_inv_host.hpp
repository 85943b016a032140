// Host side of the inverted lists of a sparse-vector index (eps_sparse_index_build_inverted; kernels: sparse_inverted.hip, host state:
// sparse_index.cpp): the column limit, the sizes of the image and of the build's scratch, the tile of rows a wavefront sums at once with the LDS
// layout that follows from it, and the launch plan of the term-at-a-time search.  Plain C++ with no device type in it:
// tests/native/sparse_inv_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sparse_host.hpp"

namespace eps {

// the column directory is dense: col_offsets int64[dim + 1].  2^24 columns are 128 MB of it and three 8-bit digits of a stable sort by column
constexpr int64_t SPARSE_INV_MAX_DIM = 16777216;
// rows whose fp32 accumulators one wavefront keeps in its LDS slice: 8 KB per wavefront, 32 KB per workgroup - with one query of
// SPARSE_MAX_QUERY_NNZ staged pairs (32 KB) exactly SPARSE_LDS_BUDGET, so the search kernel declares no static LDS at all
constexpr int SPARSE_INV_TILE_ROWS = 2048;
constexpr int64_t SPARSE_INV_ACC_BYTES = (int64_t)SPARSE_BLOCK_WAVES * SPARSE_INV_TILE_ROWS * 4;
constexpr int64_t SPARSE_INV_STATIC_LDS = 0;
constexpr int SPARSE_INV_TERMS = 64;                            // query terms matched per round: one per lane
constexpr int64_t SPARSE_INV_MAX_NNZ = (int64_t)1 << 40;        // beyond it the byte counts below are refused, long before int64 could wrap
constexpr int64_t SPARSE_INV_MIN_BLOCKS = 256;                 // workgroups wanted before a wavefront is given a whole tile of rows
constexpr int64_t SPARSE_INV_BUILD_BLOCKS = 65536;              // workgroups of a build launch at most: its kernels stride over the rest

// a posting as the image stores it: the row and the CSR's value bits, one 8-byte element
struct SparsePosting {
  int32_t row;
  float value;
};
static_assert(sizeof(SparsePosting) == 8, "a posting is 8 bytes");

// the digits the stable sort by column has to look at: the bits of dim - 1, at least one
inline int sparse_inv_key_bits(int64_t dim) {
  int bits = 1;
  while (bits < 31 && ((int64_t)1 << bits) < dim) ++bits;
  return bits;
}

// The stable sort by column: `passes` 8-bit LSD passes; in each, block b of `blocks` owns keys [b * chunk, (b + 1) * chunk) - consecutive chunks,
// so "block order, then position" is the order of the elements - and the [256 digits][blocks] table of a pass is scanned by one workgroup.
constexpr int64_t SPARSE_INV_SORT_BLOCKS = 1024;
struct SparseInvSortPlan {
  int passes;       // 1 .. 3: ceil(key bits / 8)
  int64_t blocks;   // 1 .. SPARSE_INV_SORT_BLOCKS
  int64_t chunk;    // a multiple of 256, blocks * chunk >= nnz, below 2^32 (a block counts its digits in 32 bits)
};
inline SparseInvSortPlan sparse_inv_sort_plan(int64_t nnz, int64_t dim) {
  SparseInvSortPlan p;
  p.passes = (sparse_inv_key_bits(dim) + 7) / 8;
  p.blocks = (nnz + 255) / 256;
  p.blocks = p.blocks < 1 ? 1 : (p.blocks < SPARSE_INV_SORT_BLOCKS ? p.blocks : SPARSE_INV_SORT_BLOCKS);
  p.chunk = ((nnz + p.blocks - 1) / p.blocks + 255) / 256 * 256;
  if (p.chunk < 256) p.chunk = 256;
  return p;
}
// keys [*begin, *end) of block b (those beyond the array: begin = end = nnz); the kernels call it too
EPS_AMONG_HD inline void sparse_inv_chunk(const SparseInvSortPlan& p, int64_t nnz, int64_t b, int64_t* begin, int64_t* end) {
  const int64_t at = b * p.chunk < nnz ? b * p.chunk : nnz;   // (b < 2^10, chunk < 2^32: no overflow)
  *begin = at;
  *end = nnz - at < p.chunk ? nnz : at + p.chunk;
}

struct SparseInvBytes {
  int64_t directory;   // col_offsets: 8 * (dim + 1)
  int64_t postings;    // 8 * nnz: what the image costs on top of the CSR, with the directory
  int64_t pairs;       // build scratch: the (row, value) pairs' other buffer, 8 * nnz
  int64_t keys_a;      // build scratch: the column keys after an odd pass, 4 * nnz (0 with one pass: the last pass writes no keys)
  int64_t keys_b;      // ... after an even pass, 4 * nnz (0 below three passes)
  int64_t table;       // build scratch: 8 * 256 * blocks
};
// false: dim or nnz outside what build_inverted serves (nothing was computed)
inline bool sparse_inv_bytes(int64_t dim, int64_t nnz, SparseInvBytes* b) {
  if (dim < 1 || dim > SPARSE_INV_MAX_DIM || nnz < 0 || nnz > SPARSE_INV_MAX_NNZ) return false;
  const SparseInvSortPlan p = sparse_inv_sort_plan(nnz, dim);
  b->directory = 8 * (dim + 1);
  b->postings = 8 * nnz;
  b->pairs = 8 * nnz;
  b->keys_a = p.passes >= 2 ? 4 * nnz : 0;
  b->keys_b = p.passes >= 3 ? 4 * nnz : 0;
  b->table = 8 * 256 * p.blocks;
  return true;
}
// workgroups of a build launch over `items` items, 256 threads each handling `per` of them per step
inline int64_t sparse_inv_build_blocks(int64_t items, int64_t per) {
  int64_t g = (items + per - 1) / per;
  g = g < 1 ? 1 : g;
  return g < SPARSE_INV_BUILD_BLOCKS ? g : SPARSE_INV_BUILD_BLOCKS;
}

struct SparseInvPlan {
  SparsePlan rows;        // nq_tile = 1, tiles = nq; W, rows_per_wave (a multiple of SPARSE_WAVE_ROWS) for sparse_wave_rows; qcap
  int64_t acc_offset;     // byte offset of the accumulators in dynamic LDS: qcap * 8 (the staged indices, then the staged values, in front)
  int64_t lds_dynamic;    // acc_offset + SPARSE_INV_ACC_BYTES
};
// n rows, nq queries of at most `longest_query` <= SPARSE_MAX_QUERY_NNZ non-zeros, 1 <= k <= SPARSE_MAX_K.  The scan's outer plan with one query
// per workgroup; a wavefront gets a whole tile of rows unless that leaves the chip short of workgroups, then half a tile, and so on down to 256.
inline SparseInvPlan sparse_inv_plan(int64_t n, int64_t nq, int32_t k, int64_t longest_query) {
  SparseInvPlan p;
  SparsePlan& r = p.rows;
  r.qcap = (longest_query + 3) / 4 * 4;
  if (r.qcap < 4) r.qcap = 4;
  r.nq_tile = 1;
  r.tiles = nq;
  r.lds_dynamic = r.qcap * 8;
  int64_t per_wave = SPARSE_INV_TILE_ROWS;
  const int64_t tiles = nq > 0 ? nq : 1;
  while (per_wave > 256 && (n + per_wave * SPARSE_BLOCK_WAVES - 1) / (per_wave * SPARSE_BLOCK_WAVES) * tiles < SPARSE_INV_MIN_BLOCKS) per_wave >>= 1;
  int64_t gx = (n + per_wave * SPARSE_BLOCK_WAVES - 1) / (per_wave * SPARSE_BLOCK_WAVES);
  int64_t cap = SPARSE_MAX_BLOCKS / tiles;   // many queries fill the chip by themselves
  const int64_t cap_merge = AMONG_MERGE_KEYS / ((int64_t)k * SPARSE_BLOCK_WAVES);   // launch_among_merge: W * k <= AMONG_MERGE_KEYS where W > 4
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  r.W = (int)(gx * SPARSE_BLOCK_WAVES);
  const int64_t per = (n + r.W - 1) / r.W;
  r.rows_per_wave = (per + SPARSE_WAVE_ROWS - 1) / SPARSE_WAVE_ROWS * SPARSE_WAVE_ROWS;
  if (r.rows_per_wave < SPARSE_WAVE_ROWS) r.rows_per_wave = SPARSE_WAVE_ROWS;
  p.acc_offset = r.qcap * 8;
  p.lds_dynamic = p.acc_offset + SPARSE_INV_ACC_BYTES;
  return p;
}
}  // namespace eps
