// Host side of the binary-vector index (eps_binary_index_*; kernels: binary.hip, host state: binary_index.cpp): the layout of a packed row, the
// limits, the argument refusals and the launch plan of the scan - the (NQ, KPL) form, the row slices, the grid and the scratch it needs.  Plain
// C++ with no device type in it: tests/native/binary_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"
#include "among_host.hpp"

namespace eps {

constexpr int BIN_CW = 8;                                   // words of a row a lane holds at once: the chunk of the scan (two 16-byte loads)
constexpr int64_t BIN_MAX_DIM = 65536;                      // bits of a vector: a distance fits 17 bits
constexpr int32_t BIN_MAX_K = 1024;                         // the widest WaveTopK (KPL = 16)
constexpr int64_t BIN_MAX_ROWS = ((int64_t)1 << 31) - 1;    // rows of one table (a key carries a 32-bit row)
constexpr int BIN_WAVE_ROWS = 64;                           // rows of one round of a wavefront: one per lane
constexpr int BIN_BLOCK_WAVES = 4;                          // wavefronts of a scan workgroup, each with a slice of its own
constexpr int BIN_TILE_BUDGET = 32;                         // NQ * KPL of a form: its lists cost 2 * NQ * KPL registers per lane
constexpr int BIN_MIN_TILE = 4;                             // the narrowest query tile (KPL = 16 keeps it: 128 list registers)
constexpr int64_t BIN_MAX_BLOCKS = 2048;                    // scan workgroups of one pass over the table times query tiles
constexpr int64_t BIN_GRID_Y = 32768;                       // query tiles of one launch; longer batches run in slices
constexpr int64_t BIN_MERGE_KEYS = (int64_t)1 << 18;        // partial keys per query the merge's one workgroup is given at most

EPS_AMONG_HD inline int64_t binary_words(int64_t dim) { return (dim + 31) / 32; }   // W
// bits of the LAST word that belong to the vector: bit j of a vector is bit j % 32 of word j / 32, the rest of the last word is ignored
inline uint32_t binary_tail_mask(int64_t dim) { return (dim & 31) ? (((uint32_t)1 << (dim & 31)) - 1u) : 0xFFFFFFFFu; }
// the stride of a bit table the handle owns: rows of four words and more start on 16 bytes, so that the scan reads them in 16-byte pieces
inline int64_t binary_owned_stride(int64_t W) { return W < 4 ? W : (W + 3) / 4 * 4; }

// why a call is refused, or null
inline const char* binary_create_refusal(int64_t dim) { return dim < 1 || dim > BIN_MAX_DIM ? "dim must be in [1, 65536]" : nullptr; }
inline const char* binary_attach_refusal(int64_t dim, const void* words, int64_t n, int64_t stride_words) {
  if (n < 0) return "n must be >= 0";
  if (n > BIN_MAX_ROWS) return "more than 2^31 - 1 rows per index";
  if (n > 0 && !words) return "null buffer";
  if (n > 0 && stride_words < binary_words(dim)) return "stride_words must be >= ceil(dim / 32)";
  return nullptr;
}
inline const char* binary_search_refusal(int64_t nq, int32_t k) {
  if (k < 1 || k > BIN_MAX_K) return "k must be in [1, 1024]";
  if (nq < 0) return "nq must be >= 0";
  if (nq > BIN_MAX_ROWS) return "more than 2^31 - 1 queries";
  return nullptr;
}

struct BinaryPlan {
  int kpl;                  // 64-entry registers per lane of a list: 1, 2, 4, 8 or 16
  int nq_tile;              // NQ: queries of a workgroup - 4, 8, 16 or 32, NQ * KPL <= BIN_TILE_BUDGET (KPL = 16: 4)
  int64_t tiles;            // query tiles over the whole batch (launched in slices of BIN_GRID_Y)
  int64_t launches;         // scan launches
  int64_t slices;           // row slices = wavefronts in x = partial lists per query, a multiple of BIN_BLOCK_WAVES
  int64_t rows_per_slice;   // a multiple of BIN_WAVE_ROWS: slice s takes rows [s * rows_per_slice, (s + 1) * rows_per_slice) of the table
  int64_t partial_bytes;    // nq * slices * k keys of 8 bytes
  int64_t run_bytes;        // nq * k keys
};
// the k-lists of the scan: ceil(k / 64) rounded up to a power of two
inline int binary_kpl(int32_t k) { return k <= 64 ? 1 : k <= 128 ? 2 : k <= 256 ? 4 : k <= 512 ? 8 : 16; }
// the narrowest tile of {4, 8, 16, 32} that holds the batch, within the form's register budget.  k <= 64 and 32 queries or more: a 32-query tile,
// the table read once per 32 queries
inline int binary_tile(int64_t nq, int kpl) {
  int cap = BIN_TILE_BUDGET / kpl;
  cap = cap < BIN_MIN_TILE ? BIN_MIN_TILE : cap;
  int t = BIN_MIN_TILE;
  while (t < cap && t < nq) t <<= 1;
  return t;
}
// n rows, nq >= 1 queries, 1 <= k <= BIN_MAX_K
inline BinaryPlan binary_plan(int64_t n, int64_t nq, int32_t k) {
  BinaryPlan p;
  p.kpl = binary_kpl(k);
  p.nq_tile = binary_tile(nq, p.kpl);
  p.tiles = (nq + p.nq_tile - 1) / p.nq_tile;
  p.launches = (p.tiles + BIN_GRID_Y - 1) / BIN_GRID_Y;
  const int64_t block_rows = (int64_t)BIN_WAVE_ROWS * BIN_BLOCK_WAVES;
  int64_t gx = (n + block_rows - 1) / block_rows;                 // at least one round per wavefront
  int64_t cap = BIN_MAX_BLOCKS / (p.tiles > 0 ? p.tiles : 1);     // many tiles fill the chip by themselves
  const int64_t cap_merge = BIN_MERGE_KEYS / ((int64_t)k * BIN_BLOCK_WAVES);
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  p.slices = gx * BIN_BLOCK_WAVES;
  const int64_t per = (n + p.slices - 1) / p.slices;
  p.rows_per_slice = (per + BIN_WAVE_ROWS - 1) / BIN_WAVE_ROWS * BIN_WAVE_ROWS;
  if (p.rows_per_slice < BIN_WAVE_ROWS) p.rows_per_slice = BIN_WAVE_ROWS;
  p.partial_bytes = nq * p.slices * k * 8;
  p.run_bytes = nq * k * 8;
  return p;
}
// rows [*begin, *end) of slice s (those beyond the table: begin = end = n); the kernel calls it too
EPS_AMONG_HD inline void binary_slice_rows(const BinaryPlan& p, int64_t n, int64_t s, int64_t* begin, int64_t* end) {
  const int64_t b = s * p.rows_per_slice < n ? s * p.rows_per_slice : n;   // (s < 2^13, rows_per_slice < 2^31: no overflow)
  *begin = b;
  *end = n - b < p.rows_per_slice ? n : b + p.rows_per_slice;
}

}  // namespace eps
