// Host side of the byte-vector index (eps_byte_index_*; kernels: byte.hip, host state: byte_index.cpp): the stored form of a row of bytes, the
// integer terms that turn a matrix-core dot product into the exact distance, the limits, the argument refusals and the launch plan of the scan -
// the (NB, KPL) form, the live columns of a query tile, the row slices, the grid, the LDS and the scratch it needs.  Plain C++ with no device type
// in it: tests/native/byte_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"
#include "among_host.hpp"
#include "binary_host.hpp"

namespace eps {

constexpr int64_t BYTE_MAX_DIM = 4096;                      // 255^2 * 4096 < 2^31: every distance is an int32
constexpr int32_t BYTE_MAX_K = 1024;                        // the widest WaveTopK (KPL = 16)
constexpr int64_t BYTE_MAX_ROWS = ((int64_t)1 << 31) - 1;   // rows of one table (a key carries a 32-bit row)
constexpr int BYTE_KSTEP = 64;                              // bytes of K of one v_mfma_i32_16x16x64_i8; stored rows are padded to a multiple
constexpr int BYTE_WAVE_ROWS = 64;                          // rows of one round of a wavefront: four 16-row blocks
constexpr int BYTE_BLOCK_WAVES = 4;                         // wavefronts of a scan workgroup, each with a slice of its own
constexpr int BYTE_LIST_BUDGET = 64;                        // lists of a wavefront x KPL: 2 registers per lane each
constexpr int BYTE_LDS_QUERY_BYTES = 65536;                 // operands of a query tile in LDS: columns * d_pad bytes
constexpr int64_t BYTE_MAX_BLOCKS = 2048;                   // scan workgroups of one pass over the table times query tiles
constexpr int64_t BYTE_MERGE_KEYS = (int64_t)1 << 18;       // partial keys per query the merge's one workgroup is given at most

// bytes of a stored row: whole K-steps, so that every operand load is a whole 16-byte piece
EPS_AMONG_HD inline int64_t byte_pad(int64_t dim) { return (dim + BYTE_KSTEP - 1) / BYTE_KSTEP * BYTE_KSTEP; }
// rows of the stored table: whole rounds, so that no operand load of a round needs a bound (the rows behind n are zeros and are never offered)
inline int64_t byte_pad_rows(int64_t n) { return (n + BYTE_WAVE_ROWS - 1) / BYTE_WAVE_ROWS * BYTE_WAVE_ROWS; }

// The stored value x' of a byte: a signed byte is itself; an unsigned byte b is kept as b ^ 0x80, the int8 b - 128.  Pad bytes are 0 in the stored
// domain.  With dot' = sum x' q' (what the matrix cores return, exactly) the distance is  row_term + query_term + s * dot':
//   EUCLIDEAN    sum (x - q)^2 = sum (x' - q')^2 (the shift cancels) = sum x'^2 + sum q'^2 - 2 dot':     s = -2, both terms sum v'^2
//   DOT_PRODUCT  signed:   -sum x q = -dot':                                                               s = -1, both terms 0
//                unsigned: x = x' + 128, q = q' + 128: x.q = dot' + 128 sum x' + 128 sum q' + 16384 dim, so
//                -x.q = (-128 sum x') + (-128 sum q' - 16384 dim) - dot':                                   s = -1
// The sums run over the dim real bytes only.  |term| <= 2^27 and |dot'| <= 2^26: no int32 step of the sum overflows.
EPS_AMONG_HD inline int32_t byte_stored(uint8_t b, int is_unsigned) { return (int32_t)(int8_t)(is_unsigned ? b ^ 0x80u : b); }
// sum1 = sum v', sum2 = sum v'^2 of a row (is_query = 0) or of a query (1)
EPS_AMONG_HD inline int32_t byte_term(int metric, int is_unsigned, int is_query, int32_t sum1, int32_t sum2, int64_t dim) {
  if (metric == EPS_METRIC_EUCLIDEAN) return sum2;
  if (!is_unsigned) return 0;
  return -128 * sum1 - (is_query ? (int32_t)(16384 * dim) : 0);
}
// dot' enters the distance as -(dot' << shift)
EPS_AMONG_HD inline int byte_dot_shift(int metric) { return metric == EPS_METRIC_EUCLIDEAN ? 1 : 0; }

// why a call is refused, or null
inline const char* byte_create_refusal(int64_t dim, int32_t metric) {
  if (dim < 1 || dim > BYTE_MAX_DIM) return "dim must be in [1, 4096]";
  if (metric == EPS_METRIC_COSINE) return "COSINE is not an integer rule: byte fields serve EUCLIDEAN and DOT_PRODUCT";
  if (metric != EPS_METRIC_EUCLIDEAN && metric != EPS_METRIC_DOT_PRODUCT) return "unknown metric";
  return nullptr;
}
inline const char* byte_attach_refusal(int64_t dim, const void* bytes, int64_t n, int64_t stride_bytes) {
  if (n < 0) return "n must be >= 0";
  if (n > BYTE_MAX_ROWS) return "more than 2^31 - 1 rows per index";
  if (n > 0 && !bytes) return "null buffer";
  if (n > 0 && stride_bytes < dim) return "stride_bytes must be >= dim";
  return nullptr;
}
inline const char* byte_search_refusal(int64_t nq, int32_t k) {
  if (k < 1 || k > BYTE_MAX_K) return "k must be in [1, 1024]";
  if (nq < 0) return "nq must be >= 0";
  if (nq > BYTE_MAX_ROWS) return "more than 2^31 - 1 queries";
  return nullptr;
}

struct BytePlan {
  int kpl;                  // 64-entry registers per lane of a list: binary_kpl(k)
  int nb;                   // NB: 16-column blocks of a query tile, 1 or 2
  int cols;                 // live columns of a tile = lists of a wavefront: min(16 NB, 64 / KPL); the other columns of a block are zero operands
  int64_t tiles;            // query tiles over the whole batch (launched in slices of BIN_GRID_Y)
  int64_t launches;         // scan launches
  int64_t slices;           // row slices = wavefronts in x = partial lists per query, a multiple of BYTE_BLOCK_WAVES
  int64_t rows_per_slice;   // a multiple of BYTE_WAVE_ROWS: slice s takes rows [s * rows_per_slice, (s + 1) * rows_per_slice) of the table
  int64_t rounds;           // rounds of 64 rows all wavefronts of all tiles walk together
  int64_t lds_bytes;        // dynamic LDS of a workgroup: the tile's operands and four patches
  int64_t partial_bytes;    // nq * slices * k keys of 8 bytes
  int64_t run_bytes;        // nq * k keys
};
// int32 entries between two rows of a wavefront's patch [64 rows][16 NB columns]: 16 NB + 4.  Four times the pitch is 16 modulo 64, so the 64
// lanes of a transposing store (16 columns x 4 row groups) fall into 64 different banks
EPS_AMONG_HD inline int byte_patch_pitch(int nb) { return 16 * nb + 4; }
inline int64_t byte_lds_bytes(int nb, int64_t d_pad) {
  return (int64_t)nb * 16 * d_pad + (int64_t)BYTE_BLOCK_WAVES * BYTE_WAVE_ROWS * byte_patch_pitch(nb) * 4;
}
// Two column blocks need two things: k <= 64 (32 lists of one register pair each) and both blocks' operands within 64 KB of LDS (d_pad <= 2048).
// A batch of 16 queries and fewer never needs the second block.
inline int byte_blocks(int64_t nq, int kpl, int64_t d_pad) { return kpl == 1 && nq > 16 && 32 * d_pad <= BYTE_LDS_QUERY_BYTES ? 2 : 1; }
// n rows, nq >= 1 queries, 1 <= k <= BYTE_MAX_K.  The caps are binary_plan's: the workgroups of a pass over the table divided by the number of
// tiles, and the merge's key cap.  Fewer, longer slices also make the scan's common path more common: a list's threshold starts open in every
// slice, and only a round whose 64 rows all lie above every column's k-th distance ends at the vote.
inline BytePlan byte_plan(int64_t n, int64_t dim, int64_t nq, int32_t k) {
  BytePlan p;
  const int64_t d_pad = byte_pad(dim);
  p.kpl = binary_kpl(k);
  p.nb = byte_blocks(nq, p.kpl, d_pad);
  p.cols = BYTE_LIST_BUDGET / p.kpl < 16 * p.nb ? BYTE_LIST_BUDGET / p.kpl : 16 * p.nb;
  p.tiles = (nq + p.cols - 1) / p.cols;
  p.launches = (p.tiles + BIN_GRID_Y - 1) / BIN_GRID_Y;
  const int64_t block_rows = (int64_t)BYTE_WAVE_ROWS * BYTE_BLOCK_WAVES;
  int64_t gx = (n + block_rows - 1) / block_rows;                  // at least one round per wavefront
  int64_t cap = BYTE_MAX_BLOCKS / (p.tiles > 0 ? p.tiles : 1);     // many tiles fill the chip by themselves
  const int64_t cap_merge = BYTE_MERGE_KEYS / ((int64_t)k * BYTE_BLOCK_WAVES);
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  p.slices = gx * BYTE_BLOCK_WAVES;
  const int64_t per = (n + p.slices - 1) / p.slices;
  p.rows_per_slice = (per + BYTE_WAVE_ROWS - 1) / BYTE_WAVE_ROWS * BYTE_WAVE_ROWS;
  if (p.rows_per_slice < BYTE_WAVE_ROWS) p.rows_per_slice = BYTE_WAVE_ROWS;
  p.rounds = byte_pad_rows(n) / BYTE_WAVE_ROWS * p.tiles;          // (every slice but the last non-empty one is whole rounds)
  p.lds_bytes = byte_lds_bytes(p.nb, d_pad);
  p.partial_bytes = nq * p.slices * k * 8;
  p.run_bytes = nq * k * 8;
  return p;
}
// rows [*begin, *end) of slice s (those beyond the table: begin = end = n); the kernel calls it too.  binary_slice_rows' scheme
EPS_AMONG_HD inline void byte_slice_rows(int64_t rows_per_slice, int64_t n, int64_t s, int64_t* begin, int64_t* end) {
  const int64_t b = s * rows_per_slice < n ? s * rows_per_slice : n;   // (s < 2^13, rows_per_slice < 2^31: no overflow)
  *begin = b;
  *end = n - b < rows_per_slice ? n : b + rows_per_slice;
}

}  // namespace eps
