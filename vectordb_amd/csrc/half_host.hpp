// Host side of the half-vector index (eps_half_index_*; kernels: half.hip, host state: half_index.cpp): the stored form of a row of fp16 / bf16
// elements, the float -> half rounding, the limits, the argument refusals, the launch plan of the scan - the (NB, KPL) form, the live columns of a
// query tile, the row slices, the grid, the LDS and the scratch it needs - and the rule that decides whether a call seeds its thresholds from a
// prefix of the table.  Plain C++ with no device type in it: tests/native/half_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"
#include "among_host.hpp"
#include "binary_host.hpp"

namespace eps {

constexpr int64_t HALF_MAX_DIM = 4096;                      // 16 columns of the longest row fill the 128 KB of a query tile
constexpr int32_t HALF_MAX_K = 1024;                        // the widest WaveTopK (KPL = 16)
constexpr int64_t HALF_MAX_ROWS = ((int64_t)1 << 31) - 1;   // rows of one table (a key carries a 32-bit row)
constexpr int HALF_KSTEP = 32;                              // elements of K of one v_mfma_f32_16x16x32_f16 / _bf16; stored rows are padded to a multiple
constexpr int HALF_WAVE_ROWS = 64;                          // rows of one round of a wavefront: four 16-row blocks
constexpr int HALF_BLOCK_WAVES = 4;                         // wavefronts of a scan workgroup, each with a slice of its own
constexpr int HALF_LIST_BUDGET = 64;                        // lists of a wavefront x KPL: 2 registers per lane each
constexpr int HALF_LDS_QUERY_BYTES = 131072;                // operands of a query tile in LDS: columns * d_pad * 2 bytes
constexpr int HALF_PATCH_PITCH = 20;                        // fp32 entries between two rows of a wavefront's patch [64 rows][16 columns]: 4 * 20 = 16 mod 64,
                                                            // so the 64 lanes of a transposing store (16 columns x 4 row groups) fall into 64 banks
constexpr int64_t HALF_MAX_BLOCKS = 2048;                   // scan workgroups of one pass over the table times query tiles
constexpr int64_t HALF_MERGE_KEYS = (int64_t)1 << 18;       // partial keys per query the merge's one workgroup is given at most
constexpr int64_t HALF_SEED_MIN_ROWS = 32768;               // the shortest table whose thresholds are seeded (half_seed_rows)
constexpr uint32_t HALF_BOUND_OPEN = 0xFFFFFFFFu;           // a threshold that every key passes (the high word of KEY_EMPTY)

// elements of a stored row: whole K-steps, so that every operand load is a whole 16-byte piece
EPS_AMONG_HD inline int64_t half_pad(int64_t dim) { return (dim + HALF_KSTEP - 1) / HALF_KSTEP * HALF_KSTEP; }
// rows of the stored table: whole rounds, so that no operand load of a round needs a bound (the rows behind n are zeros and are never offered)
inline int64_t half_pad_rows(int64_t n) { return (n + HALF_WAVE_ROWS - 1) / HALF_WAVE_ROWS * HALF_WAVE_ROWS; }
// HBM of the stored table
inline int64_t half_table_bytes(int64_t n, int64_t dim) { return half_pad_rows(n) * (2 * half_pad(dim) + 4); }

// ---- float -> half, round to nearest even, on the bits (the device runs these very lines: half_convert_kernel, half_prepare_kernel).
// fp16: 1 + 5 + 10 bits; a NaN stays a NaN (its top payload bits kept, never the infinity's pattern), |x| >= 65520 goes to infinity, results
// below 2^-14 are subnormal halves.  bf16: the float's upper half, a NaN quietened.
EPS_AMONG_HD inline uint16_t half_from_float_bits(uint32_t u, int is_bf16) {
  const uint32_t a = u & 0x7FFFFFFFu;
  if (is_bf16) {
    if (a > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  }
  const uint32_t sign = (u >> 16) & 0x8000u;
  if (a > 0x7F800000u) {
    const uint32_t m = (a >> 13) & 0x3FFu;
    return (uint16_t)(sign | 0x7C00u | (m ? m : 1u));
  }
  if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);   // 65520 and above, the infinity included
  uint32_t q, rem, half;
  if (a < 0x38800000u) {                                     // below 2^-14: units of 2^-24
    const uint32_t e = a >> 23;
    if (e < 102u) return (uint16_t)sign;                     // below 2^-25 (2^-25 itself: e = 102, a tie that goes to the even 0 below)
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, s = 126u - e;   // 14 <= s <= 24
    q = m >> s;
    rem = m & ((1u << s) - 1u);
    half = 1u << (s - 1u);
  } else {
    const uint32_t b = a - 0x38000000u;                      // exponent rebiased from 127 to 15
    q = b >> 13;
    rem = b & 0x1FFFu;
    half = 0x1000u;
  }
  if (rem > half || (rem == half && (q & 1u))) ++q;          // (a carry runs into the exponent: the next binade, or 0x7C00)
  return (uint16_t)(sign | q);
}
// half -> float, exact
EPS_AMONG_HD inline uint32_t half_to_float_bits(uint16_t h, int is_bf16) {
  if (is_bf16) return (uint32_t)h << 16;
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu;
  uint32_t m = h & 0x3FFu;
  if (e == 0x1Fu) return sign | 0x7F800000u | (m << 13);
  if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
  if (m == 0u) return sign;
  uint32_t x = 113u;                                         // a subnormal half: m * 2^-24, normalised
  while (!(m & 0x400u)) {
    m <<= 1;
    --x;
  }
  return sign | (x << 23) | ((m & 0x3FFu) << 13);
}

// why a call is refused, or null
inline const char* half_create_refusal(int64_t dim, int32_t metric) {
  if (dim < 1 || dim > HALF_MAX_DIM) return "dim must be in [1, 4096]";
  if (metric != EPS_METRIC_EUCLIDEAN && metric != EPS_METRIC_COSINE && metric != EPS_METRIC_DOT_PRODUCT) return "unknown metric";
  return nullptr;
}
inline const char* half_attach_refusal(int64_t dim, const void* rows, int64_t n, int64_t stride_elems) {
  if (n < 0) return "n must be >= 0";
  if (n > HALF_MAX_ROWS) return "more than 2^31 - 1 rows per index";
  if (n > 0 && !rows) return "null buffer";
  if (n > 0 && stride_elems < dim) return "stride_elems must be >= dim";
  return nullptr;
}
inline const char* half_search_refusal(int64_t nq, int32_t k) {
  if (k < 1 || k > HALF_MAX_K) return "k must be in [1, 1024]";
  if (nq < 0) return "nq must be >= 0";
  if (nq > HALF_MAX_ROWS) return "more than 2^31 - 1 queries";
  return nullptr;
}

struct HalfPlan {
  int kpl;                  // 64-entry registers per lane of a list: binary_kpl(k)
  int nb;                   // NB: 16-column blocks of a query tile, 1, 2 or 4
  int cols;                 // live columns of a tile = lists of a wavefront: min(16 NB, 64 / KPL); the other columns of a block are zero operands
  int64_t tiles;            // query tiles over the whole batch (launched in slices of BIN_GRID_Y)
  int64_t launches;         // scan launches of one pass
  int64_t slices;           // row slices = wavefronts in x = partial lists per query, a multiple of HALF_BLOCK_WAVES
  int64_t rows_per_slice;   // a multiple of HALF_WAVE_ROWS: slice s takes rows [s * rows_per_slice, (s + 1) * rows_per_slice) of the table
  int64_t rounds;           // rounds of 64 rows all wavefronts of all tiles walk together
  int64_t lds_bytes;        // dynamic LDS of a workgroup: the tile's operands and four patches
  int64_t partial_bytes;    // nq * slices * k keys of 8 bytes
  int64_t run_bytes;        // nq * k keys
};
inline int64_t half_lds_bytes(int nb, int64_t d_pad) {
  return (int64_t)nb * 16 * d_pad * 2 + (int64_t)HALF_BLOCK_WAVES * HALF_WAVE_ROWS * HALF_PATCH_PITCH * 4;
}
// The widest tile of {1, 2, 4} column blocks that the lists' registers (64 / KPL columns), the tile's 128 KB of LDS (16 NB d_pad elements) and the
// batch itself (no block without a query) allow: 4 up to d_pad = 1024 and k <= 64, 2 up to d_pad = 2048 and k <= 128, else 1
inline int half_blocks(int64_t nq, int kpl, int64_t d_pad) {
  int nb = 4;
  while (nb > 1 && (16 * nb > HALF_LIST_BUDGET / kpl || (int64_t)nb * 32 * d_pad > HALF_LDS_QUERY_BYTES || nq <= 16 * (nb / 2))) nb >>= 1;
  return nb;
}
// n rows, nq >= 1 queries, 1 <= k <= HALF_MAX_K.  The caps are binary_plan's: the workgroups of a pass over the table divided by the number of
// tiles, and the merge's key cap
inline HalfPlan half_plan(int64_t n, int64_t dim, int64_t nq, int32_t k) {
  HalfPlan p;
  const int64_t d_pad = half_pad(dim);
  p.kpl = binary_kpl(k);
  p.nb = half_blocks(nq, p.kpl, d_pad);
  p.cols = HALF_LIST_BUDGET / p.kpl < 16 * p.nb ? HALF_LIST_BUDGET / p.kpl : 16 * p.nb;
  p.tiles = (nq + p.cols - 1) / p.cols;
  p.launches = (p.tiles + BIN_GRID_Y - 1) / BIN_GRID_Y;
  const int64_t block_rows = (int64_t)HALF_WAVE_ROWS * HALF_BLOCK_WAVES;
  int64_t gx = (n + block_rows - 1) / block_rows;                  // at least one round per wavefront
  int64_t cap = HALF_MAX_BLOCKS / (p.tiles > 0 ? p.tiles : 1);     // many tiles fill the chip by themselves
  const int64_t cap_merge = HALF_MERGE_KEYS / ((int64_t)k * HALF_BLOCK_WAVES);
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  p.slices = gx * HALF_BLOCK_WAVES;
  const int64_t per = (n + p.slices - 1) / p.slices;
  p.rows_per_slice = (per + HALF_WAVE_ROWS - 1) / HALF_WAVE_ROWS * HALF_WAVE_ROWS;
  if (p.rows_per_slice < HALF_WAVE_ROWS) p.rows_per_slice = HALF_WAVE_ROWS;
  p.rounds = half_pad_rows(n) / HALF_WAVE_ROWS * p.tiles;          // (every slice but the last non-empty one is whole rounds)
  p.lds_bytes = half_lds_bytes(p.nb, d_pad);
  p.partial_bytes = nq * p.slices * k * 8;
  p.run_bytes = nq * k * 8;
  return p;
}
// rows [*begin, *end) of slice s (those beyond the table: begin = end = n); the kernel calls it too.  binary_slice_rows' scheme
EPS_AMONG_HD inline void half_slice_rows(int64_t rows_per_slice, int64_t n, int64_t s, int64_t* begin, int64_t* end) {
  const int64_t b = s * rows_per_slice < n ? s * rows_per_slice : n;   // (s < 2^13, rows_per_slice < 2^31: no overflow)
  *begin = b;
  *end = n - b < rows_per_slice ? n : b + rows_per_slice;
}

// The seed rule: rows of the prefix whose k-th distance opens every slice's threshold, or 0 - the call is not seeded and every slice starts open.
// A slice of an unseeded scan fills its own list from nothing, so on a long table cut into thousands of short slices nearly every round takes the
// hit path.  The prefix costs prefix / n of a pass and leaves about k n / prefix rows of the table under the seed, per query.  A sixteenth of the
// table, at least 4096 rows and 8 k rows (a list must be able to fill), in whole workgroup passes of 256 rows; tables below 32768 rows are not
// seeded: their slices are few, and the prefix would be a large part of them.  Every k and every batch is seeded alike
inline int64_t half_seed_rows(int64_t n, int64_t dim, int64_t nq, int32_t k) {
  (void)dim;
  (void)nq;
  if (n < HALF_SEED_MIN_ROWS) return 0;
  int64_t p = n / 16;
  p = p < 4096 ? 4096 : p;
  p = p < 8 * (int64_t)k ? 8 * (int64_t)k : p;
  return (p + 255) / 256 * 256;   // (<= n / 2: n >= 32768, k <= 1024)
}

}  // namespace eps
