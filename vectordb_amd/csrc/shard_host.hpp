// Host arithmetic of the hash-sharded index (eps_index_create_sharded; shard_group.cpp): which rows, bits, column values and attribute rows of the
// caller's memory belong to shard s of G, where an append's rows go, how the gathered per-shard lists are laid out and how counts are read off a
// merged id list.  Plain C++ with no HIP type in it: shard_group.cpp slices the caller's buffers through these functions and nothing else, and
// tests/native/shard_host_check.cpp runs the same functions under a sanitizer against buffers of exactly the size the ABI demands.
//
// The split: global row i lives on shard i mod G as local row i / G; local row l of shard s is global row l * G + s.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace eps {

// rows of an n-row table that shard s of G holds: #{i < n : i mod G == s}
inline int64_t shard_rows_of(int s, int64_t n, int G) { return n > s ? (n - s + G - 1) / G : 0; }

// the global row of local row l of shard s
inline int64_t shard_global_row(int64_t l, int s, int G) { return l * G + s; }

// An append of n_new rows to a table of n0 rows: row n0 + j goes to shard (n0 + j) mod G.  Shard s takes the rows j = first, first + G, ... of the
// appended block, `count` of them (first is meaningless when count == 0).
struct ShardSpan {
  int64_t first, count;
};
inline ShardSpan shard_append_span(int s, int64_t n0, int64_t n_new, int G) {
  const int64_t first = ((s - n0) % G + G) % G;   // the first j with (n0 + j) mod G == s
  return ShardSpan{first, n_new > first ? (n_new - first + G - 1) / G : 0};
}

// float rows of `dim` values: the block's row `first` and every G-th row after it
struct ShardRowsView {
  const float* base;
  int64_t pitch;   // floats
};
inline ShardRowsView shard_rows_view(const float* rows, int64_t dim, int64_t first, int G) { return ShardRowsView{rows + first * dim, (int64_t)G * dim}; }

// The deleted bitset (bit i of byte i / 8, least significant bit first) of an n-row table, de-interleaved: bit l of `out` = bit l * G + s of `bits`.
// out holds (shard_rows_of(s, n, G) + 7) / 8 bytes, all written; bits beyond the shard's rows are zero.  Reads bits [0, n) only.
inline void shard_split_bits(const uint8_t* bits, int64_t n, int s, int G, uint8_t* out) {
  const int64_t ns = shard_rows_of(s, n, G);
  for (int64_t b = 0; b < (ns + 7) / 8; ++b) out[b] = 0;
  for (int64_t l = 0; l < ns; ++l) {
    const int64_t i = shard_global_row(l, s, G);
    if ((bits[i >> 3] >> (i & 7)) & 1) out[l >> 3] |= uint8_t(1u << (l & 7));
  }
}

// whether any of the first nbytes bytes of a bitset is non-zero (what Index::set_deleted asks of the table's live bytes)
inline bool shard_any_byte(const uint8_t* bits, int64_t nbytes) {
  for (int64_t b = 0; b < nbytes; ++b)
    if (bits[b]) return true;
  return false;
}

// A filter column (row i's value at column + i * stride): the shard's rows are every G-th value of the same memory.
struct ShardColumnView {
  const char* base;
  int64_t stride;
};
inline ShardColumnView shard_column_view(const void* column, int64_t stride, int s, int G) {
  return ShardColumnView{static_cast<const char*>(column) + (int64_t)s * stride, stride * G};
}

// Packed attribute rows (row i at rows + i * stride, n_rows of them): the shard's `count` rows start at base and lie `pitch` bytes apart; row_bytes of
// each are the row (they are uploaded packed at row_bytes).
struct ShardAttrView {
  const char* base;
  int64_t pitch, row_bytes, count;
};
inline ShardAttrView shard_attr_view(const void* rows, int64_t stride, int64_t n_rows, int s, int G) {
  return ShardAttrView{static_cast<const char*>(rows) + (int64_t)s * stride, stride * G, stride, shard_rows_of(s, n_rows, G)};
}

// Bytes from one shard's gathered lists to the next's: [ids int64[nq * k] | dist f32[nq * k]] rounded up to 8 (the layout eps_merge_topk_packed takes).
inline size_t shard_gather_stride(int64_t nq, int k) { return ((size_t)nq * (size_t)k * 12 + 7) / 8 * 8; }

// counts[q] = the number of rows in query q's merged list.  Mirrors merge_shards_kernel (flat_kernels.hip), which counts `++found` once per slot it
// fills with a row and writes -1 into every slot after the shards ran dry: the rows are exactly the prefix of ids >= 0.
inline void shard_counts_from_ids(const int64_t* ids, int64_t nq, int k, int32_t* counts) {
  for (int64_t q = 0; q < nq; ++q) {
    int32_t c = 0;
    while (c < k && ids[q * k + c] >= 0) ++c;
    counts[q] = c;
  }
}

}  // namespace eps
