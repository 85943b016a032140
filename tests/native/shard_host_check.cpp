// Stand-alone host check of csrc/shard_host.hpp - the arithmetic by which the shard group (csrc/shard_group.cpp) slices the caller's rows, deleted
// bitset, filter column and attribute rows per shard, splits an append, lays out the gathered lists and reads counts off a merged list - for a CPU
// build under -fsanitize=address,undefined (tests/test_shard_ref_cpu.py builds and runs it).  Every caller buffer lives on the heap at EXACTLY the
// minimum size the ABI demands, and every byte a view addresses is read with memcpy, as the shards' uploads read it: an off-by-one is a heap overflow
// the sanitizer reports.  Brute force over G = 1..16, n = 0..200, appends from n0 = 0..40 of 0..40 rows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vectordb_amd/csrc/shard_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (failures < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                             \
    }                                                         \
  } while (0)

// a heap block of exactly `bytes` bytes (never the one-byte block malloc(0) may share with nothing to guard)
struct Block {
  unsigned char* p;
  size_t bytes;
  explicit Block(size_t b) : p(static_cast<unsigned char*>(malloc(b ? b : 1))), bytes(b) {}
  ~Block() { free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

// every global row on exactly one shard, at local index i / G; the shards' row counts add up
static void split(int G, int64_t n) {
  std::vector<int64_t> seen((size_t)n, 0);
  int64_t total = 0;
  for (int s = 0; s < G; ++s) {
    const int64_t ns = eps::shard_rows_of(s, n, G);
    total += ns;
    for (int64_t l = 0; l < ns; ++l) {
      const int64_t i = eps::shard_global_row(l, s, G);
      CHECK(i >= 0 && i < n);
      if (i < 0 || i >= n) continue;
      CHECK(i % G == s && i / G == l);
      ++seen[(size_t)i];
    }
    CHECK(ns == 0 || eps::shard_global_row(ns - 1, s, G) < n);
    CHECK(eps::shard_global_row(ns, s, G) >= n);   // (the next local row would lie beyond the table)
  }
  CHECK(total == n);
  for (int64_t i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
}

// the float rows: every shard reads its rows out of a table of exactly n * dim floats; row l of shard s is global row l * G + s
static void rows(int G, int64_t n, int64_t dim) {
  Block t((size_t)(n * dim) * sizeof(float));
  for (int64_t i = 0; i < n * dim; ++i) {
    const float v = (float)i;
    memcpy(t.p + i * 4, &v, 4);
  }
  for (int s = 0; s < G; ++s) {
    const eps::ShardRowsView v = eps::shard_rows_view(reinterpret_cast<const float*>(t.p), dim, s, G);
    const int64_t ns = eps::shard_rows_of(s, n, G);
    std::vector<float> row((size_t)dim);
    for (int64_t l = 0; l < ns; ++l) {
      memcpy(row.data(), v.base + l * v.pitch, (size_t)dim * 4);
      CHECK(row[0] == (float)((l * G + s) * dim) && row[(size_t)dim - 1] == (float)((l * G + s) * dim + dim - 1));
    }
  }
}

// consecutive appends tile every shard's rows with no gap or overlap: after a table of n0 rows, an append of n_new rows hands shard s exactly its
// local rows [rows_of(n0), rows_of(n0 + n_new)), in order, read out of a block of exactly n_new * dim floats
static void append(int G, int64_t n0, int64_t n_new) {
  const int64_t dim = 3;
  Block blk((size_t)(n_new * dim) * sizeof(float));
  for (int64_t j = 0; j < n_new * dim; ++j) {
    const float v = (float)(n0 * dim + j);
    memcpy(blk.p + j * 4, &v, 4);
  }
  int64_t total = 0;
  for (int s = 0; s < G; ++s) {
    const eps::ShardSpan a = eps::shard_append_span(s, n0, n_new, G);
    const int64_t before = eps::shard_rows_of(s, n0, G), after = eps::shard_rows_of(s, n0 + n_new, G);
    CHECK(a.count == after - before);
    CHECK(a.first >= 0 && a.first < G);
    total += a.count;
    if (!a.count) continue;
    const eps::ShardRowsView v = eps::shard_rows_view(reinterpret_cast<const float*>(blk.p), dim, a.first, G);
    for (int64_t c = 0; c < a.count; ++c) {
      float row[3];
      memcpy(row, v.base + c * v.pitch, sizeof(row));
      const int64_t i = eps::shard_global_row(before + c, s, G);   // the global row this local row must be
      CHECK(i >= n0 && i < n0 + n_new);
      CHECK(row[0] == (float)(i * dim) && row[2] == (float)(i * dim + 2));
    }
  }
  CHECK(total == n_new);
}

// shard_split_bits against the per-bit definition, out of a bitset of exactly ceil(n / 8) bytes into one of exactly ceil(rows_of / 8) bytes
static void bits(int G, int64_t n, unsigned pattern) {
  Block b((size_t)((n + 7) / 8));
  srand(pattern * 977u + (unsigned)n * 31u + (unsigned)G);
  for (size_t i = 0; i < b.bytes; ++i) b.p[i] = pattern == 0 ? 0 : (pattern == 1 ? 0xFF : (unsigned char)(rand() & 0xFF));
  if (pattern == 3) {   // one residue class only (and the bits beyond n in the last byte): the other shards' slices must come out all zero
    memset(b.p, 0, b.bytes);
    for (int64_t i = G - 1; i < n; i += G) b.p[i >> 3] |= (unsigned char)(1u << (i & 7));
    for (int64_t i = n; i < (int64_t)b.bytes * 8; ++i) b.p[i >> 3] |= (unsigned char)(1u << (i & 7));
  }
  for (int s = 0; s < G; ++s) {
    const int64_t ns = eps::shard_rows_of(s, n, G);
    Block out((size_t)((ns + 7) / 8));
    memset(out.p, 0xA5, out.bytes);
    eps::shard_split_bits(b.p, n, s, G, out.p);
    for (int64_t l = 0; l < (int64_t)out.bytes * 8; ++l) {
      const int got = (out.p[l >> 3] >> (l & 7)) & 1;
      const int64_t i = l * G + s;
      const int want = l < ns ? (b.p[i >> 3] >> (i & 7)) & 1 : 0;
      CHECK(got == want);
    }
    unsigned any = 0;
    for (size_t i = 0; i < b.bytes; ++i) any |= b.p[i];
    CHECK(eps::shard_any_byte(b.p, (int64_t)b.bytes) == (any != 0));
    if (pattern == 3 && s != G - 1)
      for (size_t i = 0; i < out.bytes; ++i) CHECK(out.p[i] == 0);
  }
}

// a filter column of exactly (n - 1) * stride + width bytes (offset bytes of a record in front of the value are the caller's: `column` already
// points at row 0's value): every value a shard's upload reads - (ns - 1) * view.stride + width bytes from view.base - lies inside, and is its row's
static void column(int G, int64_t n, int width, int64_t stride, int64_t offset) {
  const size_t whole = n > 0 ? (size_t)(offset + (n - 1) * stride + width) : 0;   // the caller's records end with the last row's value
  Block rec(whole);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = -(i + 1);
    memcpy(rec.p + offset + i * stride, &v, (size_t)width);   // (little endian: the low bytes)
  }
  const unsigned char* col = rec.p + offset;
  for (int s = 0; s < G; ++s) {
    const eps::ShardColumnView v = eps::shard_column_view(col, stride, s, G);
    const int64_t ns = eps::shard_rows_of(s, n, G);
    CHECK(v.stride == stride * G);
    if (ns == 0) continue;   // (nothing is read)
    const size_t bytes = (size_t)((ns - 1) * v.stride + width);   // what Index::set_int_filter uploads
    std::vector<unsigned char> up(bytes);
    memcpy(up.data(), v.base, bytes);
    for (int64_t l = 0; l < ns; ++l) {
      int64_t got = -1;   // (all ones: the sign extension of a negative value of any width)
      memcpy(&got, up.data() + l * v.stride, (size_t)width);
      CHECK(got == -(l * G + s + 1));
    }
  }
}

// attribute rows of exactly n_rows * stride bytes: the shard's count rows of row_bytes at pitch bytes, as hipMemcpy2D reads them
static void attrs(int G, int64_t n_rows, int64_t stride) {
  Block t((size_t)(n_rows * stride));
  for (int64_t i = 0; i < n_rows; ++i)
    for (int64_t b = 0; b < stride; ++b) t.p[i * stride + b] = (unsigned char)((i * 7 + b) & 0xFF);
  int64_t total = 0;
  for (int s = 0; s < G; ++s) {
    const eps::ShardAttrView v = eps::shard_attr_view(t.p, stride, n_rows, s, G);
    CHECK(v.count == eps::shard_rows_of(s, n_rows, G) && v.row_bytes == stride && v.pitch == stride * G);
    total += v.count;
    std::vector<unsigned char> row((size_t)stride);
    for (int64_t l = 0; l < v.count; ++l) {
      memcpy(row.data(), v.base + l * v.pitch, (size_t)v.row_bytes);
      const int64_t i = l * G + s;
      CHECK(row[0] == (unsigned char)((i * 7) & 0xFF) && row[(size_t)stride - 1] == (unsigned char)((i * 7 + stride - 1) & 0xFF));
    }
  }
  CHECK(total == n_rows);
}

static void gather_and_counts() {
  for (int64_t nq : {0, 1, 3, 4, 64, 129})
    for (int k : {1, 2, 3, 10, 100, 1025}) {
      const size_t st = eps::shard_gather_stride(nq, k);
      CHECK(st % 8 == 0 && st >= (size_t)nq * k * 12 && st < (size_t)nq * k * 12 + 8);
    }
  for (int k : {1, 2, 7})
    for (int64_t nq : {0, 1, 5}) {
      Block ids((size_t)(nq * k) * 8), counts((size_t)nq * 4);
      std::vector<int32_t> want((size_t)nq);
      for (int64_t q = 0; q < nq; ++q) {
        want[(size_t)q] = (int32_t)((q * 3 + 1) % (k + 1));   // 0 .. k rows, a full list among them
        for (int e = 0; e < k; ++e) {
          const int64_t id = e < want[(size_t)q] ? (e == 0 ? 0 : q * 100 + e) : -1;   // (id 0 is a row)
          memcpy(ids.p + (q * k + e) * 8, &id, 8);
        }
      }
      eps::shard_counts_from_ids(reinterpret_cast<const int64_t*>(ids.p), nq, k, reinterpret_cast<int32_t*>(counts.p));
      for (int64_t q = 0; q < nq; ++q) {
        int32_t c;
        memcpy(&c, counts.p + q * 4, 4);
        CHECK(c == want[(size_t)q]);
      }
    }
}

int main() {
  for (int G = 1; G <= 16; ++G) {
    for (int64_t n = 0; n <= 200; ++n) {
      split(G, n);
      for (unsigned pattern = 0; pattern < 4; ++pattern) bits(G, n, pattern);
      for (int width : {1, 2, 4, 8}) column(G, n, width, width, 0);
      column(G, n, 4, 12, 4);   // a 12-byte record, the value at offset 4
      column(G, n, 8, 12, 4);   // ... and one that ends with the record
      attrs(G, n, 24);
      attrs(G, n, 1);
    }
    for (int64_t n : {0, 1, 7, 8, 9, 200}) rows(G, n, 5);
    for (int64_t n0 = 0; n0 <= 40; ++n0)
      for (int64_t n_new = 0; n_new <= 40; ++n_new) append(G, n0, n_new);
  }
  gather_and_counts();
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("shard_host_check OK\n");
  return 0;
}
