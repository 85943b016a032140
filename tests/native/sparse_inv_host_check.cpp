// Stand-alone check of csrc/sparse_inv_host.hpp (the host planning of the inverted lists of a sparse index), built with
// -fsanitize=address,undefined and run as a program by tests/test_sparse_inv_ref_cpu.py: tile and LDS sizes at every k class, queries of 0, 1, 64,
// 65 and 4096 terms, n of 0, 1, tile - 1, tile, tile + 1, the size arithmetic at nnz = 2^31 - 1 and 2^33, the dim limit on both sides.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vectordb_amd/csrc/sparse_inv_host.hpp"

using namespace eps;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// every row of [0, n) belongs to exactly one wavefront, in order, and a wavefront's tiles cover its rows; walks the tiles as the kernel does
static void check_cover(const SparseInvPlan& p, int64_t n) {
  int64_t next = 0;
  for (int64_t w = 0; w < p.rows.W; ++w) {
    int64_t b = -1, e = -1;
    sparse_wave_rows(p.rows, n, w, &b, &e);
    CHECK(b == next && e >= b && e <= n);
    int64_t tiles = 0;
    std::vector<char> acc((size_t)SPARSE_INV_TILE_ROWS, 0);   // the wavefront's LDS slice: every slot index stays inside it
    for (int64_t t0 = b; t0 < e; t0 += SPARSE_INV_TILE_ROWS) {
      const int64_t t1 = e - t0 < SPARSE_INV_TILE_ROWS ? e : t0 + SPARSE_INV_TILE_ROWS;
      CHECK(t1 > t0 && t1 - t0 <= SPARSE_INV_TILE_ROWS);
      acc[(size_t)(t1 - 1 - t0)] = 1;
      acc[0] = 1;
      ++tiles;
    }
    CHECK(tiles == (e - b + SPARSE_INV_TILE_ROWS - 1) / SPARSE_INV_TILE_ROWS);
    next = e;
  }
  CHECK(next == n);
}

int main() {
  const int64_t T = SPARSE_INV_TILE_ROWS;
  static_assert(SPARSE_INV_ACC_BYTES == 32768, "four wavefronts of 2048 fp32 accumulators");
  static_assert(SPARSE_INV_STATIC_LDS + SPARSE_MAX_QUERY_NNZ * 8 + SPARSE_INV_ACC_BYTES <= SPARSE_LDS_BUDGET, "the longest query still fits");
  static_assert(SPARSE_INV_TILE_ROWS % SPARSE_WAVE_ROWS == 0, "the finish step walks a tile 64 rows at a time");
  static_assert(SPARSE_INV_TERMS == 64, "one term per lane");
  const int32_t ks[] = {1, 10, 64, 65, 128, 129, 256, 257, 512, 513, 1024};   // both sides of every WaveTopK width
  const int64_t qlens[] = {0, 1, 64, 65, 4096};
  const int64_t ns[] = {0, 1, T - 1, T, T + 1, 2 * T + 1, 20000, 1000000, SPARSE_MAX_ROWS};
  const int64_t nqs[] = {1, 3, 33, 1024, 100000};
  for (int32_t k : ks)
    for (int64_t ql : qlens)
      for (int64_t n : ns)
        for (int64_t nq : nqs) {
          const SparseInvPlan p = sparse_inv_plan(n, nq, k, ql);
          CHECK(p.rows.nq_tile == 1 && p.rows.tiles == nq);
          CHECK(p.rows.qcap >= ql && p.rows.qcap >= 4 && p.rows.qcap % 4 == 0 && p.rows.qcap <= SPARSE_MAX_QUERY_NNZ);
          CHECK(p.acc_offset == p.rows.qcap * 8 && p.acc_offset % 16 == 0);
          CHECK(p.lds_dynamic == p.acc_offset + SPARSE_INV_ACC_BYTES);
          CHECK(SPARSE_INV_STATIC_LDS + p.lds_dynamic <= SPARSE_LDS_BUDGET);
          CHECK(p.rows.W >= SPARSE_BLOCK_WAVES && p.rows.W % SPARSE_BLOCK_WAVES == 0);
          CHECK(p.rows.W == SPARSE_BLOCK_WAVES || (int64_t)p.rows.W * k <= AMONG_MERGE_KEYS);
          CHECK((int64_t)p.rows.W / SPARSE_BLOCK_WAVES * (nq < SPARSE_MAX_BLOCKS ? nq : 1) <= SPARSE_MAX_BLOCKS || p.rows.W == SPARSE_BLOCK_WAVES);
          CHECK(p.rows.rows_per_wave >= SPARSE_WAVE_ROWS && p.rows.rows_per_wave % SPARSE_WAVE_ROWS == 0);
          CHECK(p.rows.rows_per_wave * p.rows.W >= n);
          if (n <= 4 * T * 2) check_cover(p, n);
        }
  {   // a single query over a large table: wavefronts get part of a tile so that the chip has workgroups; a batch gets whole tiles
    const SparseInvPlan one = sparse_inv_plan(1000000, 1, 10, 32), many = sparse_inv_plan(1000000, 1024, 10, 32);
    CHECK(one.rows.W / SPARSE_BLOCK_WAVES >= 256 && one.rows.rows_per_wave <= T);
    CHECK(many.rows.W == 2 * SPARSE_BLOCK_WAVES && many.rows.rows_per_wave == 125056);
    check_cover(sparse_inv_plan(3 * T + 5, 1, 10, 32), 3 * T + 5);
    const SparseInvPlan big = sparse_inv_plan(SPARSE_MAX_ROWS, 1, 1024, 4096);
    int64_t b, e;
    sparse_wave_rows(big.rows, SPARSE_MAX_ROWS, big.rows.W - 1, &b, &e);
    CHECK(e == SPARSE_MAX_ROWS && b < e);
  }
  {   // sizes
    SparseInvBytes s;
    CHECK(sparse_inv_bytes(1, 0, &s) && s.directory == 16 && s.postings == 0 && s.pairs == 0 && s.keys_a == 0 && s.keys_b == 0 && s.table == 8 * 256);
    CHECK(sparse_inv_bytes(30522, ((int64_t)1 << 31) - 1, &s));   // 15 key bits: two passes, one key buffer
    CHECK(s.postings == 8 * (((int64_t)1 << 31) - 1) && s.pairs == s.postings && s.keys_a == 4 * (((int64_t)1 << 31) - 1) && s.keys_b == 0 && s.directory == 8 * 30523);
    CHECK(s.postings > ((int64_t)1 << 33) && s.keys_a > ((int64_t)1 << 32) && s.table == 8 * 256 * SPARSE_INV_SORT_BLOCKS);   // none of them fits 32 bits
    CHECK(sparse_inv_bytes(30522, (int64_t)1 << 33, &s) && s.postings == ((int64_t)1 << 36) && s.keys_a == ((int64_t)1 << 35));
    CHECK(sparse_inv_bytes(200, (int64_t)1 << 33, &s) && s.keys_a == 0 && s.keys_b == 0);   // one pass writes no keys
    CHECK(sparse_inv_bytes(SPARSE_INV_MAX_DIM, SPARSE_INV_MAX_NNZ, &s) && s.postings == ((int64_t)1 << 43) && s.keys_b == ((int64_t)1 << 42) &&
          s.directory == 8 * (SPARSE_INV_MAX_DIM + 1));
    // the sort's chunks: consecutive, covering, a multiple of 256 long and short enough for a 32-bit count
    for (int64_t nnz : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)262144, (int64_t)262145, ((int64_t)1 << 31) - 1, (int64_t)1 << 33,
                        SPARSE_INV_MAX_NNZ})
      for (int64_t dim : {(int64_t)1, (int64_t)256, (int64_t)257, (int64_t)65536, (int64_t)65537, SPARSE_INV_MAX_DIM}) {
        const SparseInvSortPlan p = sparse_inv_sort_plan(nnz, dim);
        CHECK(p.passes == (dim <= 256 ? 1 : dim <= 65536 ? 2 : 3) && p.passes * 8 >= sparse_inv_key_bits(dim));
        CHECK(p.blocks >= 1 && p.blocks <= SPARSE_INV_SORT_BLOCKS && p.chunk % 256 == 0 && p.chunk >= 256 && p.chunk < ((int64_t)1 << 32));
        CHECK(p.blocks * p.chunk >= nnz);
        int64_t next = 0;
        for (int64_t b = 0; b < p.blocks; ++b) {
          int64_t cb = -1, ce = -1;
          sparse_inv_chunk(p, nnz, b, &cb, &ce);
          CHECK(cb == next && ce >= cb && ce <= nnz && ce - cb <= p.chunk);
          next = ce;
        }
        CHECK(next == nnz);
      }
    CHECK(!sparse_inv_bytes(SPARSE_INV_MAX_DIM, SPARSE_INV_MAX_NNZ + 1, &s) && !sparse_inv_bytes(8, -1, &s) && !sparse_inv_bytes(8, INT64_MAX, &s));
    // the dim limit on both sides
    CHECK(SPARSE_INV_MAX_DIM == ((int64_t)1 << 24));
    CHECK(sparse_inv_bytes(SPARSE_INV_MAX_DIM, 10, &s) && !sparse_inv_bytes(SPARSE_INV_MAX_DIM + 1, 10, &s) && !sparse_inv_bytes(0, 10, &s));
    CHECK(sparse_inv_key_bits(1) == 1 && sparse_inv_key_bits(2) == 1 && sparse_inv_key_bits(3) == 2 && sparse_inv_key_bits(400) == 9);
    CHECK(sparse_inv_key_bits(30522) == 15 && sparse_inv_key_bits(SPARSE_INV_MAX_DIM) == 24 && sparse_inv_key_bits(SPARSE_INV_MAX_DIM - 1) == 24);
    for (int64_t d : {(int64_t)1, (int64_t)2, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)65536, SPARSE_INV_MAX_DIM})
      CHECK(((int64_t)1 << sparse_inv_key_bits(d)) >= d);   // every column index below dim has all its bits inside the sorted digits
    // build grids
    CHECK(sparse_inv_build_blocks(0, 4) == 1 && sparse_inv_build_blocks(1, 4) == 1 && sparse_inv_build_blocks(5, 4) == 2);
    CHECK(sparse_inv_build_blocks(SPARSE_MAX_ROWS, 4) == SPARSE_INV_BUILD_BLOCKS && sparse_inv_build_blocks((int64_t)1 << 33, 256) == SPARSE_INV_BUILD_BLOCKS);
  }
  std::printf("sparse_inv_host_check OK\n");
  return 0;
}
