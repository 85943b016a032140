// Stand-alone host check of csrc/binary_host.hpp - the layout of a packed row, the limits, the refusals and the launch plan of
// eps_binary_index_search - for a CPU build under -fsanitize=address,undefined (tests/test_binary_host_cpu.py builds and runs it).  Every slice of
// a plan takes its rows through binary_slice_rows, the function the kernel calls: a row taken twice or never shows in the walk.
#include <stdio.h>

#include "../../vectordb_amd/csrc/binary_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

static void layout() {
  CHECK(BIN_CW == 8 && BIN_MAX_K == 1024 && BIN_MAX_DIM == 65536 && BIN_MAX_ROWS == 2147483647);
  for (int64_t dim = 1; dim <= 200; ++dim) {   // every dim % 32, several times
    const int64_t W = binary_words(dim);
    CHECK(W * 32 >= dim && (W - 1) * 32 < dim);
    const uint32_t m = binary_tail_mask(dim);
    for (int b = 0; b < 32; ++b) CHECK((((m >> b) & 1u) != 0) == ((W - 1) * 32 + b < dim));   // bit b of the last word belongs to the vector
    const int64_t own = binary_owned_stride(W);
    CHECK(own >= W && own < W + 4 && (W < 4 ? own == W : own % 4 == 0));
  }
  CHECK(binary_words(65536) == 2048 && binary_tail_mask(65536) == 0xFFFFFFFFu && binary_tail_mask(1) == 1u && binary_tail_mask(33) == 1u);
  CHECK(binary_create_refusal(0) && binary_create_refusal(65537) && binary_create_refusal(-1) && !binary_create_refusal(1) && !binary_create_refusal(65536));
  uint32_t w = 0;
  CHECK(binary_attach_refusal(64, &w, -1, 2) && binary_attach_refusal(64, &w, (int64_t)1 << 31, 2) && binary_attach_refusal(64, nullptr, 1, 2));
  CHECK(binary_attach_refusal(65, &w, 1, 2) && !binary_attach_refusal(64, &w, 1, 2) && !binary_attach_refusal(64, nullptr, 0, 0));
  CHECK(binary_search_refusal(1, 0) && binary_search_refusal(1, 1025) && binary_search_refusal(-1, 1) && !binary_search_refusal(0, 1) && !binary_search_refusal(5, 1024));
}

static void plans() {
  const int64_t ns[] = {0, 1, 63, 64, 65, 130, 1000, 20000, 1000000, 10000000, 300000000, BIN_MAX_ROWS};
  const int ks[] = {1, 10, 64, 65, 128, 129, 256, 257, 512, 513, 1024};
  const int64_t nqs[] = {1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 1024, 100000, BIN_MAX_ROWS};
  for (int64_t n : ns)
    for (int k : ks)
      for (int64_t nq : nqs) {
        const BinaryPlan p = binary_plan(n, nq, k);
        CHECK(p.kpl == 1 || p.kpl == 2 || p.kpl == 4 || p.kpl == 8 || p.kpl == 16);
        CHECK(p.kpl * 64 >= k && (p.kpl == 1 || p.kpl * 32 < k));
        CHECK(p.nq_tile == 4 || p.nq_tile == 8 || p.nq_tile == 16 || p.nq_tile == 32);
        CHECK(p.nq_tile * p.kpl <= BIN_TILE_BUDGET || (p.kpl == 16 && p.nq_tile == BIN_MIN_TILE));   // the register budget; KPL = 16 keeps 4 queries
        CHECK(p.nq_tile == BIN_MIN_TILE || p.nq_tile / 2 < nq);                                        // no wider than the batch needs
        if (k <= 64 && nq >= 32) CHECK(p.nq_tile == 32);                                               // the table once per 32 queries
        CHECK(p.tiles == (nq + p.nq_tile - 1) / p.nq_tile && p.launches == (p.tiles + BIN_GRID_Y - 1) / BIN_GRID_Y);
        CHECK(p.slices >= BIN_BLOCK_WAVES && p.slices % BIN_BLOCK_WAVES == 0);
        CHECK(p.rows_per_slice >= BIN_WAVE_ROWS && p.rows_per_slice % BIN_WAVE_ROWS == 0);
        CHECK(p.slices * p.rows_per_slice >= n);
        const int64_t blocks = p.slices / BIN_BLOCK_WAVES;
        CHECK(blocks == 1 || (blocks * p.tiles <= BIN_MAX_BLOCKS && p.slices * k <= BIN_MERGE_KEYS));
        CHECK(blocks <= 65535 && p.slices * k < ((int64_t)1 << 31));                                   // a grid dimension; the merge's `int slots`
        if (nq <= 32 && k == 10 && n >= 1000000) CHECK(blocks >= 1024);                                // a short batch, a long table: the chip is filled
        CHECK(p.partial_bytes == nq * p.slices * k * 8 && p.run_bytes == nq * k * 8 && p.partial_bytes >= p.run_bytes);
        // every row once: the slices follow one another in multiples of 64 rows and end at n
        int64_t next = 0;
        for (int64_t s = 0; s < p.slices; ++s) {
          int64_t b = -1, e = -1;
          binary_slice_rows(p, n, s, &b, &e);
          CHECK(0 <= b && b <= e && e <= n && e - b <= p.rows_per_slice);
          CHECK(b == next || (b == n && e == n));
          CHECK(b == n || b % BIN_WAVE_ROWS == 0);
          next = e;
        }
        CHECK(next == n);
      }
}

int main() {
  layout();
  plans();
  if (failures) {
    printf("binary_host_check: %d check(s) failed\n", failures);
    return 1;
  }
  printf("binary_host_check OK\n");
  return 0;
}
