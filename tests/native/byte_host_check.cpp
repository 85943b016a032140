// Stand-alone host check of csrc/byte_host.hpp - the integer terms, the limits, the refusals and the launch plan of eps_byte_index_search - for a
// CPU build under -fsanitize=address,undefined (tests/test_byte_host_cpu.py).  Every slice takes its rows through byte_slice_rows, as the kernel does.
#include <stdio.h>
#include <initializer_list>

#include "../../vectordb_amd/csrc/byte_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

// every byte pair of a one-dimensional vector: row_term + query_term - (dot' << shift) is the plain distance
static void terms() {
  for (int metric : {EPS_METRIC_EUCLIDEAN, EPS_METRIC_DOT_PRODUCT})
    for (int uns = 0; uns < 2; ++uns)
      for (int x = 0; x < 256; ++x)
        for (int q = 0; q < 256; ++q) {
          const int64_t xv = uns ? x : (int8_t)x, qv = uns ? q : (int8_t)q;
          const int64_t want = metric == EPS_METRIC_EUCLIDEAN ? (xv - qv) * (xv - qv) : -xv * qv;
          const int32_t xs = byte_stored((uint8_t)x, uns), qs = byte_stored((uint8_t)q, uns);
          CHECK(xs >= -128 && xs <= 127 && xs == xv - (uns ? 128 : 0));
          const int64_t got = (int64_t)byte_term(metric, uns, 0, xs, xs * xs, 1) + byte_term(metric, uns, 1, qs, qs * qs, 1) -
                              ((int64_t)(xs * qs) * (1 << byte_dot_shift(metric)));
          CHECK(got == want);
        }
  // the extremes at the longest vector fit an int32 with room for the bias: |distance| < 2^31 - 1
  CHECK((int64_t)255 * 255 * BYTE_MAX_DIM < 2147483647 && (int64_t)128 * 128 * BYTE_MAX_DIM * 2 < 2147483647);
  CHECK(byte_term(EPS_METRIC_DOT_PRODUCT, 1, 1, 127 * 4096, 0, 4096) == -128 * 127 * 4096 - 16384 * 4096);
}

static void layout() {
  CHECK(BYTE_MAX_K == 1024 && BYTE_MAX_DIM == 4096 && BYTE_MAX_ROWS == 2147483647 && BYTE_KSTEP == 64 && BYTE_WAVE_ROWS == 64);
  for (int64_t dim = 1; dim <= 4096; ++dim) CHECK(byte_pad(dim) % 64 == 0 && byte_pad(dim) >= dim && byte_pad(dim) < dim + 64);
  CHECK(byte_pad_rows(0) == 0 && byte_pad_rows(1) == 64 && byte_pad_rows(64) == 64 && byte_pad_rows(65) == 128);
  for (int nb = 1; nb <= 2; ++nb) CHECK(byte_patch_pitch(nb) >= 16 * nb && (4 * byte_patch_pitch(nb)) % 64 == 16 && byte_patch_pitch(nb) % 4 == 0);
  CHECK(byte_create_refusal(0, 0) && byte_create_refusal(4097, 0) && byte_create_refusal(-1, 2) && !byte_create_refusal(1, 0) && !byte_create_refusal(4096, 2));
  CHECK(byte_create_refusal(64, EPS_METRIC_COSINE) && byte_create_refusal(64, 3) && byte_create_refusal(64, -1));
  uint8_t b = 0;
  CHECK(byte_attach_refusal(64, &b, -1, 64) && byte_attach_refusal(64, &b, (int64_t)1 << 31, 64) && byte_attach_refusal(64, nullptr, 1, 64));
  CHECK(byte_attach_refusal(65, &b, 1, 64) && !byte_attach_refusal(64, &b, 1, 64) && !byte_attach_refusal(64, nullptr, 0, 0));
  CHECK(byte_search_refusal(1, 0) && byte_search_refusal(1, 1025) && byte_search_refusal(-1, 1) && !byte_search_refusal(0, 1) && !byte_search_refusal(5, 1024));
}

static void plans() {
  const int64_t ns[] = {0, 1, 63, 64, 65, 130, 1000, 20000, 600000, 1000000, 10000000, 300000000, BYTE_MAX_ROWS};
  const int ks[] = {1, 10, 64, 65, 128, 129, 256, 257, 512, 513, 1024};
  const int64_t nqs[] = {1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 1024, 100000, BYTE_MAX_ROWS};
  const int64_t dims[] = {1, 64, 65, 768, 2048, 2049, 4096};
  for (int64_t n : ns)
    for (int k : ks)
      for (int64_t nq : nqs)
        for (int64_t dim : dims) {
          const BytePlan p = byte_plan(n, dim, nq, k);
          const int64_t d_pad = byte_pad(dim);
          CHECK(p.kpl == binary_kpl(k) && p.kpl * 64 >= k);
          // the six forms: two column blocks only with one register pair per list, more than 16 queries and both blocks' operands in 64 KB
          CHECK(p.nb == (k <= 64 && nq > 16 && d_pad <= 2048 ? 2 : 1));
          CHECK(p.cols == (p.nb == 2 ? 32 : p.kpl <= 4 ? 16 : p.kpl == 8 ? 8 : 4));
          CHECK(p.cols * p.kpl <= BYTE_LIST_BUDGET && p.cols <= 16 * p.nb);                  // registers
          CHECK((int64_t)p.nb * 16 * d_pad <= BYTE_LDS_QUERY_BYTES && p.lds_bytes <= 160 * 1024);   // LDS
          CHECK(p.lds_bytes == (int64_t)p.nb * 16 * d_pad + 4 * 64 * byte_patch_pitch(p.nb) * 4);
          CHECK(p.tiles == (nq + p.cols - 1) / p.cols && p.launches == (p.tiles + BIN_GRID_Y - 1) / BIN_GRID_Y);
          CHECK(p.slices >= BYTE_BLOCK_WAVES && p.slices % BYTE_BLOCK_WAVES == 0);
          CHECK(p.rows_per_slice >= BYTE_WAVE_ROWS && p.rows_per_slice % BYTE_WAVE_ROWS == 0);
          CHECK(p.slices * p.rows_per_slice >= n);
          const int64_t blocks = p.slices / BYTE_BLOCK_WAVES;
          CHECK(blocks == 1 || (blocks * p.tiles <= BYTE_MAX_BLOCKS && p.slices * k <= BYTE_MERGE_KEYS));
          CHECK(blocks <= 65535 && p.slices * k < ((int64_t)1 << 31));   // a grid dimension; the merge's `int slots`
          if (nq <= 32 && k == 10 && n >= 1000000) CHECK(blocks >= 1024);   // a short batch, a long table: the chip is filled
          if (n == 20000 && k == 1024 && p.tiles <= 32) CHECK(   // (the merge cap: 2^18 keys / 1024 = 256 lists)
p.slices == 256 && p.rows_per_slice == 128);
          CHECK(p.partial_bytes == nq * p.slices * k * 8 && p.run_bytes == nq * k * 8 && p.partial_bytes >= p.run_bytes && p.partial_bytes > 0);
          // every row once: the slices follow one another in multiples of 64 rows and end at n; the rounds are the plan's
          if (dim != 64 && dim != 4096) continue;   // (the slices depend on dim only through the number of tiles)
          int64_t next = 0, rounds = 0;
          for (int64_t s = 0; s < p.slices; ++s) {
            int64_t b = -1, e = -1;
            byte_slice_rows(p.rows_per_slice, n, s, &b, &e);
            CHECK(0 <= b && b <= e && e <= n && e - b <= p.rows_per_slice);
            CHECK(b == next || (b == n && e == n));
            CHECK(b == n || b % BYTE_WAVE_ROWS == 0);
            CHECK(e <= byte_pad_rows(n) && (b == e || (e - 1) / 64 * 64 + 63 < byte_pad_rows(n)));   // a round's 64 rows lie inside the padded table
            rounds += (e - b + BYTE_WAVE_ROWS - 1) / BYTE_WAVE_ROWS;
            next = e;
          }
          CHECK(next == n && rounds * p.tiles == p.rounds);
        }
}

int main() {
  terms();
  layout();
  plans();
  if (failures) printf("byte_host_check: %d check(s) failed\n", failures);
  else printf("byte_host_check OK\n");
  return failures != 0;
}
