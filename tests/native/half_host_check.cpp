// Stand-alone host check of csrc/half_host.hpp - the float -> half rounding, the limits, the refusals, the launch plan of eps_half_index_search and
// its seed rule - for a CPU build under -fsanitize=address,undefined (tests/test_half_host_cpu.py).  Every slice takes its rows through
// half_slice_rows, as the kernel does.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../vectordb_amd/csrc/half_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

static float as_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t as_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static bool is_nan_half(uint16_t h, int bf) { return bf ? (h & 0x7FFF) > 0x7F80 : (h & 0x7FFF) > 0x7C00; }

// all 2^16 patterns round-trip; between two neighbours the lower half of the gap goes down, the upper half up and the midpoint to the even one
static void rounding() {
  for (int bf = 0; bf < 2; ++bf) {
    const uint16_t inf = bf ? 0x7F80 : 0x7C00;
    for (uint32_t h = 0; h < 65536; ++h) {
      const uint32_t f = half_to_float_bits((uint16_t)h, bf);
      const uint16_t back = half_from_float_bits(f, bf);
      if (is_nan_half((uint16_t)h, bf)) {
        CHECK(isnan(as_float(f)) && is_nan_half(back, bf) && (back & 0x8000) == (h & 0x8000));
        continue;
      }
      CHECK(back == h);
      if ((h & 0x7FFF) >= inf) continue;
      const double lo = as_float(f), hi = as_float(half_to_float_bits((uint16_t)(h + 1), bf));   // the next pattern away from zero (or the infinity)
      const double top = (h & 0x7FFF) + 1 == inf ? 2.0 * lo - as_float(half_to_float_bits((uint16_t)(h - 1), bf)) : hi;   // (the step of the last binade)
      const float mid = (float)(0.5 * (lo + top));                                              // exact in a float: one more bit than a half
      CHECK(half_from_float_bits(as_bits(mid), bf) == ((h & 1) ? h + 1 : h));                   // the tie: to the even pattern
      CHECK(half_from_float_bits(as_bits(mid) - 1, bf) == h && half_from_float_bits(as_bits(mid) + 1, bf) == h + 1);
    }
    CHECK(is_nan_half(half_from_float_bits(0x7F800001u, bf), bf) && is_nan_half(half_from_float_bits(0xFFC00000u, bf), bf));
    CHECK(half_from_float_bits(0x7F800000u, bf) == inf && half_from_float_bits(0xFF800000u, bf) == (0x8000 | inf));
    CHECK(half_from_float_bits(as_bits(3.0e38f), bf) == (bf ? 0x7F62 : inf) && half_from_float_bits(as_bits(1e-45f), bf) == (bf ? 0x0000 : 0));
  }
  CHECK(half_from_float_bits(as_bits(65519.99f), 0) == 0x7BFF && half_from_float_bits(as_bits(65520.f), 0) == 0x7C00);
  CHECK(half_from_float_bits(as_bits(ldexpf(1.f, -25)), 0) == 0 && half_from_float_bits(as_bits(ldexpf(1.f, -25)) + 1, 0) == 1);
}

static void layout() {
  CHECK(HALF_MAX_K == 1024 && HALF_MAX_DIM == 4096 && HALF_MAX_ROWS == 2147483647 && HALF_KSTEP == 32 && HALF_WAVE_ROWS == 64);
  for (int64_t dim = 1; dim <= 4096; ++dim) CHECK(half_pad(dim) % 32 == 0 && half_pad(dim) >= dim && half_pad(dim) < dim + 32);
  CHECK(half_pad_rows(0) == 0 && half_pad_rows(1) == 64 && half_pad_rows(64) == 64 && half_pad_rows(65) == 128);
  CHECK(HALF_PATCH_PITCH >= 16 && (4 * HALF_PATCH_PITCH) % 64 == 16 && HALF_PATCH_PITCH % 4 == 0);
  CHECK(half_create_refusal(0, 0) && half_create_refusal(4097, 0) && half_create_refusal(-1, 2) && !half_create_refusal(1, 0) && !half_create_refusal(4096, 2));
  CHECK(!half_create_refusal(64, EPS_METRIC_COSINE) && half_create_refusal(64, 3) && half_create_refusal(64, -1));
  uint16_t b = 0;
  CHECK(half_attach_refusal(64, &b, -1, 64) && half_attach_refusal(64, &b, (int64_t)1 << 31, 64) && half_attach_refusal(64, nullptr, 1, 64));
  CHECK(half_attach_refusal(65, &b, 1, 64) && !half_attach_refusal(64, &b, 1, 64) && !half_attach_refusal(64, nullptr, 0, 0));
  CHECK(half_search_refusal(1, 0) && half_search_refusal(1, 1025) && half_search_refusal(-1, 1) && !half_search_refusal(0, 1) && !half_search_refusal(5, 1024));
}

static void plans() {
  const int64_t ns[] = {0, 1, 63, 64, 65, 257, 3000, 32767, 32768, 40000, 1000000, 10000000, 300000000, HALF_MAX_ROWS};
  const int ks[] = {1, 10, 64, 65, 128, 129, 256, 257, 512, 513, 1024};
  const int64_t nqs[] = {1, 15, 16, 17, 32, 33, 64, 65, 1024, 100000, HALF_MAX_ROWS};
  const int64_t dims[] = {1, 31, 32, 33, 768, 1024, 1056, 2048, 2080, 4096};
  for (int64_t n : ns)
    for (int k : ks)
      for (int64_t nq : nqs)
        for (int64_t dim : dims) {
          const HalfPlan p = half_plan(n, dim, nq, k);
          const int64_t d_pad = half_pad(dim);
          CHECK(p.kpl == binary_kpl(k) && p.kpl * 64 >= k);
          const int by_k = k <= 64 ? 4 : k <= 128 ? 2 : 1, by_d = d_pad <= 1024 ? 4 : d_pad <= 2048 ? 2 : 1, by_q = nq > 32 ? 4 : nq > 16 ? 2 : 1;
          const int nb = by_k < by_d ? (by_k < by_q ? by_k : by_q) : (by_d < by_q ? by_d : by_q);
          CHECK(p.nb == nb);
          CHECK(p.cols == (64 / p.kpl < 16 * p.nb ? 64 / p.kpl : 16 * p.nb) && p.cols * p.kpl <= HALF_LIST_BUDGET);
          CHECK((int64_t)p.nb * 32 * d_pad <= HALF_LDS_QUERY_BYTES && p.lds_bytes <= 160 * 1024);   // LDS
          CHECK(p.lds_bytes == (int64_t)p.nb * 32 * d_pad + 4 * 64 * HALF_PATCH_PITCH * 4);
          CHECK(p.tiles == (nq + p.cols - 1) / p.cols && p.launches == (p.tiles + BIN_GRID_Y - 1) / BIN_GRID_Y);
          CHECK(p.slices >= HALF_BLOCK_WAVES && p.slices % HALF_BLOCK_WAVES == 0);
          CHECK(p.rows_per_slice >= HALF_WAVE_ROWS && p.rows_per_slice % HALF_WAVE_ROWS == 0);
          CHECK(p.slices * p.rows_per_slice >= n);
          const int64_t blocks = p.slices / HALF_BLOCK_WAVES;
          CHECK(blocks == 1 || (blocks * p.tiles <= HALF_MAX_BLOCKS && p.slices * k <= HALF_MERGE_KEYS));
          CHECK(blocks <= 65535 && p.slices * k < ((int64_t)1 << 31));   // a grid dimension; the merge's `int slots`
          CHECK(p.partial_bytes == nq * p.slices * k * 8 && p.run_bytes == nq * k * 8 && p.partial_bytes >= p.run_bytes && p.partial_bytes > 0);
          // the seed rule: a prefix within the table, whole workgroup passes, long enough for a list to fill; its own plan needs no more scratch
          const int64_t sr = half_seed_rows(n, dim, nq, k);
          CHECK((sr > 0) == (n >= HALF_SEED_MIN_ROWS));
          if (sr > 0) {
            CHECK(sr % 256 == 0 && 2 * sr <= n && sr >= 4096 && sr >= 8 * k && sr >= n / 16 && sr < n / 16 + 256 + 8192);
            CHECK(half_plan(sr, dim, nq, k).partial_bytes <= p.partial_bytes && half_plan(sr, dim, nq, k).nb == p.nb);
          }
          if (dim != 32 && dim != 4096) continue;   // (the slices depend on dim only through the number of tiles)
          int64_t next = 0, rounds = 0;
          for (int64_t s = 0; s < p.slices; ++s) {
            int64_t b = -1, e = -1;
            half_slice_rows(p.rows_per_slice, n, s, &b, &e);
            CHECK(0 <= b && b <= e && e <= n && e - b <= p.rows_per_slice);
            CHECK(b == next || (b == n && e == n));
            CHECK(b == n || b % HALF_WAVE_ROWS == 0);
            CHECK(e <= half_pad_rows(n) && (b == e || (e - 1) / 64 * 64 + 63 < half_pad_rows(n)));   // a round's 64 rows lie inside the padded table
            rounds += (e - b + HALF_WAVE_ROWS - 1) / HALF_WAVE_ROWS;
            next = e;
          }
          CHECK(next == n && rounds * p.tiles == p.rounds);
        }
}

// The shapes at which a slice walks more than one round (tests/half_walk_ref.py: SHAPES; tests/test_gpu_half_rounds.py runs them): the caps bind
// exactly as that table says.  A change of a cap or of the seed rule fails here instead of letting those tests fall back to one round per slice
static void long_slices() {
  struct Shape {
    int64_t n, dim, nq;
    int k, cols, kpl, nb;
    int64_t tiles, slices, rows_per_slice, seed_rows, seed_slices, seed_rows_per_slice;
  };
  const Shape shapes[] = {
      {32767, 40, 2053, 10, 64, 1, 4, 33, 248, 192, 0, 0, 0},        // R1: 3 rounds; slices from 171 on are empty; the last tile has 5 queries
      {40000, 40, 2053, 10, 64, 1, 4, 33, 248, 192, 4096, 64, 64},   // R1s
      {60000, 40, 5, 1024, 4, 16, 1, 2, 256, 256, 8192, 128, 64},    // R2: 4 rounds, the merge's cap; the 8 k rule
      {40000, 40, 300, 1024, 4, 16, 1, 75, 108, 384, 8192, 108, 128},   // R3: 6 rounds; the seed pass walks two
      {15000, 40, 2060, 129, 16, 4, 1, 129, 60, 256, 0, 0, 0},       // R4
      {24000, 40, 2060, 65, 32, 2, 2, 65, 124, 256, 0, 0, 0},        // R5
      {24000, 1056, 2060, 10, 32, 1, 2, 65, 124, 256, 0, 0, 0},      // R6: NB = 2 by LDS
      {15000, 2080, 2060, 10, 16, 1, 1, 129, 60, 256, 0, 0, 0},      // R7: NB = 1 by LDS
      {12000, 40, 2060, 257, 8, 8, 1, 258, 28, 448, 0, 0, 0},        // R8: 7 rounds
  };
  for (const Shape& s : shapes) {
    const HalfPlan p = half_plan(s.n, s.dim, s.nq, s.k);
    CHECK(p.cols == s.cols && p.kpl == s.kpl && p.nb == s.nb && p.tiles == s.tiles && p.launches == 1);
    CHECK(p.slices == s.slices && p.rows_per_slice == s.rows_per_slice && p.rows_per_slice > HALF_WAVE_ROWS);
    CHECK(p.rounds == (s.n + 63) / 64 * s.tiles);
    const int64_t sr = half_seed_rows(s.n, s.dim, s.nq, s.k);
    CHECK(sr == s.seed_rows);
    if (sr > 0) {
      const HalfPlan q = half_plan(sr, s.dim, s.nq, s.k);
      CHECK(q.slices == s.seed_slices && q.rows_per_slice == s.seed_rows_per_slice && q.cols == s.cols && q.kpl == s.kpl && q.tiles == s.tiles);
    }
  }
  int64_t b = -1, e = -1;   // R1's last non-empty slice is ragged, the next one empty
  half_slice_rows(192, 32767, 170, &b, &e);
  CHECK(b == 32640 && e == 32767);
  half_slice_rows(192, 32767, 171, &b, &e);
  CHECK(b == 32767 && e == 32767);
}

int main() {
  rounding();
  layout();
  plans();
  long_slices();
  if (failures) printf("half_host_check: %d check(s) failed\n", failures);
  else printf("half_host_check OK\n");
  return failures != 0;
}
