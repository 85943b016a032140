// Stand-alone check of csrc/hybrid_host.hpp (plan, LDS layout and argument checks of the hybrid search), built with -fsanitize=address,undefined and
// run as a program by tests/test_hybrid_ref_cpu.py: the LDS budget at dim 1 / 768 / the largest accepted, the staged queries falling from 4 to 1,
// the refusal beyond, every row in exactly one wavefront's tiles, and the layout's parts written end to end inside a buffer of the plan's size.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../vectordb_amd/csrc/hybrid_host.hpp"

using namespace eps;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// the parts of a workgroup's LDS are written as the kernel writes them - into a heap buffer of exactly lds_dynamic bytes (ASan sees one byte too far)
static void check_layout(const HybridPlan& p, int64_t dim) {
  const SparsePlan& r = p.rows;
  std::vector<char> lds((size_t)r.lds_dynamic, 0);
  CHECK(p.qstride >= dim && p.qstride % 4 == 0 && p.qstride < dim + 4);
  CHECK(p.idx_offset % 16 == 0 && p.val_offset % 16 == 0 && p.acc_offset % 16 == 0);
  CHECK(p.idx_offset == (int64_t)r.nq_tile * p.qstride * 4 && p.val_offset - p.idx_offset == r.nq_tile * r.qcap * 4 && p.acc_offset - p.val_offset == r.nq_tile * r.qcap * 4);
  float* dq = reinterpret_cast<float*>(lds.data());
  int* idx = reinterpret_cast<int*>(lds.data() + p.idx_offset);
  float* val = reinterpret_cast<float*>(lds.data() + p.val_offset);
  float* acc = reinterpret_cast<float*>(lds.data() + p.acc_offset);
  for (int q = 0; q < r.nq_tile; ++q) {
    dq[q * p.qstride] = dq[q * p.qstride + p.qstride - 1] = 1.f;
    idx[q * r.qcap] = idx[q * r.qcap + r.qcap - 1] = 1;
    val[q * r.qcap] = val[q * r.qcap + r.qcap - 1] = 1.f;
    for (int w = 0; w < HYB_BLOCK_WAVES; ++w) acc[(w * r.nq_tile + q) * HYB_TILE_ROWS] = acc[(w * r.nq_tile + q) * HYB_TILE_ROWS + HYB_TILE_ROWS - 1] = 1.f;
  }
  CHECK(p.acc_offset + (int64_t)HYB_BLOCK_WAVES * r.nq_tile * HYB_TILE_ROWS * 4 == r.lds_dynamic);
  CHECK(HYB_STATIC_LDS + r.lds_dynamic <= HYB_LDS_BUDGET && hybrid_parts_lds_bytes(dim, r.qcap) <= HYB_PARTS_LDS_BUDGET);
}

static void check_cover(const HybridPlan& p, int64_t n) {
  int64_t next = 0;
  for (int64_t w = 0; w < p.rows.W; ++w) {
    int64_t b = -1, e = -1;
    sparse_wave_rows(p.rows, n, w, &b, &e);
    CHECK(b == next && e >= b && e <= n);
    for (int64_t t0 = b; t0 < e; t0 += HYB_TILE_ROWS) {
      const int64_t t1 = e - t0 < HYB_TILE_ROWS ? e : t0 + HYB_TILE_ROWS;
      CHECK(t1 > t0 && t1 - t0 <= HYB_TILE_ROWS);
    }
    next = e;
  }
  CHECK(next == n);
}

int main() {
  const int64_t T = HYB_TILE_ROWS, QMAX = HYB_MAX_QUERY_NNZ;
  static_assert(HYB_TILE_ROWS % SPARSE_WAVE_ROWS == 0 && HYB_BLOCK_WAVES == AMONG_BLOCK_WAVES && HYB_LDS_BUDGET <= 160 * 1024 / 2, "two workgroups per CU");
  HybridPlan p;
  // NQ: 4 at short queries, falling with the staged terms and the dim; 1 above k = 128; the refusal where one query no longer fits
  CHECK(hybrid_plan(1000, 5, 10, 768, 128, &p) && p.rows.nq_tile == 4 && p.rows.lds_dynamic == 12288 + 4096 + 32768 && p.rows.tiles == 2);
  CHECK(hybrid_plan(1000, 5, 10, 768, QMAX, &p) && p.rows.nq_tile == 2 && p.rows.lds_dynamic == 6144 + 16384 + 16384 && p.rows.tiles == 3);
  CHECK(hybrid_plan(1000, 5, 10, 1, QMAX, &p) && p.rows.nq_tile == 2 && p.qstride == 4);
  CHECK(hybrid_plan(1000, 5, 10, 1, 0, &p) && p.rows.nq_tile == 4 && p.rows.qcap == 4);
  CHECK(hybrid_plan(1000, 5, 10, 8192, 64, &p) && p.rows.nq_tile == 1);
  CHECK(hybrid_plan(1000, 2, 128, 768, 64, &p) && p.rows.nq_tile == 2 && hybrid_plan(1000, 5, 129, 768, 64, &p) && p.rows.nq_tile == 1);
  const int64_t dmax = hybrid_max_dim(QMAX);
  CHECK(dmax == 12288 && hybrid_plan(1000, 5, 10, dmax, QMAX, &p) && p.rows.nq_tile == 1 && p.rows.lds_dynamic == HYB_LDS_BUDGET);
  CHECK(!hybrid_plan(1000, 5, 10, dmax + 1, QMAX, &p) && !hybrid_plan(1000, 1, 10, 0, 4, &p) && hybrid_plan(1000, 5, 10, hybrid_max_dim(4), 0, &p));
  const int32_t ks[] = {1, 10, 64, 65, 128, 129, 1024};
  const int64_t dims[] = {1, 3, 4, 768, 770, dmax}, qlens[] = {0, 1, 64, 65, QMAX}, ns[] = {0, 1, T - 1, T, T + 1, 2 * T + 1, 1000000, SPARSE_MAX_ROWS};
  for (int32_t k : ks)
    for (int64_t dim : dims)
      for (int64_t ql : qlens)
        for (int64_t n : ns)
          for (int64_t nq : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)1024, (int64_t)100000}) {
            CHECK(hybrid_plan(n, nq, k, dim, ql, &p));
            const SparsePlan& r = p.rows;
            CHECK((r.nq_tile == 1 || r.nq_tile == 2 || r.nq_tile == 4) && (k <= 128 || r.nq_tile == 1) && r.tiles == (nq + r.nq_tile - 1) / r.nq_tile);
            CHECK(r.qcap >= ql && r.qcap >= 4 && r.qcap % 4 == 0 && r.qcap <= QMAX);
            CHECK(r.W >= HYB_BLOCK_WAVES && r.W % HYB_BLOCK_WAVES == 0 && (r.W == HYB_BLOCK_WAVES || (int64_t)r.W * k <= AMONG_MERGE_KEYS));
            CHECK(r.rows_per_wave >= SPARSE_WAVE_ROWS && r.rows_per_wave % SPARSE_WAVE_ROWS == 0 && r.rows_per_wave * r.W >= n);
            check_layout(p, dim);
            if (n <= 8 * T) check_cover(p, n);
          }
  CHECK(hybrid_plan(2 * T + 1, 1024, 10, 768, 64, &p) && p.rows.W == HYB_BLOCK_WAVES);   // a batch: few wavefronts, whole tiles and more
  CHECK(hybrid_plan(1000000, 1, 10, 768, 64, &p) && p.rows.W / HYB_BLOCK_WAVES >= HYB_MIN_BLOCKS);   // one query: the chip still gets workgroups
  // the scalar arguments
  const char* why = nullptr;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  CHECK(hybrid_args_check(1, 1, 1.f, 1.f, &why) == EPS_OK && hybrid_args_check(0, 1024, 0.f, -2.f, &why) == EPS_OK);
  CHECK(hybrid_args_check(1, 0, 1.f, 1.f, &why) == EPS_USER_ERROR && hybrid_args_check(1, 1025, 1.f, 1.f, &why) == EPS_USER_ERROR && why[0] == 'k');
  CHECK(hybrid_args_check(-1, 1, 1.f, 1.f, &why) == EPS_USER_ERROR);
  for (float w : {inf, -inf, nan}) CHECK(hybrid_args_check(1, 1, w, 1.f, &why) == EPS_USER_ERROR && hybrid_args_check(1, 1, 1.f, w, &why) == EPS_USER_ERROR);
  std::printf("hybrid_host_check OK\n");
  return 0;
}
