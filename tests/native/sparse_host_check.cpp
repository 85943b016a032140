// Stand-alone host check of csrc/sparse_host.hpp - the validation of CSR offsets and host-resident indices, the limits and the launch plan of
// eps_sparse_index_search - for a CPU build under -fsanitize=address,undefined (tests/test_sparse_ref_cpu.py builds and runs it).  Offsets and
// indices live in heap blocks exactly as long as the caller's arrays: an entry read outside them is a heap overflow the sanitizer reports.  Every
// wavefront of a plan takes its rows through sparse_wave_rows, the function the kernel calls: a row taken twice or never shows in the tally.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../vectordb_amd/csrc/sparse_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

struct Verdict {
  int32_t rc, kind;
  int64_t nnz, longest, bad;
};
static Verdict check_offsets(const std::vector<int64_t>& off, int64_t n) {
  int64_t* heap = static_cast<int64_t*>(malloc(off.size() * sizeof(int64_t) + 1));   // exactly n + 1 entries: one read further is caught
  for (size_t i = 0; i < off.size(); ++i) heap[i] = off[i];
  Verdict v;
  v.rc = sparse_offsets_check(off.empty() ? nullptr : heap, n, &v.nnz, &v.longest, &v.bad, &v.kind);
  CHECK((v.rc == EPS_OK) == (v.kind == SPARSE_BAD_NONE));
  CHECK((v.rc == EPS_OK) == (sparse_bad_text(v.kind)[0] == 0));
  free(heap);
  return v;
}
static Verdict check_rows(const std::vector<int64_t>& off, const std::vector<int32_t>& idx, int64_t dim) {
  int64_t* ho = static_cast<int64_t*>(malloc(off.size() * sizeof(int64_t) + 1));
  int32_t* hi = static_cast<int32_t*>(malloc(idx.size() * sizeof(int32_t) + 1));
  for (size_t i = 0; i < off.size(); ++i) ho[i] = off[i];
  for (size_t i = 0; i < idx.size(); ++i) hi[i] = idx[i];
  Verdict v{};
  v.rc = sparse_rows_check(ho, hi, (int64_t)off.size() - 1, dim, &v.bad, &v.kind);
  free(ho);
  free(hi);
  return v;
}

static void offsets() {
  Verdict v = check_offsets({0, 3, 3, 10}, 3);
  CHECK(v.rc == EPS_OK && v.nnz == 10 && v.longest == 7 && v.bad == -1);
  v = check_offsets({0}, 0);                                   // n = 0: one entry
  CHECK(v.rc == EPS_OK && v.nnz == 0 && v.longest == 0);
  v = check_offsets({0, 0}, 1);                                // n = 1, an empty row
  CHECK(v.rc == EPS_OK && v.nnz == 0 && v.longest == 0);
  v = check_offsets({0, 5}, 1);
  CHECK(v.rc == EPS_OK && v.nnz == 5 && v.longest == 5);
  v = check_offsets({1, 3, 10}, 2);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_FIRST && v.bad == 0);
  v = check_offsets({-1, 3, 10}, 2);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_FIRST && v.bad == 0);
  v = check_offsets({0, 4, 3, 10}, 3);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_OFFSETS && v.bad == 1);
  v = check_offsets({0, 4, 6, -2}, 3);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_OFFSETS && v.bad == 2);
  v = check_offsets({0, -4, 10}, 2);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_OFFSETS && v.bad == 0);
  v = check_offsets({7}, 0);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_FIRST);
  v = check_offsets({}, 3);                                    // no array at all
  CHECK(v.rc == EPS_USER_ERROR);
  v = check_offsets({0, 1}, -1);
  CHECK(v.rc == EPS_USER_ERROR);
  v = check_offsets({0, (int64_t)1 << 40, (int64_t)1 << 41}, 2);   // more elements than an int holds
  CHECK(v.rc == EPS_OK && v.nnz == (int64_t)1 << 41 && v.longest == (int64_t)1 << 40);
}

static void rows() {
  const int64_t top = SPARSE_MAX_DIM;
  Verdict v = check_rows({0, 3, 3, 5}, {0, 5, 9, 2, 2147483646}, top);
  CHECK(v.rc == EPS_OK && v.bad == -1);
  v = check_rows({0, 3, 3, 5}, {0, 5, 9, 2, 2147483646}, top - 1);   // an index equal to dim
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_RANGE && v.bad == 2);
  v = check_rows({0, 2, 4}, {1, 2, -1, 3}, 10);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_RANGE && v.bad == 1);
  v = check_rows({0, 2, 4}, {1, 2, 3, 3}, 10);                 // a repeated index
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_ORDER && v.bad == 1);
  v = check_rows({0, 3}, {4, 2, 9}, 10);
  CHECK(v.rc == EPS_USER_ERROR && v.kind == SPARSE_BAD_ORDER && v.bad == 0);
  v = check_rows({0, 2, 4}, {5, 9, 0, 5}, 10);                 // the order starts again with every row
  CHECK(v.rc == EPS_OK);
  v = check_rows({0, 0, 0}, {}, 1);                            // empty rows are accepted
  CHECK(v.rc == EPS_OK);
  v = check_rows({0, 1}, {0}, 1);
  CHECK(v.rc == EPS_OK);
}

static void limits() {
  CHECK(SPARSE_MAX_K == 1024 && SPARSE_MAX_ROWS == 2147483647 && SPARSE_MAX_DIM == 2147483647);
  CHECK(SPARSE_MAX_QUERY_NNZ >= 4096);
  CHECK(SPARSE_MAX_QUERY_NNZ * 8 + SPARSE_STATIC_LDS <= SPARSE_LDS_BUDGET);    // one query of the longest kind fits next to the pieces
  CHECK(SPARSE_LDS_BUDGET <= 160 * 1024 && 2 * SPARSE_LDS_BUDGET <= 160 * 1024);
  CHECK(SPARSE_STATIC_LDS >= 4 * 8);   // four staged queries: a length and a norm each
  CHECK(SPARSE_BLOCK_WAVES == AMONG_BLOCK_WAVES && SPARSE_PIECE % SPARSE_WAVE_ROWS == 0);
}

static void plans() {
  const int64_t ns[] = {0, 1, 63, 64, 65, 130, 257, 1000, 20000, 1000000, 100000000, SPARSE_MAX_ROWS};
  const int ks[] = {1, 10, 64, 65, 128, 129, 1024};
  const int64_t nqs[] = {1, 2, 3, 5, 33, 1024, 100000};
  const int64_t qls[] = {0, 1, 32, 1500, 1501, 3000, SPARSE_MAX_QUERY_NNZ};
  for (int64_t n : ns)
    for (int k : ks)
      for (int64_t nq : nqs)
        for (int64_t ql : qls) {
          const SparsePlan p = sparse_plan(n, nq, k, ql);
          CHECK(p.nq_tile == 1 || p.nq_tile == 2 || p.nq_tile == 4);
          CHECK(k <= 128 || p.nq_tile == 1);
          CHECK(p.qcap >= ql && p.qcap >= 4 && p.qcap % 4 == 0);
          CHECK(p.lds_dynamic == p.nq_tile * p.qcap * 8 && p.lds_dynamic + SPARSE_STATIC_LDS <= SPARSE_LDS_BUDGET);
          CHECK(p.tiles == (nq + p.nq_tile - 1) / p.nq_tile);
          CHECK(p.W >= SPARSE_BLOCK_WAVES && p.W % SPARSE_BLOCK_WAVES == 0);
          CHECK(p.rows_per_wave >= SPARSE_WAVE_ROWS && p.rows_per_wave % SPARSE_WAVE_ROWS == 0);
          CHECK((int64_t)p.W * p.rows_per_wave >= n);
          const int64_t blocks = p.W / SPARSE_BLOCK_WAVES;
          CHECK(blocks == 1 || (blocks * p.tiles <= SPARSE_MAX_BLOCKS && (int64_t)p.W * k <= AMONG_MERGE_KEYS));   // the merge's key budget
          CHECK(blocks <= 65535);
          CHECK((double)nq * p.W * k * 8.0 < 9.0e18);   // the partial lists' byte count stays inside an int64
          if (nq == 1 && k == 10 && n >= 1000000) CHECK(blocks >= 1024);   // one query, a long table: enough workgroups to fill the device
          // every row once: the wavefronts' ranges follow one another and end at n
          int64_t next = 0;
          for (int64_t w = 0; w < p.W; ++w) {
            int64_t b = -1, e = -1;
            sparse_wave_rows(p, n, w, &b, &e);
            CHECK(0 <= b && b <= e && e <= n && e - b <= p.rows_per_wave);
            CHECK(b == next || (b == n && e == n));
            CHECK(b == n || b % SPARSE_WAVE_ROWS == 0);
            next = e;
          }
          CHECK(next == n);
        }
  // a table behind real offsets: every wavefront reads its rows' offsets inside the n + 1 entries, and the rounds' element ranges tile [0, nnz)
  const int64_t n = 1000;
  int64_t* off = static_cast<int64_t*>(malloc((size_t)(n + 1) * sizeof(int64_t)));
  off[0] = 0;
  for (int64_t r = 0; r < n; ++r) off[r + 1] = off[r] + (r * 7) % 13;
  const SparsePlan p = sparse_plan(n, 3, 10, 32);
  int64_t covered = 0;
  for (int64_t w = 0; w < p.W; ++w) {
    int64_t b, e;
    sparse_wave_rows(p, n, w, &b, &e);
    for (int64_t r0 = b; r0 < e; r0 += SPARSE_WAVE_ROWS) {
      const int64_t r1 = r0 + SPARSE_WAVE_ROWS < e ? r0 + SPARSE_WAVE_ROWS : e;
      CHECK(off[r0] == covered);
      covered = off[r1];
    }
  }
  CHECK(covered == off[n]);
  free(off);
}

int main() {
  offsets();
  rows();
  limits();
  plans();
  if (failures) {
    printf("sparse_host_check: %d check(s) failed\n", failures);
    return 1;
  }
  printf("sparse_host_check OK\n");
  return 0;
}
