// Stand-alone host check of csrc/among_host.hpp - the validation of the per-query offsets and the launch plan of eps_index_search_among - for a CPU
// build under -fsanitize=address,undefined (tests/test_among_ref_cpu.py builds and runs it).  The lists live in heap blocks exactly as long as
// the caller's arrays, and every wavefront of the plan reads its chunk through among_chunk, the function the kernel calls: an entry outside its
// list is a heap overflow the sanitizer reports, an entry read twice or never shows in the tally.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../vectordb_amd/csrc/among_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

static int pick_nq(int64_t nq, int k) { return k > 128 ? 1 : (nq >= 3 ? 4 : (nq == 2 ? 2 : 1)); }   // (kernels.hpp, rows of <= 4096 floats)

static int32_t check(const std::vector<int64_t>& off, int64_t nq, int64_t n_cand, int64_t* longest) {
  const char* why = nullptr;
  int64_t* heap = static_cast<int64_t*>(malloc(off.size() * sizeof(int64_t) + 1));   // exactly nq + 1 entries: one read further is caught
  for (size_t i = 0; i < off.size(); ++i) heap[i] = off[i];
  const int32_t rc = among_lists_check(off.empty() ? nullptr : heap, nq, n_cand, longest, &why);
  CHECK(why != nullptr && (rc == EPS_OK) == (why[0] == 0));
  free(heap);
  return rc;
}

static void offsets() {
  int64_t longest = -1;
  CHECK(check({0, 3, 3, 10}, 3, 10, &longest) == EPS_OK && longest == 7);
  CHECK(check({0, 0, 0, 0}, 3, 0, &longest) == EPS_OK && longest == 0);        // empty lists
  CHECK(check({0, 5}, 1, 5, &longest) == EPS_OK && longest == 5);
  CHECK(check({0, 0, 5}, 2, 5, &longest) == EPS_OK && longest == 5);
  CHECK(check({1, 3, 10}, 2, 10, &longest) == EPS_USER_ERROR);                 // offsets[0] != 0
  CHECK(check({0, 4, 3, 10}, 3, 10, &longest) == EPS_USER_ERROR);              // decreasing
  CHECK(check({0, 4, 9}, 2, 10, &longest) == EPS_USER_ERROR);                  // offsets[nq] < n_cand
  CHECK(check({0, 4, 11}, 2, 10, &longest) == EPS_USER_ERROR);                 // offsets[nq] > n_cand
  CHECK(check({0, 12, 10}, 2, 10, &longest) == EPS_USER_ERROR);                // beyond n_cand in the middle
  CHECK(check({-1, 4, 10}, 2, 10, &longest) == EPS_USER_ERROR);
  CHECK(check({0, -4, 10}, 2, 10, &longest) == EPS_USER_ERROR);
  CHECK(check({}, 5, 17, &longest) == EPS_OK && longest == 17);                // one list for every query
  CHECK(check({}, 5, 0, &longest) == EPS_OK && longest == 0);
  CHECK(check({}, 5, -1, &longest) == EPS_USER_ERROR);
  CHECK(check({}, -1, 5, &longest) == EPS_USER_ERROR);
  CHECK(check({}, 1, AMONG_MAX_CAND, &longest) == EPS_OK && longest == AMONG_MAX_CAND);
  CHECK(check({}, 1, AMONG_MAX_CAND + 1, &longest) == EPS_USER_ERROR);
  CHECK(check({0, AMONG_MAX_CAND}, 1, AMONG_MAX_CAND, &longest) == EPS_OK && longest == AMONG_MAX_CAND);   // (planned below, never allocated)
  CHECK(check({7}, 0, 3, &longest) == EPS_OK);                                 // nq = 0: nothing is read
  CHECK(AMONG_MAX_CAND == 2147483647 && AMONG_MAX_K == 1024);
}

// every wavefront's chunk of a list of `len` entries: inside the list, one after the other, all of it
static void walk(const AmongPlan& p, const int64_t* list, int64_t len, bool read) {
  int64_t next = 0, sum = 0;
  for (int64_t w = 0; w < p.W; ++w) {
    int64_t b = -1, e = -1;
    among_chunk(len, p.chunk, w, &b, &e);
    CHECK(0 <= b && b <= e && e <= len && e - b <= p.chunk);
    CHECK(b == next || (b == len && e == len));
    next = e;
    if (read)
      for (int64_t i = b; i < e; ++i) sum += list[i];
  }
  CHECK(next == len);
  if (read) CHECK(sum == len * (len - 1) / 2);   // (list[i] = i: every entry exactly once)
}

static void plans() {
  const int64_t lens[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1000, 4096, 20000, 100000, 10000000, AMONG_MAX_CAND};
  const int ks[] = {1, 10, 64, 65, 130, 1024};
  const int64_t nqs[] = {1, 2, 3, 5, 70, 1024, 100000};
  for (int64_t longest : lens)
    for (int k : ks)
      for (int64_t nq : nqs)
        for (int shared = 0; shared < 2; ++shared) {
          const AmongPlan p = among_plan(shared != 0, nq, longest, k, pick_nq(nq, k));
          CHECK(p.nq_tile == (shared ? pick_nq(nq, k) : 1));
          CHECK(p.tiles == (nq + p.nq_tile - 1) / p.nq_tile);
          CHECK(p.W >= AMONG_BLOCK_WAVES && p.W % AMONG_BLOCK_WAVES == 0 && p.chunk >= 1);
          CHECK((int64_t)p.W * p.chunk >= longest);
          const int64_t blocks = p.W / AMONG_BLOCK_WAVES;
          CHECK(blocks == 1 || (blocks * p.tiles <= AMONG_MAX_BLOCKS && (int64_t)p.W * k <= AMONG_MERGE_KEYS));
          CHECK(blocks == 1 || (blocks - 1) * AMONG_BLOCK_WAVES * AMONG_WAVE_MIN < longest);   // no workgroup for fewer than 32 entries per wavefront
          CHECK((double)nq * p.W * k * 8.0 < 9.0e18);   // the partial lists' byte count stays inside an int64
          if (nq == 1 && k == 10 && longest >= 1000000) CHECK(blocks >= 1024);   // one query, a long list: enough workgroups to fill the chip
          // a list of the longest length, and shorter ones of the same launch (per-query lists: wavefronts beyond the end get nothing)
          for (int64_t len : {longest, longest / 2, longest / 3 + 1, (int64_t)1, (int64_t)0}) {
            if (len > longest) continue;
            if (len <= 20000) {
              int64_t* list = static_cast<int64_t*>(malloc((size_t)len * sizeof(int64_t) + 1));
              for (int64_t i = 0; i < len; ++i) list[i] = i;
              walk(p, list, len, true);
              free(list);
            } else {
              walk(p, nullptr, len, false);
            }
          }
        }
  // the plan of per-query lists behind real offsets: each query's chunks stay inside ITS slice of the concatenated array
  const std::vector<int64_t> off = {0, 0, 1, 8, 8, 24, 25, 1025, 1025};
  const int64_t nq = (int64_t)off.size() - 1, n_cand = off.back();
  int64_t longest = 0;
  const char* why;
  CHECK(among_lists_check(off.data(), nq, n_cand, &longest, &why) == EPS_OK && longest == 1000);
  int64_t* ids = static_cast<int64_t*>(malloc((size_t)n_cand * sizeof(int64_t)));
  for (int64_t j = 0; j < nq; ++j)
    for (int64_t i = off[j]; i < off[j + 1]; ++i) ids[i] = i - off[j];
  const AmongPlan p = among_plan(false, nq, longest, 10, 4);
  CHECK(p.nq_tile == 1 && p.tiles == nq);
  for (int64_t j = 0; j < nq; ++j) walk(p, ids + off[j], off[j + 1] - off[j], true);
  free(ids);
}

int main() {
  offsets();
  plans();
  if (failures) {
    printf("among_host_check: %d check(s) failed\n", failures);
    return 1;
  }
  printf("among_host_check OK\n");
  return 0;
}
