// Stand-alone host check of csrc/groups_host.hpp - the relabelling of eps_index_set_groups, the argument checks and the plan of
// eps_index_search_groups - for a CPU build under -fsanitize=address,undefined (tests/test_groups_ref_cpu.py builds and runs it).  The caller's
// arrays live in heap blocks exactly as long as the call says they are, and the plan's chunks and slices are walked the way the host loop and
// the read-back kernel walk them: a slot outside the table is a heap overflow the sanitizer reports, one read twice or never shows in the tally.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vectordb_amd/csrc/groups_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

// relabels keys held in a heap block of exactly n entries into a label block of exactly n entries
static int64_t relabel(const std::vector<int64_t>& keys, std::vector<int32_t>* label, std::vector<int64_t>* kol, int64_t* largest) {
  const size_t n = keys.size();
  int64_t* hk = static_cast<int64_t*>(malloc(n * sizeof(int64_t) + 1));
  int32_t* hl = static_cast<int32_t*>(malloc(n * sizeof(int32_t) + 1));
  if (n) memcpy(hk, keys.data(), n * sizeof(int64_t));
  const int64_t G = groups_relabel(hk, (int64_t)n, hl, kol, largest);
  label->assign(hl, hl + n);
  free(hk);
  free(hl);
  return G;
}

static void relabelling() {
  std::vector<int32_t> label;
  std::vector<int64_t> kol;
  int64_t largest = -1;
  const int64_t lo = INT64_MIN, hi = INT64_MAX;
  CHECK(relabel({hi, lo, -1, 0, lo, hi, hi, 7}, &label, &kol, &largest) == 5 && largest == 3);
  CHECK((kol == std::vector<int64_t>{lo, -1, 0, 7, hi}));
  CHECK((label == std::vector<int32_t>{4, 0, 1, 2, 0, 4, 4, 3}));
  CHECK(relabel({}, &label, &kol, &largest) == 0 && largest == 0 && label.empty() && kol.empty());   // an empty table
  CHECK(relabel({5}, &label, &kol, &largest) == 1 && largest == 1 && label[0] == 0 && kol[0] == 5);
  CHECK(relabel({9, 9, 9, 9}, &label, &kol, &largest) == 1 && largest == 4);                          // one group
  // every row its own group, non-contiguous keys in descending order: label = n - 1 - row
  std::vector<int64_t> keys;
  for (int64_t i = 0; i < 1000; ++i) keys.push_back(hi - i * 1000003);
  CHECK(relabel(keys, &label, &kol, &largest) == 1000 && largest == 1);
  bool ok = true;
  for (int64_t i = 0; i < 1000; ++i) ok = ok && label[(size_t)i] == 999 - i && kol[(size_t)label[(size_t)i]] == keys[(size_t)i];
  CHECK(ok);
}

static void arguments() {
  const char* why = nullptr;
  CHECK(groups_args_check(0, 1, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_OK && why[0] == 0);
  CHECK(groups_args_check(5, 1024, EPS_GROUPS_SCAN, 1024, (int64_t)1 << 40, &why) == EPS_OK);
  CHECK(groups_args_check(5, 1, EPS_GROUPS_PAGES, 1, 1, &why) == EPS_OK);
  CHECK(groups_args_check(-1, 1, 0, 0, 0, &why) == EPS_USER_ERROR && why[0] != 0);
  CHECK(groups_args_check(1, 0, 0, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k must be"));
  CHECK(groups_args_check(1, 1025, 0, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k must be"));
  CHECK(groups_args_check(1, 1, 3, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "engine"));
  CHECK(groups_args_check(1, 1, -1, 0, 0, &why) == EPS_USER_ERROR);
  CHECK(groups_args_check(1, 1, 0, 1025, 0, &why) == EPS_USER_ERROR && strstr(why, "page_rows"));
  CHECK(groups_args_check(1, 1, 0, -1, 0, &why) == EPS_USER_ERROR);
  CHECK(groups_args_check(1, 1, 0, 0, -1, &why) == EPS_USER_ERROR && strstr(why, "scratch_bytes"));
  CHECK(groups_page_rows(1, 0) == 64 && groups_page_rows(16, 0) == 64 && groups_page_rows(17, 0) == 128 && groups_page_rows(256, 0) == 1024);
  CHECK(groups_page_rows(1024, 0) == 1024 && groups_page_rows(10, 16) == 16 && groups_page_rows(1024, 1) == 1);
  CHECK(GROUPS_LDS_SLOTS >= 2 * (GROUPS_MAX_K + GROUPS_MAX_PAGE) && (GROUPS_LDS_SLOTS & (GROUPS_LDS_SLOTS - 1)) == 0);   // the probe always ends
}

// walks a plan as search_groups and groups_table_topk_kernel do: every query in exactly one chunk, every slot of a chunk's table read once
static void walk(int64_t m, int64_t G, int32_t k, int64_t scratch) {
  const GroupsScanPlan p = groups_scan_plan(m, G, k, scratch);
  CHECK(p.c >= GROUPS_SCAN_NQ && p.c % GROUPS_SCAN_NQ == 0 && p.c <= GROUPS_SCAN_MAX_CHUNK);
  CHECK(p.chunks == (m + p.c - 1) / p.c);
  CHECK(p.W >= GROUPS_BLOCK_WAVES && p.W % GROUPS_BLOCK_WAVES == 0 && (int64_t)p.W * p.slice >= G);
  CHECK(p.W == GROUPS_BLOCK_WAVES || (int64_t)p.W * k <= GROUPS_MERGE_KEYS);
  const int64_t cap = scratch > 0 ? scratch : GROUPS_SCRATCH_DEFAULT;
  CHECK(p.c == GROUPS_SCAN_NQ || groups_table_bytes(p, G) <= cap);   // (never below one tile of 4 queries, whatever the cap)
  int64_t served = 0;
  for (int64_t i0 = 0; i0 < m; i0 += p.c) {
    const int64_t mc = p.c < m - i0 ? p.c : m - i0;
    served += mc;
    if (mc * G > ((int64_t)1 << 22)) continue;   // (large tables: the arithmetic above only)
    unsigned char* table = static_cast<unsigned char*>(calloc((size_t)(mc * G), 1));   // exactly mc * G slots
    for (int64_t i = 0; i < mc; ++i)
      for (int64_t w = 0; w < p.W; ++w) {
        const int64_t begin = w * p.slice < G ? w * p.slice : G;
        const int64_t end = G - begin < p.slice ? G : begin + p.slice;
        for (int64_t s = begin; s < end; ++s) table[i * G + s] += 1;
      }
    bool once = true;
    for (int64_t s = 0; s < mc * G; ++s) once = once && table[s] == 1;
    CHECK(once);
    free(table);
  }
  CHECK(served == m);
}

static void plans() {
  for (int64_t m : {1, 3, 4, 5, 9, 64, 1000})
    for (int64_t G : {1, 2, 255, 256, 257, 1024, 1025, 3000, 40000})
      for (int32_t k : {1, 10, 64, 65, 1024})
        for (int64_t scratch : {(int64_t)0, (int64_t)1, G * 8, 4 * G * 8, 4 * G * 8 + 7, 8 * G * 8, (int64_t)1 << 40}) walk(m, G, k, scratch);
  walk(100000, 1 << 20, 10, 0);
  walk(3, ((int64_t)1 << 31) - 1, 1024, 0);   // the largest table: no overflow in the byte counts
  // nq = 9 with room for 4 queries: three chunks of 4, 4, 1
  GroupsScanPlan p = groups_scan_plan(9, 375, 7, 4 * 375 * 8);
  CHECK(p.c == 4 && p.chunks == 3);
  p = groups_scan_plan(9, 375, 7, 1);   // below one chunk: still 4
  CHECK(p.c == 4 && p.chunks == 3);
  p = groups_scan_plan(9, 375, 7, 0);   // the default holds all nine: two tiles of 4 and a third chunk of 1
  CHECK(p.c == 8 && p.chunks == 2);
  p = groups_scan_plan(3, 375, 7, 0);   // nq not a multiple of 4
  CHECK(p.c == 4 && p.chunks == 1);
}

int main() {
  relabelling();
  arguments();
  plans();
  if (failures) {
    printf("groups_host_check: %d failures\n", failures);
    return 1;
  }
  printf("groups_host_check OK\n");
  return 0;
}
