// Stand-alone host check of csrc/multi_host.hpp - the argument and offset checks, the scratch cap with its refusal, and the plan of
// eps_index_search_multi - for a CPU build under -fsanitize=address,undefined (tests/test_multi_ref_cpu.py builds and runs it).  The plan is walked
// over a grid of (nq, t, k, G, n_cand, scratch) up to t = 1024 and G = 2^31 - 1: at every point the passes cover the bags in order without cutting
// one, a pass stays within the cap unless it is one bag alone, the read-back's wavefronts cover the columns and its lists stay bounded; on small
// points the tables of a pass are written into a heap block of exactly the planned size, the way the kernels index them: an element beyond the
// plan is a heap overflow the sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vectordb_amd/csrc/multi_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

static void arguments() {
  const char* why = nullptr;
  CHECK(multi_args_check(0, 1, 0, 0, &why) == EPS_OK);
  CHECK(multi_args_check(7, 1024, AMONG_MAX_CAND, 1, &why) == EPS_OK);
  CHECK(multi_args_check(-1, 1, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "nq"));
  CHECK(multi_args_check(1, 0, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k must"));
  CHECK(multi_args_check(1, 1025, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k must"));
  CHECK(multi_args_check(1, 1, -1, 0, &why) == EPS_USER_ERROR && strstr(why, "n_cand"));
  CHECK(multi_args_check(1, 1, AMONG_MAX_CAND + 1, 0, &why) == EPS_USER_ERROR && strstr(why, "n_cand"));
  CHECK(multi_args_check(1, 1, 0, -1, &why) == EPS_USER_ERROR && strstr(why, "scratch"));
}

static void bags() {
  const char* why = nullptr;
  int64_t total = -1, largest = -1;
  CHECK(multi_bags_check(nullptr, 0, &total, &largest, &why) == EPS_OK && total == 0 && largest == 0);   // (nothing is read)
  const int64_t ok[] = {0, 0, 3, 3, 1027, 1028};
  CHECK(multi_bags_check(ok, 5, &total, &largest, &why) == EPS_OK && total == 1028 && largest == 1024);
  const int64_t first[] = {1, 2};
  CHECK(multi_bags_check(first, 1, &total, &largest, &why) == EPS_USER_ERROR && strstr(why, "[0]"));
  const int64_t down[] = {0, 5, 4};
  CHECK(multi_bags_check(down, 2, &total, &largest, &why) == EPS_USER_ERROR && strstr(why, "non-decreasing"));
  const int64_t big[] = {0, 1025};
  CHECK(multi_bags_check(big, 1, &total, &largest, &why) == EPS_USER_ERROR && strstr(why, "1024"));
  std::vector<int64_t> many((size_t)(1 << 21) + 2);   // 2^21 bags of 1024 vectors: the total reaches 2^31
  for (size_t j = 0; j < many.size(); ++j) many[j] = (int64_t)j * 1024;
  CHECK(multi_bags_check(many.data(), (int64_t)many.size() - 1, &total, &largest, &why) == EPS_USER_ERROR && strstr(why, "2^31"));
  CHECK(multi_bags_check(many.data(), (int64_t)1 << 20, &total, &largest, &why) == EPS_OK && total == (int64_t)1 << 30);
}

static void scratch() {
  int64_t cap = 0;
  CHECK(multi_scratch_cap(0, 0, &cap) && cap == GROUPS_SCRATCH_DEFAULT);
  CHECK(multi_scratch_cap(0, GROUPS_SCRATCH_DEFAULT + 8, &cap) && cap == GROUPS_SCRATCH_DEFAULT + 8);   // the default grows to the largest bag
  const int64_t G = ((int64_t)1 << 31) - 1, t = 1024;
  const int64_t need = t * G * 8;   // 2^44 - 2^13: no overflow
  CHECK(need > 0 && multi_scratch_cap(0, need, &cap) && cap == need);
  CHECK(multi_scratch_cap(need, need, &cap) && cap == need);       // exactly at t x G x 8 = scratch: served
  CHECK(!multi_scratch_cap(need - 1, need, &cap));                 // one byte below: refused
  CHECK(multi_scratch_cap(need + 1, need, &cap) && cap == need + 1);
  CHECK(multi_scratch_cap(5, 0, &cap) && cap == 5);                // (nothing to hold: any cap serves)
  CHECK(multi_table_vectors(need, G) == t && multi_table_vectors(need - 1, G) == t - 1 && multi_table_vectors(8, 0) == 1);   // (no group: no division by zero)
  CHECK(multi_table_vectors((int64_t)1 << 40, 1) == GROUPS_SCAN_MAX_CHUNK);
}

// the passes of the whole-table form (cand = 0: columns = G) or the candidate form (every bag names n_cand candidates) over nq bags of the sizes
// `ts` cycles through; small = the tables are written too
static void walk(int64_t nq, const std::vector<int64_t>& ts, int32_t k, int64_t G, int64_t n_cand, bool cand, int64_t scratch_bytes, bool small) {
  std::vector<int64_t> qoff((size_t)nq + 1, 0), elems((size_t)nq + 1, 0), pairs((size_t)nq + 1, 0);
  int64_t largest = 0, t_max = 0;
  for (int64_t j = 0; j < nq; ++j) {
    const int64_t t = ts[(size_t)j % ts.size()];
    qoff[(size_t)j + 1] = qoff[(size_t)j] + t;
    pairs[(size_t)j + 1] = pairs[(size_t)j] + n_cand;
    elems[(size_t)j + 1] = elems[(size_t)j] + n_cand * t;
    t_max = t > t_max ? t : t_max;
    const int64_t own = (cand ? n_cand : G) * t * 8;
    largest = own > largest ? own : largest;
  }
  const char* why = nullptr;
  int64_t total = 0, big = 0;
  CHECK(multi_bags_check(qoff.data(), nq, &total, &big, &why) == EPS_OK && big == t_max);
  int64_t cap = 0;
  const bool served = multi_scratch_cap(scratch_bytes, largest, &cap);
  CHECK(served == (scratch_bytes == 0 || largest <= scratch_bytes));
  if (!served) return;
  CHECK(cap >= largest);
  const int64_t columns = cand ? n_cand : G;
  const MultiTopkPlan plan = multi_topk_plan(columns, k);
  CHECK(plan.W >= GROUPS_BLOCK_WAVES && plan.W % GROUPS_BLOCK_WAVES == 0 && plan.W <= GROUPS_TOPK_MAX_WAVES && plan.slice >= 1);
  CHECK((int64_t)plan.W * plan.slice >= columns);
  CHECK((int64_t)plan.W * k <= GROUPS_MERGE_KEYS || plan.W == GROUPS_BLOCK_WAVES);
  CHECK(plan.bags >= 1 && plan.bags <= MULTI_MAX_BAGS && plan.bags * plan.W * k * 8 <= GROUPS_LISTS_BYTES);
  const int64_t* cum = cand ? elems.data() : qoff.data();
  const int64_t cap_a = cand ? cap / 8 : multi_table_vectors(cap, G);
  int64_t expect = 0, passes = 0;
  for (int64_t j0 = 0; j0 < nq; ++passes) {
    const int64_t j1 = multi_slice_end(cum, cap_a, cand ? pairs.data() : nullptr, MULTI_MAX_PAIRS, nq, j0, plan.bags);
    CHECK(j0 == expect && j1 > j0 && j1 <= nq && j1 - j0 <= plan.bags);   // in order, whole bags, at least one
    const int64_t units = cum[j1] - cum[j0];
    CHECK(j1 - j0 == 1 || units <= cap_a);
    CHECK(units * (cand ? 1 : G) * 8 <= cap);                            // (a single bag fits too: it was not refused)
    if (!cand) CHECK(units <= GROUPS_SCAN_MAX_CHUNK);
    if (cand) CHECK(j1 - j0 == 1 || pairs[(size_t)j1] - pairs[(size_t)j0] <= MULTI_MAX_PAIRS);
    if (j1 < nq) {   // (the pass is full: the next bag would not have fitted)
      const bool room_a = cum[j1 + 1] - cum[j0] <= cap_a, room_b = !cand || pairs[(size_t)j1 + 1] - pairs[(size_t)j0] <= MULTI_MAX_PAIRS;
      CHECK(j1 - j0 == plan.bags || !room_a || !room_b);
    }
    if (small) {   // the table of the pass, indexed as the kernels index it
      std::vector<unsigned long long> table((size_t)(units * (cand ? 1 : G)), ~0ull);
      for (int64_t j = j0; j < j1; ++j) {
        const int64_t t = qoff[(size_t)j + 1] - qoff[(size_t)j];
        const int64_t base = (cum[j] - cum[j0]) * (cand ? 1 : G), su = cand ? 1 : G, sx = cand ? t : 1;
        for (int64_t u = 0; u < t; ++u)
          for (int64_t x = 0; x < columns; ++x) table[(size_t)(base + u * su + x * sx)] -= 1;
      }
      for (unsigned long long v : table) CHECK(v == ~0ull - 1);   // every element belongs to exactly one (bag, vector, column)
    }
    expect = j0 = j1;
  }
  CHECK(expect == nq && passes >= 1);
}

static void plans() {
  const int64_t Gs[] = {1, 2, 63, 1024, 1025, 100000, ((int64_t)1 << 31) - 1};
  const int32_t ks[] = {1, 10, 64, 65, 1024};
  const std::vector<std::vector<int64_t>> bag_sizes = {{1}, {0}, {1, 3, 4, 5, 9, 0}, {1024}, {1024, 0, 1}};
  for (int64_t nq : {1, 2, 7, 100, 40000})
    for (const auto& ts : bag_sizes)
      for (int32_t k : ks)
        for (int64_t G : Gs)
          for (int64_t scratch_bytes : {(int64_t)0, (int64_t)1, (int64_t)4096, (int64_t)1 << 20, (int64_t)1 << 45}) {
            if (nq > 100 && !((k == 1 || k == 1024) && (G == 1 || G == 1025 || G > 100000))) continue;   // (the long batches: the corners only)
            const bool small = nq <= 7 && G <= 1025 && k == 10;
            walk(nq, ts, k, G, 0, false, scratch_bytes, small);
            for (int64_t n_cand : {(int64_t)0, (int64_t)1, (int64_t)257, (int64_t)3000000})
              if (nq <= 100 || n_cand <= 257) walk(nq, ts, k, G, n_cand, true, scratch_bytes, small && n_cand <= 257);
          }
  // the refusal boundary on a walked point: t x G x 8 = scratch is served in passes of one bag, one byte less is refused
  walk(3, {1024}, 10, ((int64_t)1 << 31) - 1, 0, false, 1024 * (((int64_t)1 << 31) - 1) * 8, false);
  walk(3, {1024}, 10, ((int64_t)1 << 31) - 1, 0, false, 1024 * (((int64_t)1 << 31) - 1) * 8 - 1, false);
  walk(3, {5}, 10, 77, 0, false, 5 * 77 * 8, true);
  walk(3, {5}, 10, 77, 0, false, 5 * 77 * 8 - 1, true);
  walk(3, {5}, 10, 77, 13, true, 5 * 13 * 8, true);
  walk(3, {5}, 10, 77, 13, true, 5 * 13 * 8 - 1, true);
  // work items of a pair
  CHECK(multi_pair_items(1, 1) == 1 && multi_pair_items(256, 4) == 1 && multi_pair_items(257, 5) == 4 && multi_pair_items(513, 1024) == 3 * 256);
  CHECK(multi_pair_items(7, 0) == 0 && multi_pair_items(((int64_t)1 << 31) - 1, 1024) == ((int64_t)1 << 23) * 256);
}

int main() {
  arguments();
  bags();
  scratch();
  plans();
  if (failures) {
    printf("multi_host_check: %d FAILED\n", failures);
    return 1;
  }
  printf("multi_host_check OK\n");
  return 0;
}
