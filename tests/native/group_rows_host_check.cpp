// Stand-alone host check of csrc/group_rows_host.hpp - the argument checks and the plan of eps_index_search_group_rows - for a CPU build under
// -fsanitize=address,undefined (tests/test_group_rows_ref_cpu.py builds and runs it).  The plan is walked over a grid of (nq, k, m, n, largest):
// at every point the bound on the work items, the cap on the partial lists, what the merge's one workgroup is given and chunk >= 1 are asserted;
// on small points the work list is built the way the device builds it - ceil(size / chunk) per pair - for the worst groups the inputs allow, and
// every list is written into a heap block of exactly the planned size: an item beyond the bound is a heap overflow the sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vectordb_amd/csrc/group_rows_host.hpp"

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
  CHECK(group_rows_args_check(0, 1, 1, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_OK);
  CHECK(group_rows_args_check(5, 1024, 64, EPS_GROUPS_SCAN, 1024, 1, &why) == EPS_OK);   // k * m = 65536
  CHECK(group_rows_args_check(5, 64, 1024, EPS_GROUPS_PAGES, 0, 0, &why) == EPS_OK);
  CHECK(group_rows_args_check(5, 1, 1024, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_OK);
  CHECK(group_rows_args_check(5, 7, 0, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "m must"));
  CHECK(group_rows_args_check(5, 7, -1, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR);
  CHECK(group_rows_args_check(5, 1, 1025, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "m must"));
  CHECK(group_rows_args_check(5, 65537, 1, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k must"));
  CHECK(group_rows_args_check(5, 1024, 65, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k * m"));
  CHECK(group_rows_args_check(5, 257, 256, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "k * m"));   // 65792
  CHECK(group_rows_args_check(5, 0, 1, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR);
  CHECK(group_rows_args_check(-1, 1, 1, EPS_GROUPS_AUTO, 0, 0, &why) == EPS_USER_ERROR);
  CHECK(group_rows_args_check(5, 1, 1, 3, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "engine"));
  CHECK(group_rows_args_check(5, 1, 1, EPS_GROUPS_AUTO, 1025, 0, &why) == EPS_USER_ERROR);
  CHECK(group_rows_args_check(5, 1, 1, EPS_GROUPS_AUTO, 0, -1, &why) == EPS_USER_ERROR);
}

static int64_t points = 0, walked = 0;

static void point(int64_t nq, int32_t k, int32_t m, int64_t n, int64_t largest) {
  const GroupRowsPlan p = group_rows_plan(nq, k, m, n, largest);
  ++points;
  CHECK(p.chunk >= 1);
  CHECK(p.slice >= 1 && p.slice <= nq && p.slice * k <= GROUP_ROWS_MAX_PAIRS);
  CHECK(p.passes == (nq + p.slice - 1) / p.slice);
  CHECK(p.items == group_rows_items_bound(p.slice, k, n, largest, p.chunk));
  CHECK(p.items >= p.slice * k);
  CHECK(p.items * m * 8 <= GROUPS_LISTS_BYTES);                                    // the 512 MiB cap
  CHECK(((largest + p.chunk - 1) / p.chunk) * m <= GROUPS_MERGE_KEYS + m);         // one pair's lists: what the merge's one workgroup is given
  CHECK(p.waves >= 1 && p.waves <= GROUP_ROWS_MAX_WAVES && p.waves <= p.items);
  // the worst a pass can meet: every query's k groups as large as the inputs allow
  const int64_t rows = n < (int64_t)k * largest ? n : (int64_t)k * largest;
  int64_t per_query = 0, left = rows;
  for (int s = 0; s < k && left > 0; ++s) {
    const int64_t size = left < largest ? left : largest;
    per_query += (size + p.chunk - 1) / p.chunk;
    left -= size;
  }
  CHECK(p.slice * per_query <= p.items);
  // ... and with groups of one row above a multiple of the chunk, the most chunks per row
  if (p.chunk + 1 <= largest && (int64_t)k * (p.chunk + 1) <= rows) CHECK(p.slice * 2 * k <= p.items);
  if (p.items * m > ((int64_t)1 << 16) || p.slice * k > 4096) return;
  // small: build the work list as the device does and touch every partial list's keys in a block of exactly the planned size
  ++walked;
  uint64_t* partial = static_cast<uint64_t*>(malloc((size_t)(p.items * m) * sizeof(uint64_t) + 1));
  std::vector<uint32_t> prefix((size_t)(p.slice * k) + 1);
  uint32_t base = 0;
  for (int64_t q = 0; q < p.slice; ++q) {
    int64_t rest = rows;
    for (int s = 0; s < k; ++s) {
      const int64_t size = rest < largest ? rest : largest;
      rest -= size;
      prefix[(size_t)(q * k + s)] = base;
      base += (uint32_t)((size + p.chunk - 1) / p.chunk);
    }
  }
  prefix[(size_t)(p.slice * k)] = base;
  CHECK((int64_t)base <= p.items);
  for (int64_t item = 0; item < (int64_t)base; ++item) {
    int64_t lo = 0, hi = p.slice * k;   // the gather's search
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)prefix[(size_t)mid] <= item) lo = mid; else hi = mid;
    }
    CHECK((int64_t)prefix[(size_t)lo] <= item && item < (int64_t)prefix[(size_t)lo + 1]);
    for (int e = 0; e < m; ++e) partial[item * m + e] = (uint64_t)lo;
  }
  free(partial);
}

int main() {
  arguments();
  const int64_t N31 = ((int64_t)1 << 31) - 1;
  const int64_t nqs[] = {1, 2, 3, 64, 1000, 1024, 32768, 1000000};
  const int32_t ks[] = {1, 2, 7, 10, 64, 65, 1024};
  const int32_t ms[] = {1, 2, 3, 7, 64, 65, 256, 1024};
  const int64_t ns[] = {1, 2, 65, 255, 256, 257, 3000, 1000000, N31};
  for (int64_t nq : nqs)
    for (int32_t k : ks)
      for (int32_t m : ms) {
        if ((int64_t)k * m > GROUP_ROWS_MAX_ANSWER) continue;
        for (int64_t n : ns) {
          const int64_t largests[] = {1, 2, 8, 255, 256, 257, 511, 512, 513, n / 2, n - 1, n};
          for (int64_t largest : largests)
            if (largest >= 1 && largest <= n) point(nq, k, m, n, largest);
        }
      }
  point(1, 1024, 64, N31, N31);   // k * m = 65536, one group owns a table of 2^31 - 1 rows
  point(1, 64, 1024, N31, N31);
  point(1000000, 1024, 64, N31, N31);
  point(1, 1, 1, 1, 1);
  CHECK(points > 10000 && walked > 1000);
  // a table in one group is spread over many work items, not given to one
  CHECK(group_rows_plan(1, 10, 3, 1000000, 1000000).chunk == GROUP_ROWS_CHUNK);
  CHECK(group_rows_plan(1, 10, 1024, 1000000, 1000000).chunk == 3907);   // (the merge's keys: 2^18 / 1024 = 256 lists, ceil(1000000 / 256) rows each)
  if (failures) {
    printf("group_rows_host_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("group_rows_host_check OK (%lld points, %lld walked)\n", (long long)points, (long long)walked);
  return 0;
}
