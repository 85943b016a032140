// Host side of the grouped search with m rows per group (eps_index_search_group_rows; kernels: group_rows.hip): the call's argument checks and the
// plan of its second phase - how many rows of a group one wavefront walks (chunk), how many queries one pass serves (slice) and the bound on the
// work items, hence on the partial lists, of such a pass.  Plain C++ with no HIP type in it: tests/native/group_rows_host_check.cpp runs it under
// a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "groups_host.hpp"

namespace eps {

constexpr int32_t GROUP_ROWS_MAX_M = 1024;                 // the widest WaveTopK (KPL = 16)
constexpr int64_t GROUP_ROWS_MAX_ANSWER = 65536;           // k * m at most: 768 KiB of answer per query
constexpr int64_t GROUP_ROWS_CHUNK = 256;                  // rows of a group one wavefront walks, unless a bound below asks for more
constexpr int64_t GROUP_ROWS_MAX_PAIRS = (int64_t)1 << 20; // (query, slot) pairs of one pass: what the work list's one workgroup scans
constexpr int64_t GROUP_ROWS_MAX_WAVES = 4096;             // workgroups (of one wavefront) of the gather at most: they stride over the work list

// EPS_OK, or EPS_USER_ERROR with the reason in *why
inline int32_t group_rows_args_check(int64_t nq, int32_t k, int32_t m, int32_t engine, int32_t page_rows, int64_t scratch_bytes, const char** why) {
  if (groups_args_check(nq, k, engine, page_rows, scratch_bytes, why) != EPS_OK) return EPS_USER_ERROR;
  if (m < 1 || m > GROUP_ROWS_MAX_M) return *why = "m must be in [1, 1024]", EPS_USER_ERROR;
  if ((int64_t)k * m > GROUP_ROWS_MAX_ANSWER) return *why = "k * m must be <= 65536", EPS_USER_ERROR;
  return EPS_OK;
}

// work items of `nq` queries at most: every (query, slot) pair has ceil(size / chunk) <= 1 + size / chunk of them, and the k groups of a query
// hold min(n, k * largest) rows at most.  (nq <= 2^20, n < 2^31, k * largest < 2^41: no overflow)
inline int64_t group_rows_items_bound(int64_t nq, int32_t k, int64_t n, int64_t largest, int64_t chunk) {
  const int64_t rows = n < (int64_t)k * largest ? n : (int64_t)k * largest;
  return nq * k + nq * rows / chunk;
}

struct GroupRowsPlan {
  int64_t chunk;    // rows of a group per work item, >= 1
  int64_t slice;    // queries of one pass, >= 1
  int64_t passes;   // ceil(nq / slice)
  int64_t items;    // the bound on the work items of one pass: the partial lists hold items * m keys
  int64_t waves;    // wavefronts of the gather's grid, >= 1
};
// nq > 0 queries, checked arguments, n > 0 rows, 1 <= largest <= n.  chunk: the rows that keep a pair's partial lists within what the merge's one
// workgroup is given (GROUPS_MERGE_KEYS) and one query's lists within GROUPS_LISTS_BYTES; slice: the queries whose lists fit GROUPS_LISTS_BYTES.
inline GroupRowsPlan group_rows_plan(int64_t nq, int32_t k, int32_t m, int64_t n, int64_t largest) {
  GroupRowsPlan p;
  const int64_t cap_items = GROUPS_LISTS_BYTES / ((int64_t)m * 8);   // >= 65536 > k
  const int64_t rows = n < (int64_t)k * largest ? n : (int64_t)k * largest;
  int64_t chunk = GROUP_ROWS_CHUNK;
  const int64_t lists = GROUPS_MERGE_KEYS / m;   // partial lists of one pair at most (>= 256)
  const int64_t for_merge = (largest + lists - 1) / lists;
  chunk = chunk > for_merge ? chunk : for_merge;
  const int64_t room = cap_items - k;            // items one query may have beyond one per pair
  const int64_t for_cap = (rows + room - 1) / room;
  chunk = chunk > for_cap ? chunk : for_cap;
  p.chunk = chunk;
  int64_t slice = GROUP_ROWS_MAX_PAIRS / k;
  slice = slice < nq ? slice : nq;
  while (slice > 1 && group_rows_items_bound(slice, k, n, largest, chunk) > cap_items) slice = (slice + 1) / 2;
  p.slice = slice;
  p.passes = (nq + slice - 1) / slice;
  p.items = group_rows_items_bound(slice, k, n, largest, chunk);
  p.waves = p.items < GROUP_ROWS_MAX_WAVES ? p.items : GROUP_ROWS_MAX_WAVES;
  return p;
}

}  // namespace eps
