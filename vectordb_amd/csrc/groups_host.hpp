// Host side of the grouped search (eps_index_set_groups, eps_index_search_groups; kernels: groups.hip): the relabelling of the caller's int64 keys
// to dense int32 labels, the call's argument checks and its plan - the page size, how many queries share the scan engine's table and how that
// table is cut among the wavefronts that read it back.  Plain C++ with no HIP type in it: tests/native/groups_host_check.cpp runs it under a
// sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/epsilla_gfx950.h"

namespace eps {

constexpr int32_t GROUPS_MAX_K = 1024;                           // the widest WaveTopK (KPL = 16)
constexpr int32_t GROUPS_MAX_PAGE = 1024;                        // keys of a page: what one flat search returns per query
constexpr int GROUPS_LDS_SLOTS = 4096;                           // open-addressing slots of groups_first_kernel: <= 1024 carried + <= 1024 new labels, load <= 1/2
constexpr int64_t GROUPS_SCRATCH_DEFAULT = (int64_t)256 << 20;   // bytes of the scan engine's table where the caller names none
constexpr int GROUPS_SCAN_NQ = 4;                                // queries staged per workgroup of the scan (the flat scan's figure)
constexpr int64_t GROUPS_SCAN_MAX_CHUNK = 32768;                 // queries of one scan launch at most (the read-back's grid has one row of workgroups per query)
constexpr int64_t GROUPS_LISTS_BYTES = (int64_t)512 << 20;       // bytes of the read-back's partial lists of one chunk at most
constexpr int GROUPS_AUTO_ROUNDS = 1;                           // page rounds of EPS_GROUPS_AUTO before the scan takes the unfinished queries
constexpr int GROUPS_BLOCK_WAVES = 4;                            // wavefronts of a scan / read-back workgroup
constexpr int64_t GROUPS_TOPK_SLICE_MIN = 256;                   // table slots per wavefront before the read-back is split further
constexpr int64_t GROUPS_TOPK_MAX_WAVES = 1024;                  // wavefronts per query of the read-back
constexpr int64_t GROUPS_MERGE_KEYS = (int64_t)1 << 18;          // partial keys per query launch_among_merge's one workgroup is given at most (AMONG_MERGE_KEYS)

// The caller's keys -> dense labels: label[i] = rank of keys[i] among the distinct keys (ascending as int64), key_of_label[label[i]] = keys[i].
// Returns G, the number of distinct keys (<= n); *largest = rows of the largest group.  n < 2^31.
inline int64_t groups_relabel(const int64_t* keys, int64_t n, int32_t* label, std::vector<int64_t>* key_of_label, int64_t* largest) {
  key_of_label->assign(keys, keys + n);
  std::sort(key_of_label->begin(), key_of_label->end());
  key_of_label->erase(std::unique(key_of_label->begin(), key_of_label->end()), key_of_label->end());
  const int64_t G = (int64_t)key_of_label->size();
  std::vector<int64_t> rows((size_t)G, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t l = std::lower_bound(key_of_label->begin(), key_of_label->end(), keys[i]) - key_of_label->begin();
    label[i] = (int32_t)l;
    rows[(size_t)l] += 1;
  }
  int64_t most = 0;
  for (int64_t g = 0; g < G; ++g) most = rows[(size_t)g] > most ? rows[(size_t)g] : most;
  *largest = most;
  return G;
}

// EPS_OK, or EPS_USER_ERROR with the reason in *why
inline int32_t groups_args_check(int64_t nq, int32_t k, int32_t engine, int32_t page_rows, int64_t scratch_bytes, const char** why) {
  *why = "";
  if (nq < 0) return *why = "nq must be >= 0", EPS_USER_ERROR;
  if (k < 1 || k > GROUPS_MAX_K) return *why = "k must be in [1, 1024]", EPS_USER_ERROR;
  if (engine < EPS_GROUPS_AUTO || engine > EPS_GROUPS_SCAN) return *why = "unknown engine", EPS_USER_ERROR;
  if (page_rows < 0 || page_rows > GROUPS_MAX_PAGE) return *why = "page_rows must be 0 or in [1, 1024]", EPS_USER_ERROR;
  if (scratch_bytes < 0) return *why = "scratch_bytes must be >= 0", EPS_USER_ERROR;
  return EPS_OK;
}

// The rule's page: 4 k keys, rounded up to a multiple of 64, at most 1024 - a table whose groups hold 4 rows near a query on average finishes
// in one page.  page_rows > 0: the caller's.
inline int32_t groups_page_rows(int32_t k, int32_t page_rows) {
  if (page_rows > 0) return page_rows;
  const int64_t p = ((int64_t)4 * k + 63) / 64 * 64;
  return (int32_t)(p < GROUPS_MAX_PAGE ? p : GROUPS_MAX_PAGE);
}

struct GroupsScanPlan {
  int64_t c;        // queries that share the table at a time: a multiple of 4, >= 4
  int64_t chunks;   // ceil(m / c)
  int W;            // read-back wavefronts = partial lists per query, a multiple of GROUPS_BLOCK_WAVES
  int64_t slice;    // table slots per read-back wavefront: W * slice >= G
};
// m queries for the scan (> 0), G labels (> 0), scratch_bytes as the call was given it (0: the default)
inline GroupsScanPlan groups_scan_plan(int64_t m, int64_t G, int32_t k, int64_t scratch_bytes) {
  GroupsScanPlan p;
  int64_t gx = (G + GROUPS_TOPK_SLICE_MIN * GROUPS_BLOCK_WAVES - 1) / (GROUPS_TOPK_SLICE_MIN * GROUPS_BLOCK_WAVES);
  const int64_t cap_merge = GROUPS_MERGE_KEYS / ((int64_t)k * GROUPS_BLOCK_WAVES);
  const int64_t cap_waves = GROUPS_TOPK_MAX_WAVES / GROUPS_BLOCK_WAVES;
  gx = gx < cap_merge ? gx : cap_merge;
  gx = gx < cap_waves ? gx : cap_waves;
  gx = gx < 1 ? 1 : gx;
  p.W = (int)(gx * GROUPS_BLOCK_WAVES);
  p.slice = (G + p.W - 1) / p.W;
  const int64_t cap = scratch_bytes > 0 ? scratch_bytes : GROUPS_SCRATCH_DEFAULT;
  int64_t c = cap / (G * 8);   // (G < 2^31: no overflow)
  const int64_t lists = GROUPS_LISTS_BYTES / ((int64_t)p.W * k * 8);   // the read-back's partial lists, W * k keys per query, stay bounded too
  c = c < lists ? c : lists;
  c = c < m ? c : m;
  c = c < GROUPS_SCAN_MAX_CHUNK ? c : GROUPS_SCAN_MAX_CHUNK;
  c = c / GROUPS_SCAN_NQ * GROUPS_SCAN_NQ;
  p.c = c < GROUPS_SCAN_NQ ? GROUPS_SCAN_NQ : c;
  p.chunks = (m + p.c - 1) / p.c;
  return p;
}
// bytes of the table the plan asks for
inline int64_t groups_table_bytes(const GroupsScanPlan& p, int64_t G) { return p.c * G * 8; }

}  // namespace eps
