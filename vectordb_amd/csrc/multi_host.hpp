// Host side of the multi-vector search (eps_index_search_multi; kernels: multi.hip): the checks of the call's arguments and of the bags' offsets, the
// refusal of a bag whose own table exceeds the caller's cap, and the plan - which whole bags share one table at a time, how the table's columns are
// cut among the wavefronts that read it back.  Plain C++ with no HIP type in it: tests/native/multi_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "among_host.hpp"
#include "groups_host.hpp"

namespace eps {

constexpr int32_t MULTI_MAX_K = 1024;                          // the widest WaveTopK (KPL = 16)
constexpr int64_t MULTI_MAX_BAG = 1024;                        // vectors of one bag
constexpr int64_t MULTI_MAX_VECTORS = ((int64_t)1 << 31) - 1;  // vectors of all bags together
constexpr int64_t MULTI_CHUNK = 256;                           // rows of a group one work item of the gather walks
constexpr int MULTI_QUAD = 4;                                  // vectors of a bag one work item serves (the flat scan's figure)
constexpr int64_t MULTI_MAX_PAIRS = (int64_t)1 << 20;          // (bag, candidate) pairs of one pass, unless one bag alone names more
constexpr int64_t MULTI_MAX_WAVES = 4096;                      // workgroups (of one wavefront) of the gather at most: they stride over the work list
constexpr int64_t MULTI_MAX_BAGS = 32768;                      // bags of one pass (the read-back's grid has one row of workgroups per bag)

// EPS_OK, or EPS_USER_ERROR with the reason in *why
inline int32_t multi_args_check(int64_t nq, int32_t k, int64_t n_cand, int64_t scratch_bytes, const char** why) {
  *why = "";
  if (nq < 0) return *why = "nq must be >= 0", EPS_USER_ERROR;
  if (k < 1 || k > MULTI_MAX_K) return *why = "k must be in [1, 1024]", EPS_USER_ERROR;
  if (n_cand < 0 || n_cand > AMONG_MAX_CAND) return *why = "n_cand must be in [0, 2^31)", EPS_USER_ERROR;
  if (scratch_bytes < 0) return *why = "scratch_bytes must be >= 0", EPS_USER_ERROR;
  return EPS_OK;
}

// The bags: q_offsets[nq + 1], [0] = 0, non-decreasing, no bag above 1024 vectors.  *total = q_offsets[nq], *largest = the largest bag
inline int32_t multi_bags_check(const int64_t* q_offsets, int64_t nq, int64_t* total, int64_t* largest, const char** why) {
  *why = "";
  *total = *largest = 0;
  if (nq == 0) return EPS_OK;   // (nothing is read)
  if (q_offsets[0] != 0) return *why = "q_offsets[0] must be 0", EPS_USER_ERROR;
  int64_t most = 0;
  for (int64_t j = 0; j < nq; ++j) {
    if (q_offsets[j + 1] < q_offsets[j]) return *why = "q_offsets must be non-decreasing", EPS_USER_ERROR;
    const int64_t t = q_offsets[j + 1] - q_offsets[j];
    if (t > MULTI_MAX_BAG) return *why = "a bag holds more than 1024 vectors", EPS_USER_ERROR;
    most = t > most ? t : most;
  }
  if (q_offsets[nq] > MULTI_MAX_VECTORS) return *why = "q_offsets[nq] must be < 2^31", EPS_USER_ERROR;
  *total = q_offsets[nq];
  *largest = most;
  return EPS_OK;
}

// The bytes the tables of a pass may take: the caller's cap, or (0) max(256 MiB, the largest bag's own table).  largest_bytes: the 8-byte keys of
// the one bag that needs most - t x G for the whole-table form, t x its candidates for the candidate form (t <= 2^10, either factor < 2^31: no
// overflow).  False: that bag does not fit the caller's cap - the call is refused before any launch
inline bool multi_scratch_cap(int64_t scratch_bytes, int64_t largest_bytes, int64_t* cap) {
  if (scratch_bytes > 0) {
    *cap = scratch_bytes;
    return largest_bytes <= scratch_bytes;
  }
  *cap = largest_bytes > GROUPS_SCRATCH_DEFAULT ? largest_bytes : GROUPS_SCRATCH_DEFAULT;
  return true;
}

// Whole bags of one pass: [j0, the value returned), at least one.  cum_a / cum_b: non-decreasing running totals over the bags ([nq + 1], cum_b
// may be null); the pass keeps cum[j1] - cum[j0] within cap_a and cap_b unless bag j0 alone exceeds them (a bag is never cut), and takes
// MULTI_MAX_BAGS bags at most
inline int64_t multi_slice_end(const int64_t* cum_a, int64_t cap_a, const int64_t* cum_b, int64_t cap_b, int64_t nq, int64_t j0, int64_t max_bags) {
  int64_t j1 = j0 + 1;
  while (j1 < nq && j1 - j0 < max_bags && cum_a[j1 + 1] - cum_a[j0] <= cap_a && (!cum_b || cum_b[j1 + 1] - cum_b[j0] <= cap_b)) ++j1;
  return j1;
}

struct MultiTopkPlan {
  int W;            // read-back wavefronts = partial lists per bag, a multiple of GROUPS_BLOCK_WAVES
  int64_t slice;    // columns (labels, or candidates of a bag) per wavefront: W * slice >= columns
  int64_t bags;     // bags of one pass at most: their partial lists stay within GROUPS_LISTS_BYTES
};
// columns: G, or the longest candidate list (>= 0); cut as groups_scan_plan cuts a table
inline MultiTopkPlan multi_topk_plan(int64_t columns, int32_t k) {
  const GroupsScanPlan g = groups_scan_plan(1, columns > 0 ? columns : 1, k, 0);
  MultiTopkPlan p;
  p.W = g.W;
  p.slice = g.slice;
  const int64_t lists = GROUPS_LISTS_BYTES / ((int64_t)p.W * k * 8);   // (W * k <= 2^18: >= 256)
  p.bags = lists < MULTI_MAX_BAGS ? lists : MULTI_MAX_BAGS;
  return p;
}

// vectors that share the whole-table form's table at a time: what the cap holds, and what one scan launch takes
inline int64_t multi_table_vectors(int64_t cap_bytes, int64_t G) {
  const int64_t fit = cap_bytes / ((G > 0 ? G : 1) * 8);
  return fit < GROUPS_SCAN_MAX_CHUNK ? fit : GROUPS_SCAN_MAX_CHUNK;
}

// work items of a (bag, candidate) pair: chunks of its group's rows x quads of the bag's vectors
EPS_AMONG_HD inline int64_t multi_pair_items(int64_t group_rows, int64_t t) {
  return ((group_rows + MULTI_CHUNK - 1) / MULTI_CHUNK) * ((t + MULTI_QUAD - 1) / MULTI_QUAD);
}

}  // namespace eps
