// Host side of the list merges (eps_merge_range, eps_merge_range_packed, eps_merge_select; kernel: merge_lists.hip): the arguments of the launch,
// the layout of one shard's packed radius answer, the argument checks and the staging of host buffers.  Plain C++ with no HIP type in it: the device
// is whatever `Dev` the caller hands in (c_abi.cpp: the HIP runtime; tests/native/merge_host_check.cpp: the host's own memory under a sanitizer).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"

namespace eps {

constexpr int32_t MERGE_MAX_SHARDS = 16;
constexpr int32_t MERGE_MAX_CAP = 8192;   // = RANGE_MAX_CAP: what one eps_index_search_range returns per query

// `shards` sorted lists per query, list s of query j = elements [j * L, j * L + len) of shard s's arrays, len = its counts entry clamped to [0, L];
// ranks [skip, skip + cap) of their merged order go to out_ids (and out_dist) [nq][cap].  Radius form: keys (ordinal of dist, id), counts int32,
// out_counts int32; select form: keys = ids, dist = null, counts int64, out_counts int64.  Shard s's arrays start `*_stride` BYTES after shard s - 1's.
struct MergeRankArgs {
  const char* ids;      // int64
  const char* dist;     // float, or null
  const char* counts;   // int32 [nq] (radius) | int64 [nq] (select)
  const char* totals;   // int64 [nq]
  int64_t ids_stride, dist_stride, counts_stride, totals_stride;
  int32_t shards;
  int64_t nq, L, skip, cap;
  int64_t* out_ids;
  float* out_dist;      // or null
  void* out_counts;     // [nq] clamp(sum of len - skip, 0, cap), or null
  int64_t* out_totals;  // [nq] sum of totals, or null
};

// one shard's packed radius answer: ids i64[nq][cap] | totals i64[nq] | dist f32[nq][cap] | counts i32[nq], rounded up to 8 bytes
struct RangePack {
  int64_t totals_off, dist_off, counts_off, bytes;
};
inline RangePack range_pack(int64_t nq, int64_t cap) {
  RangePack p;
  p.totals_off = nq * cap * 8;
  p.dist_off = p.totals_off + nq * 8;
  p.counts_off = p.dist_off + nq * cap * 4;
  p.bytes = (p.counts_off + nq * 4 + 7) / 8 * 8;
  return p;
}
inline bool merge_sizes_ok(int32_t shards, int64_t nq, int64_t cap) {   // every byte count below stays far inside an int64
  return shards >= 1 && shards <= MERGE_MAX_SHARDS && nq >= 0 && cap >= 0 && (cap == 0 || nq <= (INT64_MAX >> 8) / cap);
}

inline MergeRankArgs merge_range_args(const void* ids, int64_t ids_stride, const void* dist, int64_t dist_stride, const void* counts, int64_t counts_stride,
                                      const void* totals, int64_t totals_stride, int32_t shards, int64_t nq, int32_t cap, int64_t* out_ids, float* out_dist,
                                      int32_t* out_counts, int64_t* out_totals) {
  MergeRankArgs a;
  a.ids = static_cast<const char*>(ids);
  a.dist = static_cast<const char*>(dist);
  a.counts = static_cast<const char*>(counts);
  a.totals = static_cast<const char*>(totals);
  a.ids_stride = ids_stride;
  a.dist_stride = dist_stride;
  a.counts_stride = counts_stride;
  a.totals_stride = totals_stride;
  a.shards = shards;
  a.nq = nq;
  a.L = cap;
  a.skip = 0;
  a.cap = cap;
  a.out_ids = out_ids;
  a.out_dist = out_dist;
  a.out_counts = out_counts;
  a.out_totals = out_totals;
  return a;
}
inline MergeRankArgs merge_range_args_packed(const void* gathered, int64_t stride, int32_t shards, int64_t nq, int32_t cap, int64_t* out_ids, float* out_dist,
                                             int32_t* out_counts, int64_t* out_totals) {
  const RangePack p = range_pack(nq, cap);
  const char* g = static_cast<const char*>(gathered);
  return merge_range_args(g, stride, g + p.dist_off, stride, g + p.counts_off, stride, g + p.totals_off, stride, shards, nq, cap, out_ids, out_dist, out_counts,
                          out_totals);
}
inline MergeRankArgs merge_select_args(const int64_t* ids, const int64_t* counts, const int64_t* totals, int32_t shards, int64_t len, int64_t skip, int64_t limit,
                                       int64_t* out_ids, int64_t* count_out, int64_t* total_out) {
  MergeRankArgs a = merge_range_args(ids, len * 8, nullptr, 0, counts, 8, totals, 8, shards, 1, 0, out_ids, nullptr, nullptr, total_out);
  a.L = len;
  a.skip = skip;
  a.cap = limit;
  a.out_counts = count_out;
  return a;
}

// EPS_OK, or the status of the refusal with its reason in *why.  The radius form looks at its pointers after these (nq = 0 needs none).
inline int32_t merge_range_check(int32_t shards, int64_t nq, int32_t cap, const char** why) {
  *why = "";
  if (shards < 1 || shards > MERGE_MAX_SHARDS) return *why = "shards must be in 1 .. 16", EPS_USER_ERROR;
  if (cap < 1 || cap > MERGE_MAX_CAP) return *why = "cap must be in 1 .. 8192", EPS_USER_ERROR;
  if (nq < 0 || !merge_sizes_ok(shards, nq, cap)) return *why = "nq is negative or too large", EPS_USER_ERROR;
  return EPS_OK;
}
inline int32_t merge_select_check(bool pointers, int32_t shards, int64_t len, int64_t skip, int64_t limit, const char** why) {
  *why = "";
  if (!pointers) return *why = "null pointer", EPS_USER_ERROR;
  if (shards < 1 || shards > MERGE_MAX_SHARDS) return *why = "shards must be in 1 .. 16", EPS_USER_ERROR;
  if (len < 0 || skip < 0 || limit < 0) return *why = "negative len, skip or limit", EPS_USER_ERROR;
  if (!merge_sizes_ok(shards, 1, len) || skip > len || limit > len - skip) return *why = "len < skip + limit: a shard's list must reach as far as the window", EPS_USER_ERROR;
  return EPS_OK;
}

// 1: every pointer that is not null is a device pointer; 0: none is; -1: a mixed set
template <class Dev>
inline int merge_side(Dev& dev, const void* const* ptrs, int n) {
  int side = -1;
  for (int i = 0; i < n; ++i) {
    if (!ptrs[i]) continue;
    const int d = dev.is_device(ptrs[i]) ? 1 : 0;
    if (side >= 0 && d != side) return -1;
    side = d;
  }
  return side;
}

// Host buffers: the shards' answers are staged in the packed layout (one device block of shards + 1 packs: the last receives the merged answer),
// the packed launch runs, the parts come back.  Synchronises.
template <class Dev>
inline int32_t merge_range_host(Dev& dev, const int64_t* ids, const float* dist, const int32_t* counts, const int64_t* totals, int32_t shards, int64_t nq,
                                int32_t cap, int64_t* out_ids, float* out_dist, int32_t* out_counts, int64_t* out_totals) {
  const RangePack p = range_pack(nq, cap);
  const size_t nk = (size_t)nq * (size_t)cap;
  char* d = static_cast<char*>(dev.alloc((size_t)p.bytes * ((size_t)shards + 1)));
  if (!d) return EPS_INFRA_UNEXPECTED_ERROR;
  bool ok = true;
  for (int32_t s = 0; s < shards && ok; ++s) {
    char* slot = d + (size_t)p.bytes * s;
    ok = dev.h2d(slot, ids + nk * s, nk * 8) && dev.h2d(slot + p.totals_off, totals + (size_t)nq * s, (size_t)nq * 8) &&
         dev.h2d(slot + p.dist_off, dist + nk * s, nk * 4) && dev.h2d(slot + p.counts_off, counts + (size_t)nq * s, (size_t)nq * 4);
  }
  char* out = d + (size_t)p.bytes * shards;
  if (ok) {
    dev.launch(merge_range_args_packed(d, p.bytes, shards, nq, cap, reinterpret_cast<int64_t*>(out), reinterpret_cast<float*>(out + p.dist_off),
                                       reinterpret_cast<int32_t*>(out + p.counts_off), reinterpret_cast<int64_t*>(out + p.totals_off)));
    ok = dev.d2h(out_ids, out, nk * 8) && dev.d2h(out_dist, out + p.dist_off, nk * 4) && (!out_counts || dev.d2h(out_counts, out + p.counts_off, (size_t)nq * 4)) &&
         (!out_totals || dev.d2h(out_totals, out + p.totals_off, (size_t)nq * 8));
  }
  ok = dev.sync() && ok;
  dev.free(d);
  return ok ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

// device block: ids [shards][len] | counts [shards] | totals [shards] | out ids [limit] | count, total
template <class Dev>
inline int32_t merge_select_host(Dev& dev, const int64_t* ids, const int64_t* counts, const int64_t* totals, int32_t shards, int64_t len, int64_t skip,
                                 int64_t limit, int64_t* out_ids, int64_t* count_out, int64_t* total_out) {
  const size_t in_n = (size_t)shards * (size_t)len;
  int64_t* d = static_cast<int64_t*>(dev.alloc((in_n + 2 * (size_t)shards + (size_t)limit + 2) * 8));
  if (!d) return EPS_INFRA_UNEXPECTED_ERROR;
  int64_t* d_counts = d + in_n;
  int64_t* d_totals = d_counts + shards;
  int64_t* d_out = d_totals + shards;
  int64_t* d_scal = d_out + limit;
  bool ok = (in_n == 0 || dev.h2d(d, ids, in_n * 8)) && dev.h2d(d_counts, counts, (size_t)shards * 8) && dev.h2d(d_totals, totals, (size_t)shards * 8);
  if (ok) {
    dev.launch(merge_select_args(d, d_counts, d_totals, shards, len, skip, limit, d_out, d_scal, d_scal + 1));
    ok = (limit == 0 || dev.d2h(out_ids, d_out, (size_t)limit * 8)) && dev.d2h(count_out, d_scal, 8) && (!total_out || dev.d2h(total_out, d_scal + 1, 8));
  }
  ok = dev.sync() && ok;
  dev.free(d);
  return ok ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

}  // namespace eps
