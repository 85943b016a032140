// Host side of the search among given rows (eps_index_search_among; kernels: among.hip): the limits, the validation of the per-query offsets and the
// launch plan - how many wavefronts share a query's list and which entries each of them takes.  Plain C++ with no HIP type in it: the kernel reads
// its chunk through among_chunk below, the same function tests/native/among_host_check.cpp runs under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"

#if defined(__HIPCC__)
#define EPS_AMONG_HD __host__ __device__
#else
#define EPS_AMONG_HD
#endif

namespace eps {

constexpr int32_t AMONG_MAX_K = 1024;                          // the widest WaveTopK (KPL = 16)
constexpr int64_t AMONG_MAX_CAND = ((int64_t)1 << 31) - 1;     // entries of all lists together
constexpr int AMONG_BLOCK_WAVES = 4;                           // wavefronts of a gather workgroup
constexpr int64_t AMONG_WAVE_MIN = 32;                         // list entries per wavefront before a list is split further (flat_scan_waves' figure)
constexpr int64_t AMONG_MAX_BLOCKS = 2048;                     // gather workgroups of one launch, all queries together (flat_scan_waves' figure)
constexpr int64_t AMONG_MERGE_KEYS = (int64_t)1 << 18;         // partial keys per query the merge's one workgroup is given at most (k = 1024: 256 wavefronts)
constexpr int64_t AMONG_GRID_Y = 32768;                        // query tiles of one launch; longer batches run in slices

// EPS_OK, or EPS_USER_ERROR with the reason in *why.  offsets == null: one list of n_cand entries for every query.  *longest: the longest list.
inline int32_t among_lists_check(const int64_t* offsets, int64_t nq, int64_t n_cand, int64_t* longest, const char** why) {
  *why = "";
  *longest = 0;
  if (nq < 0) return *why = "nq must be >= 0", EPS_USER_ERROR;
  if (n_cand < 0 || n_cand > AMONG_MAX_CAND) return *why = "n_cand must be in [0, 2^31)", EPS_USER_ERROR;
  if (!offsets) {
    *longest = n_cand;
    return EPS_OK;
  }
  if (nq == 0) return EPS_OK;   // (nothing is read)
  if (offsets[0] != 0) return *why = "cand_offsets[0] must be 0", EPS_USER_ERROR;
  int64_t most = 0;
  for (int64_t j = 0; j < nq; ++j) {
    if (offsets[j + 1] < offsets[j]) return *why = "cand_offsets must be non-decreasing", EPS_USER_ERROR;
    if (offsets[j + 1] > n_cand) return *why = "cand_offsets[nq] must be n_cand", EPS_USER_ERROR;   // (non-decreasing: the last entry is beyond it too)
    const int64_t len = offsets[j + 1] - offsets[j];
    most = len > most ? len : most;
  }
  if (offsets[nq] != n_cand) return *why = "cand_offsets[nq] must be n_cand", EPS_USER_ERROR;
  *longest = most;
  return EPS_OK;
}

// Wavefront w of a query takes entries [*begin, *end) of the query's list of `len` entries: consecutive chunks of `chunk`, the ones beyond the
// list's end empty (begin = end = len).
EPS_AMONG_HD inline void among_chunk(int64_t len, int64_t chunk, int64_t w, int64_t* begin, int64_t* end) {
  // (w * chunk < 2^13 * 2^31: no overflow)
  const int64_t b = w * chunk < len ? w * chunk : len;
  *begin = b;
  *end = len - b < chunk ? len : b + chunk;
}

struct AmongPlan {
  int nq_tile;      // queries of one workgroup: pick_nq's for the shared list, 1 for per-query lists
  int64_t tiles;    // workgroups in y over the whole batch (launched in slices of AMONG_GRID_Y)
  int W;            // wavefronts = partial lists per query, a multiple of AMONG_BLOCK_WAVES
  int64_t chunk;    // list entries per wavefront: W * chunk >= the longest list
};
// nq_tile: what the launcher stages per workgroup for this (nq, k, dim) when the list is shared; `longest` >= 0 as among_lists_check leaves it
inline AmongPlan among_plan(bool shared, int64_t nq, int64_t longest, int32_t k, int nq_tile) {
  AmongPlan p;
  p.nq_tile = shared ? nq_tile : 1;
  p.tiles = (nq + p.nq_tile - 1) / p.nq_tile;
  int64_t gx = (longest + AMONG_WAVE_MIN * AMONG_BLOCK_WAVES - 1) / (AMONG_WAVE_MIN * AMONG_BLOCK_WAVES);   // >= 32 entries per wavefront
  int64_t cap = AMONG_MAX_BLOCKS / (p.tiles > 0 ? p.tiles : 1);   // many queries fill the chip by themselves
  const int64_t cap_merge = AMONG_MERGE_KEYS / ((int64_t)k * AMONG_BLOCK_WAVES);
  cap = cap < cap_merge ? cap : cap_merge;
  gx = gx < cap ? gx : cap;
  gx = gx < 1 ? 1 : gx;
  p.W = (int)(gx * AMONG_BLOCK_WAVES);
  p.chunk = (longest + p.W - 1) / p.W;
  if (p.chunk < 1) p.chunk = 1;
  return p;
}

}  // namespace eps
