// Host side of the diverse search (eps_index_search_diverse; kernel: diverse.hip): the checks of the call's arguments and the LDS layout of
// diverse_select_kernel - one function, diverse_lds, that the launcher sizes the launch with and the kernel takes its pointers from.  Plain C++
// with no HIP type in it: tests/native/diverse_host_check.cpp runs it under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/epsilla_gfx950.h"

#if defined(__HIPCC__)
#define EPS_DIVERSE_HD __host__ __device__
#else
#define EPS_DIVERSE_HD
#endif

namespace eps {

constexpr int32_t DIVERSE_MAX_FETCH = 1024;       // pool rows per query: a page of the flat engines, the widest list of search_among
constexpr int DIVERSE_THREADS = 256;              // one workgroup per query
constexpr int DIVERSE_WAVES = DIVERSE_THREADS / 64;
constexpr int64_t DIVERSE_LDS_BUDGET = 65536;     // what a launch gets without an attribute
constexpr int64_t DIVERSE_GRID = 32768;           // queries of one launch; longer batches run in slices

// EPS_OK, or EPS_USER_ERROR with the reason in *why
inline int32_t diverse_args_check(int64_t nq, int32_t k, int32_t fetch_k, float lambda, const char** why) {
  *why = "";
  if (nq < 0) return *why = "nq must be >= 0", EPS_USER_ERROR;
  if (k < 1 || fetch_k > DIVERSE_MAX_FETCH || k > fetch_k) return *why = "1 <= k <= fetch_k <= 1024 must hold", EPS_USER_ERROR;
  if (!(lambda >= 0.0f && lambda <= 1.0f)) return *why = "lambda must be in [0, 1]", EPS_USER_ERROR;   // (a NaN fails both tests)
  return EPS_OK;
}

// Byte offsets of the kernel's dynamic LDS: the selected row first (16-byte pieces are read from it), the 8-byte keys, the 8-byte reduction
// words, the 4-byte m, the marks.  Every region starts at a multiple of its element size; `bytes` is the launch's size.
struct DiverseLds {
  int row;      // float [(dim + 3) & ~3]: the row selected last, zeros behind its dim floats
  int keys;     // u64 [fetch_k]: the pool, ascending, KEY_EMPTY behind its np entries
  int red;      // u64 [DIVERSE_WAVES]: every wavefront's smallest (score ordinal, position) key
  int m;        // float [fetch_k]: the smallest distance to a selected row so far
  int taken;    // uint8 [fetch_k]: 1 = selected
  int bytes;
};
EPS_DIVERSE_HD inline DiverseLds diverse_lds(int fetch_k, int dim) {
  DiverseLds L;
  L.row = 0;
  L.keys = ((dim + 3) & ~3) * 4;           // (a multiple of 16)
  L.red = L.keys + fetch_k * 8;
  L.m = L.red + DIVERSE_WAVES * 8;
  L.taken = L.m + fetch_k * 4;
  L.bytes = (L.taken + fetch_k + 15) & ~15;
  return L;
}

}  // namespace eps
