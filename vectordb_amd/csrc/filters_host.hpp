// Host side of the search under per-query filters (eps_index_search_filters; kernels: filters.hip): the limits, the validation of the programs, and
// the plan - which programs share a verdict plane, how the planes are cut into verdict passes, the queries sorted by plane, and, once the visible
// counts are known, the engine of every plane, where its list lies, and the gather's query blocks and work items.  Plain C++ with no HIP type in
// it: tests/native/filters_host_check.cpp runs it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/epsilla_gfx950.h"

namespace eps {

constexpr int32_t FILTERS_MAX_PROGS = 64;                      // programs of one call
constexpr int32_t FILTERS_MAX_OPS = 64, FILTERS_MAX_STACK = 16;   // eps_index_set_filter_program's limits
constexpr int32_t FILTERS_MAX_K = 1024;                        // the widest WaveTopK (KPL = 16)
constexpr int FILTERS_BLOCK_Q = 4;                             // queries of one plane a gather workgroup serves at most
constexpr int FILTERS_BLOCK_WAVES = 4;                         // wavefronts of a gather workgroup: one chunk of the list each
constexpr int64_t FILTERS_CHUNK = 512;                         // list entries per wavefront, at least
constexpr int64_t FILTERS_MAX_WAVES = 1024;                    // wavefronts over one list, at most (longer lists: longer chunks)
constexpr int64_t FILTERS_MERGE_KEYS = (int64_t)1 << 18;       // partial keys per query the merge's one workgroup is given at most
constexpr int32_t FILTERS_LDS_OPS = 2048;                      // instructions of one verdict pass: 48 KB of LDS
constexpr int64_t FILTERS_SCRATCH_BYTES = (int64_t)256 << 20;  // AUTO: lists and partial lists of the list engine together

// One compiled program as eps_index_set_filter_program and eps_index_search_filters both accept it: known opcodes, attribute loads inside a row
// of `stride` bytes, stack discipline, exactly one value left.  EPS_OK (*uses_dist: it pushes @distance), or EPS_USER_ERROR with the reason
inline int32_t filter_program_check(const eps_filter_op* ops, int32_t nops, int64_t stride, bool* uses_dist, const char** why) {
  static const int width[] = {0, 0, 0, 1, 2, 4, 8, 4, 8, 1};
  int sp = 0, maxsp = 0;
  *uses_dist = false;
  for (int32_t i = 0; i < nops; ++i) {
    const int op = ops[i].op;
    if (op < EPS_FOP_PUSH_CONST || op > EPS_FOP_NE_BOOL) return *why = "unknown opcode", EPS_USER_ERROR;
    if (op <= EPS_FOP_PUSH_BOOL) {
      if (op >= EPS_FOP_PUSH_I8 && (ops[i].arg < 0 || (int64_t)ops[i].arg + width[op] > stride))   // (in 64 bits: arg = INT32_MAX must not wrap)
        return *why = "attribute offset outside the row", EPS_USER_ERROR;
      *uses_dist |= op == EPS_FOP_PUSH_DIST;
      ++sp;
    } else if (op == EPS_FOP_NOT) {
      if (sp < 1) return *why = "stack underflow", EPS_USER_ERROR;
    } else {
      if (sp < 2) return *why = "stack underflow", EPS_USER_ERROR;
      --sp;
    }
    maxsp = sp > maxsp ? sp : maxsp;
  }
  if (sp != 1 || maxsp > FILTERS_MAX_STACK) return *why = "the program must leave exactly one value (stack depth <= 16)", EPS_USER_ERROR;
  return EPS_OK;
}

// EPS_OK, or the status with the reason in *why.  stride: bytes of an attribute row (<= 0: no rows were given - only empty programs pass)
inline int32_t filters_programs_check(const eps_filter_op* ops, const int32_t* prog_offsets, int32_t n_progs, int64_t stride, const char** why) {
  *why = "";
  if (n_progs < 1 || n_progs > FILTERS_MAX_PROGS) return *why = "n_progs must be in [1, 64]", EPS_USER_ERROR;
  if (!prog_offsets) return *why = "null buffer", EPS_USER_ERROR;
  if (prog_offsets[0] != 0) return *why = "prog_offsets[0] must be 0", EPS_USER_ERROR;
  for (int32_t j = 0; j < n_progs; ++j) {
    if (prog_offsets[j + 1] < prog_offsets[j]) return *why = "prog_offsets must be non-decreasing", EPS_USER_ERROR;
    if (prog_offsets[j + 1] - prog_offsets[j] > FILTERS_MAX_OPS) return *why = "a program of more than 64 instructions", EPS_DB_UNSUPPORTED_ERROR;
  }
  if (prog_offsets[n_progs] > 0 && !ops) return *why = "null buffer", EPS_USER_ERROR;
  if (prog_offsets[n_progs] > 0 && stride <= 0) return *why = "attribute rows missing", EPS_USER_ERROR;
  for (int32_t j = 0; j < n_progs; ++j) {
    if (prog_offsets[j + 1] == prog_offsets[j]) continue;   // the empty program: every row
    bool uses_dist;
    if (filter_program_check(ops + prog_offsets[j], prog_offsets[j + 1] - prog_offsets[j], stride, &uses_dist, why) != EPS_OK) return EPS_USER_ERROR;
    if (uses_dist) return *why = "a program reads @distance: a verdict plane is computed before any distance exists", EPS_USER_ERROR;
  }
  return EPS_OK;
}

struct FiltersBlock {     // up to block_q queries of one plane: what a gather workgroup stages
  int64_t list_begin;     // the plane's list inside the lists' buffer
  int32_t list_len;
  int32_t chunk;          // list entries per wavefront
  int32_t q0, nq;         // sorted positions [q0, q0 + nq) of its queries
  int32_t wave0, waves;   // its partial lists: [wave0, wave0 + waves) x block_q x k keys; waves a multiple of FILTERS_BLOCK_WAVES
};
struct FiltersItem {      // one gather workgroup: wavefront w takes chunk group * FILTERS_BLOCK_WAVES + w of the block's list
  int32_t block, group;
};

struct FiltersPlan {
  // ---- before the counts are known
  int32_t planes = 0;                  // distinct programs
  std::vector<int32_t> plane_of_prog;  // [n_progs]
  std::vector<int32_t> prog_of_plane;  // [planes] the first program with that text
  std::vector<int32_t> op_off;         // [planes + 1] the planes' instructions, one after the other
  std::vector<int32_t> pass_begin;     // verdict pass i judges planes [pass_begin[i], pass_begin[i + 1]): at most FILTERS_LDS_OPS instructions
  std::vector<int32_t> order;          // [nq] sorted position -> the caller's query; by plane, the caller's order inside a plane
  std::vector<int32_t> inverse;        // [nq] the caller's query -> sorted position
  std::vector<int32_t> plane_q0;       // [planes + 1] sorted positions of a plane's queries
  // ---- after them
  std::vector<int32_t> engine;         // [planes] 0: no query, EPS_FILTERS_LISTS, EPS_FILTERS_PLANES
  std::vector<int64_t> list_begin;     // [planes] where a list-engine plane's list starts
  int64_t list_total = 0;              // entries of all lists
  int block_q = 1;
  std::vector<FiltersBlock> blocks;
  std::vector<FiltersItem> items;
  std::vector<int32_t> block_of;       // [nq] by sorted position: the query's block, -1 on the plane engine
  int64_t partial_waves = 0;           // partial lists of block_q x k keys
  int64_t list_queries = 0, list_evals = 0;   // queries on the list engine; (row, query) pairs it gives a distance
};

// EPS_OK, or EPS_USER_ERROR with the reason.  Programs with identical instructions share a plane; the queries sorted by plane
inline int32_t filters_plan_queries(const eps_filter_op* ops, const int32_t* prog_offsets, int32_t n_progs, const int32_t* query_prog, int64_t nq,
                                    FiltersPlan* p, const char** why) {
  *why = "";
  p->plane_of_prog.assign((size_t)n_progs, 0);
  p->prog_of_plane.clear();
  for (int32_t j = 0; j < n_progs; ++j) {
    const int32_t len = prog_offsets[j + 1] - prog_offsets[j];
    int32_t found = -1;
    for (size_t d = 0; d < p->prog_of_plane.size() && found < 0; ++d) {
      const int32_t o = p->prog_of_plane[d];
      if (prog_offsets[o + 1] - prog_offsets[o] == len && (len == 0 || memcmp(ops + prog_offsets[o], ops + prog_offsets[j], (size_t)len * sizeof(eps_filter_op)) == 0))
        found = (int32_t)d;
    }
    if (found < 0) {
      found = (int32_t)p->prog_of_plane.size();
      p->prog_of_plane.push_back(j);
    }
    p->plane_of_prog[(size_t)j] = found;
  }
  p->planes = (int32_t)p->prog_of_plane.size();
  p->op_off.assign((size_t)p->planes + 1, 0);
  p->pass_begin.assign(1, 0);
  int32_t in_pass = 0;
  for (int32_t d = 0; d < p->planes; ++d) {
    const int32_t o = p->prog_of_plane[(size_t)d], len = prog_offsets[o + 1] - prog_offsets[o];
    p->op_off[(size_t)d + 1] = p->op_off[(size_t)d] + len;
    if (in_pass + len > FILTERS_LDS_OPS) {   // (len <= 64: a pass is never empty)
      p->pass_begin.push_back(d);
      in_pass = 0;
    }
    in_pass += len;
  }
  p->pass_begin.push_back(p->planes);
  // the queries by plane: a counting sort, stable
  p->plane_q0.assign((size_t)p->planes + 1, 0);
  for (int64_t q = 0; q < nq; ++q) {
    if (query_prog[q] < 0 || query_prog[q] >= n_progs) return *why = "a query_prog entry outside [0, n_progs)", EPS_USER_ERROR;
    p->plane_q0[(size_t)p->plane_of_prog[(size_t)query_prog[q]] + 1] += 1;
  }
  for (int32_t d = 0; d < p->planes; ++d) p->plane_q0[(size_t)d + 1] += p->plane_q0[(size_t)d];
  std::vector<int32_t> cursor(p->plane_q0.begin(), p->plane_q0.end() - 1);
  p->order.assign((size_t)nq, 0);
  p->inverse.assign((size_t)nq, 0);
  for (int64_t q = 0; q < nq; ++q) {
    const int32_t s = cursor[(size_t)p->plane_of_prog[(size_t)query_prog[q]]]++;
    p->order[(size_t)s] = (int32_t)q;
    p->inverse[(size_t)q] = s;
  }
  return EPS_OK;
}

// list entries per wavefront and wavefronts (a multiple of FILTERS_BLOCK_WAVES; 0 for an empty list) over a list of `len` entries
inline void filters_chunking(int64_t len, int32_t k, int32_t* chunk, int32_t* waves) {
  int64_t most = FILTERS_MERGE_KEYS / k;
  most = most < FILTERS_MAX_WAVES ? most : FILTERS_MAX_WAVES;
  most = most / FILTERS_BLOCK_WAVES * FILTERS_BLOCK_WAVES;   // (>= 256)
  int64_t c = (len + most - 1) / most;
  c = c < FILTERS_CHUNK ? FILTERS_CHUNK : c;
  const int64_t w = (len + c - 1) / c;
  *chunk = (int32_t)c;
  *waves = (int32_t)((w + FILTERS_BLOCK_WAVES - 1) / FILTERS_BLOCK_WAVES * FILTERS_BLOCK_WAVES);
}

// bytes of a plane's list and of the partial lists of its m queries
inline int64_t filters_list_bytes(int64_t count, int64_t m, int32_t k, int block_q) {
  int32_t chunk, waves;
  filters_chunking(count, k, &chunk, &waves);
  const int64_t blocks = (m + block_q - 1) / block_q;
  return count * 4 + blocks * waves * block_q * (int64_t)k * 8;
}

// AUTO's crossover, from the forced engines' times at 1M x 768, k = 10: the gather costs ~0.48 ns per (list entry, query block), the
// matrix engine under a plane costs the more the fewer rows the plane shows (~1 / s), so the break-even selectivity falls as 1 / sqrt(blocks):
// 40 % for one block of 4 queries, 10 % for 16 blocks, 2.5 % for 256.  A plane is dense when s x sqrt(blocks) > 0.4
inline bool filters_dense(int64_t count, int64_t n, int64_t blocks) {
  return 25.0 * (double)count * (double)count * (double)blocks > 4.0 * (double)n * (double)n;
}

// counts[planes]: visible rows of every plane.  engine: EPS_FILTERS_AUTO / _LISTS / _PLANES.  matrix[planes] (AUTO only; null: none): the flat
// engine a plane's queries would take is the matrix engine.  AUTO: the plane engine for a dense plane (filters_dense) the matrix engine would
// serve, and for the planes whose lists no longer fit scratch_bytes; the list engine otherwise
inline void filters_plan_engines(FiltersPlan* p, const int64_t* counts, int64_t n, int32_t k, int block_q, int32_t engine, const bool* matrix,
                                 int64_t scratch_bytes) {
  p->block_q = block_q;
  p->engine.assign((size_t)p->planes, 0);
  p->list_begin.assign((size_t)p->planes, 0);
  p->blocks.clear();
  p->items.clear();
  p->block_of.assign(p->order.size(), -1);
  p->list_total = p->partial_waves = p->list_queries = p->list_evals = 0;
  int64_t used = 0;
  for (int32_t d = 0; d < p->planes; ++d) {
    const int64_t m = p->plane_q0[(size_t)d + 1] - p->plane_q0[(size_t)d], count = counts[d];
    if (m == 0) continue;
    int32_t e = engine;
    if (e == EPS_FILTERS_AUTO) {
      const int64_t bytes = filters_list_bytes(count, m, k, block_q);
      const bool dense = matrix && matrix[d] && filters_dense(count, n, (m + block_q - 1) / block_q);
      e = (!dense && used + bytes <= scratch_bytes) ? EPS_FILTERS_LISTS : EPS_FILTERS_PLANES;
      if (e == EPS_FILTERS_LISTS) used += bytes;
    }
    p->engine[(size_t)d] = e;
    if (e != EPS_FILTERS_LISTS) continue;
    p->list_begin[(size_t)d] = p->list_total;
    int32_t chunk, waves;
    filters_chunking(count, k, &chunk, &waves);
    for (int64_t b0 = 0; b0 < m; b0 += block_q) {
      FiltersBlock b;
      b.list_begin = p->list_total;
      b.list_len = (int32_t)count;
      b.chunk = chunk;
      b.q0 = (int32_t)(p->plane_q0[(size_t)d] + b0);
      b.nq = (int32_t)(m - b0 < block_q ? m - b0 : block_q);
      b.wave0 = (int32_t)p->partial_waves;
      b.waves = waves;
      for (int32_t g = 0; g < waves / FILTERS_BLOCK_WAVES; ++g) p->items.push_back(FiltersItem{(int32_t)p->blocks.size(), g});
      for (int32_t q = 0; q < b.nq; ++q) p->block_of[(size_t)(b.q0 + q)] = (int32_t)p->blocks.size();
      p->blocks.push_back(b);
      p->partial_waves += waves;
    }
    p->list_total += count;
    p->list_queries += m;
    p->list_evals += m * count;
  }
}

}  // namespace eps
