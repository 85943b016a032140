// Host side of the graph unit (graph_build.hip, traverse.hip) that needs no device: the seed list of a search, the connectivity repair and the
// CSR assembly of the build, the traversal's launch plan with its device-range refusals, the LDS layouts of prune_kernel, traverse_kernel and
// traverse2_kernel and the arithmetic of the tail merge.  Plain C++ with no device type in it: the kernels carve their LDS arrays from the layout
// structs below, the same functions tests/native/graph_host_check.cpp runs under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/epsilla_gfx950.h"

#if defined(__HIPCC__)
#define EPS_GRAPH_HD __host__ __device__
#else
#define EPS_GRAPH_HD
#endif

namespace eps {

// ------------------------------------------------------------------------------------------------ seed list
// PrepareInitIds (vec_search_executor.cpp:487-516; GetNeighbors' seeds, nsg.cpp:174-195, follow the same rule): the distinct neighbours of the
// navigation node in list order, then nav+1, nav+2, ... wrapping, until there are L.  adj[0..count) is the node's list as u32 or int64 ids; an
// entry that names no node (the 0xFFFFFFFF / -1 padding of a fixed-stride list) is skipped.  The reference requires n >= L (its fill loop never
// ends otherwise); callers clamp L to n.
template <class Id>
inline void seed_list(const Id* adj, int64_t count, int64_t nav, int64_t n, int64_t L, std::vector<uint32_t>& out) {
  std::vector<uint8_t> sel((size_t)n, 0);
  out.clear();
  out.reserve((size_t)L);
  for (int64_t e = 0; e < count && (int64_t)out.size() < L; ++e) {
    const int64_t v = (int64_t)adj[e];
    if (v < 0 || v >= n || sel[v]) continue;
    sel[v] = 1;
    out.push_back((uint32_t)v);
  }
  int64_t tmp = nav + 1;
  while ((int64_t)out.size() < L) {
    if (tmp >= n) tmp = 0;
    const int64_t v = tmp++;
    if (sel[v]) continue;
    sel[v] = 1;
    out.push_back((uint32_t)v);
  }
}

// ------------------------------------------------------------------------------------------------ connectivity and CSR of the build
// Fixed-stride lists as the build's kernels leave them: node v's edges are ids[v * R + 0 .. deg[v]).
// Depth-first from `from` (marked reached here): everything it reaches over the lists is marked.  `stack` is scratch, empty on entry and exit.
inline void mark_reached(uint32_t from, const uint32_t* ids, const uint32_t* deg, int R, std::vector<uint8_t>& reached, std::vector<uint32_t>& stack) {
  reached[from] = 1;
  stack.push_back(from);
  while (!stack.empty()) {
    const uint32_t x = stack.back();
    stack.pop_back();
    for (uint32_t j = 0; j < deg[x]; ++j) {
      const uint32_t y = ids[(size_t)x * R + j];
      if (!reached[y]) {
        reached[y] = 1;
        stack.push_back(y);
      }
    }
  }
}

constexpr int TRACE_K = 32;               // closest evaluated nodes kept of every orphan's search
constexpr unsigned long long TRACE_EMPTY = ~0ull;   // end of a shorter trace (the kernels' KEY_EMPTY); a trace key carries the node id in its low word

// FindUnconnectedNode (nsg.cpp:734-775): the lowest-id unreached node x gets an in-edge from the closest REACHED node of a search for V[x]; the
// DFS then continues through x, so only one node per unreached component receives an extra edge.  The searches of all initially unreached
// nodes have run as one device batch (top[i * TRACE_K ..]: the closest evaluated nodes of orphans[i]'s search, ascending); the attach +
// DFS-continue loop runs here in id order against the live `reached` set.  Returns the (root, orphan) edges in the order found.
// Out-degree stays <= deg_cap (the reference has no cap: on hub-prone data its repair edges pile up on a few nodes - 291 edges on one node at
// 1M x 768): a saturated node passes the orphan on to the next closest reached node of the trace, so every adjacency list keeps the fixed
// 256-byte stride the traversal kernel reads with one row fetch.
inline std::vector<std::pair<uint32_t, uint32_t>> repair_orphans(int64_t n, int R, const uint32_t* ids, const uint32_t* deg, const std::vector<uint32_t>& orphans,
                                                                 const unsigned long long* top, std::vector<uint8_t>& reached, uint32_t deg_cap, uint64_t lcg) {
  std::vector<std::pair<uint32_t, uint32_t>> extra;
  std::vector<uint32_t> live_extra((size_t)n, 0);
  std::vector<uint32_t> stack;
  for (size_t i = 0; i < orphans.size(); ++i) {
    const uint32_t x = orphans[i];
    if (reached[x]) continue;   // linked through an earlier orphan's subtree
    int64_t root = -1;
    for (int e = 0; e < TRACE_K; ++e) {
      const unsigned long long key = top[i * TRACE_K + e];
      if (key == TRACE_EMPTY) break;
      const uint32_t c = (uint32_t)key;
      if (reached[c] && deg[c] + live_extra[c] < deg_cap) {
        root = c;
        break;
      }
    }
    while (root < 0) {          // a random linked node (nsg.cpp:763-771), here one that still has room
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      const uint32_t c = (uint32_t)((lcg >> 33) % (uint64_t)n);
      if (reached[c] && deg[c] + live_extra[c] < deg_cap) root = c;
    }
    live_extra[root]++;
    extra.emplace_back((uint32_t)root, x);
    mark_reached(x, ids, deg, R, reached, stack);
  }
  return extra;
}

// CSR in the reference's layout (ann_graph_segment.cpp:222-241): every node's edges in list order, then its repair edges in the order found
inline void graph_csr(int64_t n, int R, const uint32_t* ids, const uint32_t* deg, const std::vector<std::pair<uint32_t, uint32_t>>& extra, std::vector<int64_t>& off,
                      std::vector<int64_t>& nbr) {
  off.assign((size_t)n + 1, 0);
  std::vector<uint32_t> extra_cnt((size_t)n, 0);
  for (auto& pr : extra) extra_cnt[pr.first]++;
  int64_t e = 0;
  for (int64_t i = 0; i < n; ++i) {
    off[i] = e;
    e += deg[i] + extra_cnt[i];
  }
  off[n] = e;
  nbr.assign((size_t)e, 0);
  std::vector<int64_t> fill((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    for (uint32_t j = 0; j < deg[i]; ++j) nbr[off[i] + j] = ids[(size_t)i * R + j];
    fill[i] = off[i] + deg[i];
  }
  for (auto& pr : extra) nbr[fill[pr.first]++] = pr.second;
}

// fixed-stride u32 lists with degrees -> the ABI's int64 lists (-1 behind every list's end) and int32 degrees
inline void lists_to_abi(const uint32_t* ids, const uint32_t* deg, int64_t rows, int R, int64_t* out_ids, int32_t* out_deg) {
  for (int64_t v = 0; v < rows; ++v) {
    out_deg[v] = (int32_t)deg[v];
    for (int j = 0; j < R; ++j) out_ids[v * R + j] = (uint32_t)j < deg[v] ? (int64_t)ids[(size_t)v * R + j] : -1;
  }
}

// ------------------------------------------------------------------------------------------------ LDS layouts
// One struct of byte offsets per kernel, computed by one function that the host sizes the launch with (total) and the kernel carves its
// pointers from (smem_raw + l.field): an array the one side has and the other lacks cannot exist.  Offsets ascend in field order; a field
// marked "over X" is an overlay - it names bytes of X that X does not use while the overlay is live.
EPS_GRAPH_HD inline size_t lds_up16(size_t b) { return (b + 15) & ~(size_t)15; }
EPS_GRAPH_HD inline int lds_qstride(int dim) { return (dim + 3) & ~3; }   // floats of a staged row: dim rounded up to a 16-byte piece

// The 8-bit prefilter's block, last in its kernel's layout: the query's four statistics, then the query on the mirror's 8-bit grid.  The block
// starts on the next multiple of 16 at or behind `at`; `bytes` is what a launch with the block adds to its total, 16 of them for that round-up.
EPS_GRAPH_HD inline int q8_bytes(int dim, int cols8) { return ((cols8 > dim ? cols8 : dim) + 15) & ~15; }   // the query on the grid
struct Pf8Lds {
  size_t qst;   // float [4] |q|^2, |q|, |q - qh|, C + c
  size_t sq8;   // signed char [q8_bytes]
  size_t bytes;
};
EPS_GRAPH_HD inline Pf8Lds pf8_lds(size_t at, int dim, int cols8) {
  Pf8Lds l;
  l.qst = lds_up16(at);
  l.sq8 = l.qst + 16;
  l.bytes = 16 + 16 + (size_t)q8_bytes(dim, cols8);
  return l;
}

// ---- the build's kernels
constexpr int PRUNE_POOL = 4096;   // sorted candidate pool per node of prune_kernel (LDS)
constexpr int TRV_HASH = 8192;     // LDS visited hash slots of traverse_kernel (HASHVIS mode), power of two
constexpr int TRV_CHUNK = 256;     // neighbours traverse_kernel handles per sub-round
constexpr int BUILD_MAX_DIM = 8192;   // widest row the library accepts
constexpr int PRUNE_PB = 4;        // candidates prune_kernel judges per round of its SelectEdge walk

struct PruneLds {
  size_t sq;      // float [qstride] V[v]
  size_t pool;    // u64 [PRUNE_POOL]
  size_t kept;    // u32 [R] kept ids ...
  size_t keptd;   // float [R] ... and their distances
  size_t sh;      // int [64] scalars (PruneSlot)
  size_t sqb;     // float [PRUNE_PB][qstride] staged candidate vectors of the SelectEdge walk, 16-byte aligned
  size_t total;
};
EPS_GRAPH_HD inline PruneLds prune_lds(int dim, int R) {
  const size_t qrow = (size_t)lds_qstride(dim) * 4;
  PruneLds l;
  l.sq = 0;
  l.pool = l.sq + qrow;
  l.kept = l.pool + (size_t)PRUNE_POOL * 8;
  l.keptd = l.kept + (size_t)R * 4;
  l.sh = l.keptd + (size_t)R * 4;
  l.sqb = lds_up16(l.sh + 64 * 4);
  l.total = l.sh + 64 * 4 + 16 + PRUNE_PB * qrow;   // (16: sqb's round-up)
  return l;
}
EPS_GRAPH_HD inline size_t prune_lds_bytes(int dim, int R) { return prune_lds(dim, R).total; }
enum PruneSlot {   // prune_kernel's sh[]
  PRN_FILL = 0,     // keys in the pool
  PRN_NK = 1,       // edges kept
  PRN_CURSOR = 2,   // next pool position of the walk
  PRN_PASSED = 3,   // pool positions passed (repeats not counted)
  PRN_TIES = 4,     // copies of the threshold key taken into an overfull pool
  PRN_NB = 6,       // members of this round's batch
  PRN_WAVE = 8,     // [4] per-wave counts
  PRN_POS = 16,     // [PRUNE_PB] pool position of batch member b
  PRN_KEPT_CLOSER = 24,   // [PRUNE_PB] "a row kept before the batch is closer to member b than v is"
  PRN_PEER_CLOSER = 32,   // [PRUNE_PB][PRUNE_PB] "batch member b2 (< b) is closer to member b than v is"
};

struct TrvLds {
  size_t sq;       // float [qstride] the query
  size_t queue;    // u64 [Lp2]
  size_t newk;     // u64 [TRV_CHUNK] unsorted keys of this sub-round
  size_t sorted;   // u64 [TRV_CHUNK]
  size_t surv;     // over sorted: u32 [TRV_CHUNK] ids that passed the 8-bit test (step 3a; `sorted` is written from step 4 on)
  size_t work;     // u32 [TRV_CHUNK] surviving neighbour ids
  size_t sh;       // int [64] scalars (TrvSlot)
  size_t hash;     // u32 [TRV_HASH] visited hash, when it lives in LDS
  Pf8Lds pf;       // prefilter only
  size_t total;
};
EPS_GRAPH_HD inline TrvLds traverse_lds(int dim, int Lp2, bool hash_in_lds, bool prefilter, int cols8) {
  TrvLds l;
  l.sq = 0;
  l.queue = l.sq + (size_t)lds_qstride(dim) * 4;
  l.newk = l.queue + (size_t)Lp2 * 8;
  l.sorted = l.newk + TRV_CHUNK * 8;
  l.surv = l.sorted;
  l.work = l.sorted + TRV_CHUNK * 8;
  l.sh = l.work + TRV_CHUNK * 4;
  l.hash = l.sh + 64 * 4;
  const size_t end = l.hash + (hash_in_lds ? TRV_HASH * 4 : 0);
  l.pf = pf8_lds(end, dim, cols8);
  l.total = end + (prefilter ? l.pf.bytes : 0);
  return l;
}
EPS_GRAPH_HD inline size_t traverse_lds_bytes(int dim, int Lp2, bool hashvis, bool prefilter = false, int cols8 = 0) {
  return traverse_lds(dim, Lp2, hashvis, prefilter, cols8).total;
}
constexpr int TRV_MAXM = 16;   // expansions of traverse_kernel per round, at most
enum TrvSlot {   // traverse_kernel's sh[]
  TRV_NWORK = 0,    // ids to evaluate in this chunk
  TRV_NSEL = 1,     // candidates selected this round
  TRV_K = 2,        // first possibly-unchecked queue position
  TRV_NNEW = 3,     // keys of this chunk that passed the bound
  TRV_RMIN = 4,     // lowest insert position of this chunk
  TRV_SELPOS = 5,   // position of the first selected candidate
  TRV_HFILL = 6,    // fill of the visited hash
  TRV_LOGFILL = 7,  // keys logged
  TRV_NODE = 8,     // [TRV_MAXM] selected node ids
  TRV_EDGE0 = 24,   // [TRV_MAXM + 1] first edge of every selected node
  TRV_TQ = 41,      // prefilter threshold of this chunk
  TRV_NSURV = 42,   // prefilter survivors of this chunk
  TRV_FP32 = 43,    // fp32 rows read in step 3
  TRV_WAVE = 48,    // [4] per-wave counts
};

struct Refusal {   // what IndexBase::fail takes
  int32_t code = EPS_OK, err_class = 0;
  std::string msg;
};

// What a build's two LDS-hungry kernels need against what a workgroup of the device can have (lds_limit bytes), BEFORE anything is launched:
// a launch above the limit fails inside the runtime, and the caller would read a HIP error string.  need = the larger of the Link search
// (queue of Lp2 keys, visited hash in LDS when hashvis) and SelectEdge at out-degree R.  The refusal names the widest row the same build
// would still run with, found by arithmetic on the two layouts.
inline size_t build_lds_need(int dim, int R, int Lp2, bool hashvis, bool prefilter, int cols8) {
  return std::max(prune_lds_bytes(dim, R), traverse_lds_bytes(dim, Lp2, hashvis, prefilter, cols8));
}
inline int32_t build_lds_check(int dim, int R, int Lp2, bool hashvis, bool prefilter, int cols8, size_t lds_limit, Refusal* r) {
  const size_t need = build_lds_need(dim, R, Lp2, hashvis, prefilter, cols8);
  if (need <= lds_limit) return EPS_OK;
  int widest = 0;   // largest multiple of 4 that fits (the mirror row of another width is not known here: the width itself stands in)
  for (int w = 4; w <= BUILD_MAX_DIM; w += 4)
    if (build_lds_need(w, R, Lp2, hashvis, prefilter, 0) <= lds_limit) widest = w;
  r->msg = "build: rows of " + std::to_string(dim) + " dimensions need " + std::to_string(need) + " bytes of LDS per workgroup, the device has " +
           std::to_string(lds_limit) + " (width limit of the graph build at out_degree " + std::to_string(R) + ": " + std::to_string(widest) + " dimensions)";
  r->err_class = EPS_ERRCLASS_DEVICE_RANGE;
  return r->code = EPS_DB_UNSUPPORTED_ERROR;
}

// ------------------------------------------------------------------------------------------------ LDS layout of traverse2_kernel
constexpr int TRV2_SB = 4096;       // keys of the LDS staging block of the QGLOBAL bitonic sort
constexpr int TRV2_MAXT = 128;      // the reference's limit for IntraQueryThreads (config/config.hpp:29)
// ints of scalar scratch: 16 scalars (Trv2Slot), nine [TS] per-worker arrays, [16] per-wave counts, [TS + 16] edge offsets; TS = T rounded up to 16
EPS_GRAPH_HD inline int trv2_tstride(int T) { return T <= 16 ? 16 : (T + 15) & ~15; }
EPS_GRAPH_HD inline int trv2_sh_ints(int T) { return 48 + 10 * trv2_tstride(T); }
enum Trv2Slot {   // traverse2_kernel's sh[0..16)
  TRV2_SCRATCH = 0,    // longest chunk count of a queue insert
  TRV2_VLOG = 2,       // undo-log fill
  TRV2_ANYSEL = 3,     // a worker selected a candidate this step
  TRV2_PREFIX = 4,     // running prefix (PickTopMToWorkers, MergeAll)
  TRV2_VLOG_OVER = 7,  // the undo log overflowed
  TRV2_ELOG = 8,       // evaluations logged (elog)
  TRV2_TQ = 9,         // prefilter threshold of this step
  TRV2_NEVAL = 10,     // prefilter form: nodes to evaluate this step
};
// slots of the per-step table of edge owners: power of two >= 2*T*dp, 0 when T == 1
EPS_GRAPH_HD inline int traverse2_hash_slots(int T, int dp) {
  if (T <= 1) return 0;
  int h = 64;
  while (h < 2 * T * dp) h <<= 1;
  return h;
}
struct Trv2Lds {   // ecap = T * dp edge slots of a step
  int H;           // slots of the owner table (traverse2_hash_slots)
  size_t sq;       // float [qstride] the query
  size_t qlds;     // u64 [qtot] the queues, or [TRV2_SB] the sort's staging block when they live in HBM
  size_t newk;     // u64 [ecap] keys of this step, per worker segment
  size_t eacc;     // over newk: int [ecap] row constant per edge slot (steps b-c; `newk` is written from step d on) ...
  size_t wacc;     // over newk: int [ecap] ... and per entry of `work` (steps c-d0)
  size_t sorted;   // u64 [ecap]
  size_t wwk;      // over sorted, first half: u32 [ecap] worker of every entry of `work` (steps c-d0; `sorted` is written in step e)
  size_t surv;     // over sorted, second half: u32 [ecap] ids that passed the 8-bit test (step d0)
  size_t eid;      // u32 [ecap] neighbour id per edge slot
  size_t eraw;     // u32 [ecap] 1 = this slot's test-and-set made the node visited
  size_t work;     // u32 [ecap] ids to evaluate, per worker segment
  size_t npos;     // int [ecap] insert positions
  size_t hid;      // u32 [H] node id of the owner table, TRV2_NONE = empty
  size_t hmin;     // int [H] lowest edge slot that met the node this step
  size_t auxl;     // int [2 * Lq] MergeAll scratch (queues in LDS and T > 1)
  size_t sh;       // int [trv2_sh_ints(T)]
  Pf8Lds pf;       // prefilter only
  size_t total;
};
// qglobal = queues in HBM
EPS_GRAPH_HD inline Trv2Lds traverse2_lds(int dim, int T, int Lq, int64_t qtot, int dp, bool qglobal, bool prefilter, int cols8) {
  Trv2Lds l;
  l.H = traverse2_hash_slots(T, dp);
  const size_t ecap = (size_t)T * dp, H = (size_t)l.H;
  l.sq = 0;
  l.qlds = l.sq + (size_t)lds_qstride(dim) * 4;
  l.newk = l.qlds + (qglobal ? (size_t)TRV2_SB : (size_t)qtot) * 8;
  l.eacc = l.newk;
  l.wacc = l.eacc + ecap * 4;
  l.sorted = l.newk + ecap * 8;
  l.wwk = l.sorted;
  l.surv = l.wwk + ecap * 4;
  l.eid = l.sorted + ecap * 8;
  l.eraw = l.eid + ecap * 4;
  l.work = l.eraw + ecap * 4;
  l.npos = l.work + ecap * 4;
  l.hid = l.npos + ecap * 4;
  l.hmin = l.hid + H * 4;
  l.auxl = l.hmin + H * 4;
  l.sh = l.auxl + ((qglobal || T == 1) ? 0 : (size_t)2 * Lq * 4);
  const size_t end = l.sh + (size_t)trv2_sh_ints(T) * 4;
  l.pf = pf8_lds(end, dim, cols8);
  l.total = end + (prefilter ? l.pf.bytes : 0);
  return l;
}
// LDS bytes of one workgroup
EPS_GRAPH_HD inline size_t traverse2_lds_bytes(int dim, int T, int Lq, int64_t qtot, int dp, bool qglobal, bool prefilter = false, int cols8 = 0) {
  return traverse2_lds(dim, T, Lq, qtot, dp, qglobal, prefilter, cols8).total;
}

// The 8-bit test pays only where it settles most neighbours: where more than 60 % of the neighbour evaluations still read the fp32 row
// (distances small against the table's value range: clustered / low intrinsic dimension) it is pure overhead.  No evaluations: no verdict.
inline bool prefilter_pays(double neighbour_evals, double fp32_rows_read) { return !(neighbour_evals > 0 && fp32_rows_read > 0.6 * neighbour_evals); }

// ------------------------------------------------------------------------------------------------ launch plan of a traversal
struct TrvIn {
  int64_t n_indexed, nq;
  int dim;
  int64_t master_queue, local_queue;   // the caller's SearchQueueSize, LocalQueueSize ...
  int intra_threads;                   // ... IntraQueryThreads
  int64_t sync_interval;               // ... GlobalSyncInterval
  int fixed_deg;                       // stride of the device lists, 0: CSR
  int64_t max_degree;
  bool prefilter;                      // the 8-bit prefilter runs (its block is part of the LDS need) ...
  int cols8;                           // ... over this many leading bytes of a mirror row
  int cus;
  int waves;                           // wavefronts per query the caller forces (EPS_TRV_WAVES), 0: the plan's choice
  bool filter_in_traversal, filtered;  // asked for / in effect for this call
  int64_t ecap_min;                    // slots of the evaluation log an earlier attempt of this call found necessary
};

struct TrvPlan {
  // queue layout (trv_queues)
  int64_t L, Lq;   // SearchQueueSize clamped to n; the capacity a worker's queue is laid out with
  int Lp2, I;      // next power of two >= L; expansions per worker and round
  int dp;          // edge slots per worker and step
  int hslots;
  int64_t qtot;    // keys of queue storage per slot = (T-1)*Lq + Lp2
  // launch (trv_launch)
  bool qglobal;    // queues in HBM
  int nw;          // wavefronts per query: 4, 8 or 16
  size_t shm;      // LDS bytes of a workgroup
  int per_cu;      // workgroups per CU
  int64_t words;   // u32 words of a slot's visited bitmap
  int64_t slots;   // visited sets = workgroups of a launch
  int vcap;        // entries of a slot's undo log
  int64_t ecap_plan;   // slots of a query's evaluation log (filtered traversal)
  int64_t slice;   // queries per launch
};

// The reference accepts SearchQueueSize up to 10^7 and IntraQueryThreads up to 128 (config/config.hpp:28-44).  What the device does not run
// it refuses - it never runs a different configuration than the one asked for.
inline int32_t trv_queues(const TrvIn& in, TrvPlan* p, Refusal* r) {
  auto refuse = [&](const std::string& msg) {
    r->msg = msg;
    r->err_class = EPS_ERRCLASS_DEVICE_RANGE;
    return r->code = EPS_DB_UNSUPPORTED_ERROR;
  };
  const int64_t n = in.n_indexed;
  int64_t L = in.master_queue;
  if (L > n) L = n;  // the reference would spin forever in PrepareInitIds when L > n (see seed_list)
  if (L > ((int64_t)1 << 20)) return refuse("search: SearchQueueSize > 1048576 is not supported (use the flat engines)");
  int64_t Lq = in.local_queue;
  if (Lq > n) Lq = n;
  if (Lq > ((int64_t)1 << 20)) return refuse("search: LocalQueueSize > 1048576 is not supported (use the flat engines)");
  const int T = in.intra_threads;
  if (T > TRV2_MAXT) return refuse("search: IntraQueryThreads > 128 is not supported (the reference's own limit, config/config.hpp:29)");
  const int I = (int)std::min<int64_t>(in.sync_interval, 1 << 20);
  int Lp2 = 1;
  while (Lp2 < L) Lp2 <<= 1;
  const int dp = (int)(((in.fixed_deg > 0 ? (int64_t)in.fixed_deg : std::max<int64_t>(in.max_degree, 1)) + 7) / 8 * 8);
  if ((int64_t)T * dp > 2048)   // the T adjacency lists of one lockstep step share the workgroup's LDS
    return refuse("search: IntraQueryThreads x maximum out-degree (rounded up to 8) > 2048 is not supported: " + std::to_string(T) + " x " + std::to_string(dp) +
                  " (at the build's out-degree cap of 64: IntraQueryThreads <= 32)");
  // r6: the capacity a worker's queue is LAID OUT with.  Between two MergeAllQueuesToMaster calls (which empty it, :297-326) a worker's queue holds its
  // share of the master's unchecked candidates - PickTopMToWorkers deals them round-robin, every T-th stays with the master: <= ceil(L / T) (:328-356) -
  // plus what its <= I expansions of the round insert, <= out-degree each (:384-444).  A capacity above that bound never clamps an insert and never
  // stops the dealing early, so the walk with LocalQueueSize = min(LocalQueueSize, bound) is the walk with LocalQueueSize, key for key
  // (test_lockstep_workers_match_oracle holds whole queues against the oracle, which keeps the caller's value).  What it buys: T = 4, L = 2000
  // needs 3 x 1460 + 2048 keys instead of 3 x 2000 + 2048 - the queues stay in LDS where the larger layout sent them to HBM.
  if (T > 1) Lq = std::min<int64_t>(Lq, (L + T - 1) / T + (int64_t)I * dp);
  p->L = L;
  p->Lq = Lq;
  p->Lp2 = Lp2;
  p->I = I;
  p->dp = dp;
  p->hslots = traverse2_hash_slots(T, dp);
  p->qtot = (int64_t)(T - 1) * Lq + Lp2;
  return EPS_OK;
}

// The rest of the plan, once it is known whether the prefilter runs (in.prefilter, in.cols8) and on how many CUs (in.cus).
inline void trv_launch(const TrvIn& in, TrvPlan* p) {
  const int64_t n = in.n_indexed, nq = in.nq, L = p->L;
  const int T = in.intra_threads;
  // queues in LDS while a workgroup's working set leaves room for at least two workgroups per CU (the row gathers of
  // the other one cover this one's queue maintenance); larger SearchQueueSize: queues in HBM
  // Between 80 and 150 KB the queues still fit the CU's LDS once: one workgroup of 16 wavefronts per CU then beats queues in
  // HBM with 4 x 4 wavefronts (T = 4, L = 2000 at 10M x 768, batch 1024: 80 ms vs 108 ms); beyond that: queues in HBM.
  const size_t lds_need = traverse2_lds_bytes(in.dim, T, (int)p->Lq, p->qtot, p->dp, false, in.prefilter, in.cols8);
  // r3 (scripts/lab/trv_large_l2.sh, bench_random_graph.py): for BATCHES that band is better served with the queues in HBM and 8
  // wavefronts per query, two queries per CU (T = 4, L = 2000, batch 1024: 1M x 768 46.6 -> 39.4 ms, 10M-row proxy 56.8 -> 49.3 ms;
  // 4 wavefronts 64.6, 16 wavefronts 66.1), and 8 wavefronts also beat the 4 that queues in HBM used to get (L = 4000: 126.6 ->
  // 93.6 ms, L = 8000: 350.8 -> 246.7 ms).  A handful of queries (<= 256, latency) keeps the one-workgroup-per-CU form.
  const size_t lds_limit = nq <= 256 ? (size_t)150 * 1024 : (size_t)80 * 1024;
  p->qglobal = lds_need > lds_limit;
  const bool one_per_cu = !p->qglobal && lds_need > (size_t)80 * 1024;
  p->shm = traverse2_lds_bytes(in.dim, T, (int)p->Lq, p->qtot, p->dp, p->qglobal, in.prefilter, in.cols8);
  // few queries: 16 wavefronts per query (latency); many queries: fewer per query (throughput, more queries per CU)
  // r6: LDS queues that leave room for only TWO workgroups per CU (40-80 KB: T = 4 from L ~ 600) get 8 wavefronts each - 16 per CU as with four small
  // workgroups, and the step's T x degree rows spread over twice the lanes (10M x 768 proxy, batch 1024, T = 4: L = 700 14.3 -> 12.5 ms, L = 1000
  // 18.8 -> 17.1, L = 2000 37.1 -> 33.3 where HBM queues took 42.5; 16 wavefronts: 17.1 / 23.4 / 45.7 - profiles/r6_traverse_large_queues_proxy.txt)
  int nw = in.waves ? in.waves : ((nq <= 256 || one_per_cu) ? 16 : ((p->qglobal || p->shm > (size_t)40 * 1024) ? 8 : 4));
  if (nw != 4 && nw != 8 && nw != 16) nw = 4;
  p->nw = nw;
  int per_cu = (int)std::min<size_t>((size_t)(16 / nw), (size_t)(160 * 1024) / p->shm);   // 4 wavefronts per SIMD at this register use (~104 VGPRs)
  if (per_cu < 1) per_cu = 1;
  p->per_cu = per_cu;
  p->words = (n + 31) / 32;
  int64_t slots = std::min<int64_t>(nq, (int64_t)in.cus * per_cu);
  slots = std::min<int64_t>(slots, std::max<int64_t>(1, ((int64_t)4 << 30) / (p->words * 4)));
  if (p->qglobal) slots = std::min<int64_t>(slots, std::max<int64_t>(1, ((int64_t)8 << 30) / (p->qtot * 8)));
  p->slots = slots;
  p->vcap = (int)std::min<int64_t>((int64_t)1 << 20, std::max<int64_t>(1024, p->words / 4));
  // results of the traversal are consumed per slice of queries so that the [slice][L] queue copy stays below 2 GiB
  // filtered traversal: slots of a query's evaluation log - every distance the walk evaluates is logged; a walk that evaluates more
  // (large T x I, high degree) reports it and the search is repeated with a log that holds them all (ecap_min)
  p->ecap_plan = std::min<int64_t>(n, std::max<int64_t>(std::max<int64_t>(16384, 64 * L), in.ecap_min));
  p->slice = std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)2 << 30) / (std::max<int64_t>(L, in.filter_in_traversal ? p->ecap_plan : 0) * 8)));
}

inline int32_t trv_plan(const TrvIn& in, TrvPlan* p, Refusal* r) {
  const int32_t rc = trv_queues(in, p, r);
  if (rc == EPS_OK) trv_launch(in, p);
  return rc;
}

// ------------------------------------------------------------------------------------------------ tail merge
// Search()'s epilogue (vec_search_executor.cpp:873-927) in numbers: `limit` is the reference's limit (the walk's, or k), n_total - n_indexed
// rows are not covered by the graph yet.
struct TailPlan {
  int tail_k;          // keys of a query's tail list: only min(|tail|, limit) tail entries are ever merged (:890-899)
  int K;               // searchLimit = min(n_indexed, limit, LocalQueueSize, L): slots that take part in the tail merge
  int Klds;            // of them staged in LDS: K when there is a tail (<= 64 KB), else none, whatever K
  int Kout;            // results wanted per query
  int cand_num_tail;   // min(L, n_total)
  int cand_num;        // min(L, n_indexed)
};
inline int32_t tail_plan(int64_t n_indexed, int64_t n_total, int64_t L, int64_t local_queue, int k, int walk_limit, TailPlan* t, Refusal* r) {
  const int limit = walk_limit > 0 ? walk_limit : k;
  const bool tail = n_total > n_indexed;
  t->tail_k = std::min(limit, 8192);
  int64_t K = n_indexed;
  if (limit < K) K = limit;
  if (local_queue < K) K = local_queue;
  if (L < K) K = L;
  if (tail && K > 8192) {
    r->msg = "search: limit > 8192 with an un-indexed tail is not supported (rebuild the graph over the new rows)";
    r->err_class = 0;
    return r->code = EPS_DB_UNSUPPORTED_ERROR;
  }
  t->K = (int)K;
  t->Klds = tail ? (int)K : 0;
  t->Kout = walk_limit > 0 ? k : (int)K;
  t->cand_num_tail = (int)std::min<int64_t>(L, n_total);
  t->cand_num = (int)std::min<int64_t>(L, n_indexed);
  return EPS_OK;
}

}  // namespace eps
