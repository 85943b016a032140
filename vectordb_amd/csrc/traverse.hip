// Graph traversal path of libepsilla_gfx950: the device form of VecSearchExecutor::SearchImpl and the
// graph branch of VecSearchExecutor::Search (reference: engine/db/execution/vec_search_executor.cpp:518-715,
// 873-927; algorithm spec SURVEY.md Appendix A.2/A.4).
//
// The kernel is traverse2_kernel.hpp (one workgroup per visited-set slot walking over the queries of the batch;
// T workers with local queues in lockstep; queues in LDS or, for large SearchQueueSize, in HBM; visited bitmap
// with an undo log instead of an O(N) reset per query).  This file holds the host side: device CSR, scratch,
// PrepareInitIds, the launch, and post_kernel = the epilogue of Search() (tail merge + post-filter walk).
// With IntraQueryThreads = 1 the sequence of expansions and the final queue are exactly the reference's
// single-thread result; with T > 1 they are the reference's result under the lockstep interleaving of its
// workers (deterministic here, racy in the reference), restated by oracle/epsilla_oracle.c for parity.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "index.hpp"
#include "traverse2_kernel.hpp"

namespace eps {

struct GraphDev {
  DevBuf off;        // int64 [n+1]            (CSR form, used when max_degree > 64)
  DevBuf nbr;        // u32 [E]                (CSR) or u32 [n][fixed_deg] padded with 0xFFFFFFFF
  int fixed_deg = 0; // > 0: fixed-stride adjacency — one dependent load less per expansion than CSR
  DevBuf init_ids;   // u32 [L]
  int64_t init_L = -1;
  int64_t max_degree = 0;
  DevBuf visited;    // u32 [slots][words]: all-zero between searches (the kernel undoes what it sets)
  int64_t vis_slots = 0, vis_words = 0;
  bool vis_dirty = true;   // a failed launch may have left bits behind: re-zero before the next search
  DevBuf vlog;       // u32 [slots][vcap] undo log of the visited set
  // r5: visited set by generation stamp (Trv2Args::gens) where HBM allows - u32 [slots][n], zero-initialised once; gen_last = the last stamp handed out
  DevBuf gens;
  int64_t gens_slots = 0, gens_n = 0;
  uint32_t gen_last = 0;
  ScratchClaim gens_claim;   // r6: the table is reclaimable scratch (index.hpp) - any failed allocation of the process may take it back between searches
  GraphDev() { gens_claim.buf = &gens; }
  DevBuf qglobal;    // u64 [slots][qtot] queues of large-L searches
  DevBuf auxglobal;  // int [slots][2*Lq]
  DevBuf queue;      // u64 [nq][L]
  DevBuf counters;   // unsigned long long [2]
  DevBuf tail;       // u64 [nq][k] brute-force tail lists
  DevBuf q8, qstat8;       // prefilter: the batch on the mirror's grid, signed char [nq][d_pad8], float [nq][4]
  // r5, edge constants: the mirror's row constant (acc0) of every neighbour, stored in the adjacency list's layout ([n][fixed_deg] int32), so that
  // an expansion gets the constants of its neighbours in the access that fetches the list and the prefilter gathers nothing but the mirror rows.
  // Valid for one build of the mirror (acc0_epoch); not used while the mirror folds per-batch margins into the constants.
  DevBuf nbr_acc0;
  int64_t acc0_epoch = -1;
  // the prefilter pays only where the 8-bit bound settles most neighbours (uniform-like value distributions: 82 % at 10M x 768);
  // where distances are small against the table's value range (clustered / low intrinsic dimension) most rows pass it and it is
  // pure overhead.  Judged on what the kernel counts: two consecutive searches in which more than 60 % of the neighbour evaluations
  // still read the fp32 row switch it off for this graph (until the graph is replaced).
  int pf_strikes = 0;
  bool pf_off = false;
  DevBuf elog, elog_cnt;   // filtered traversal: u64 [slice][ecap] evaluated (dist, id) keys, u32 [slice] counts
};

void graph_free(GraphDev* g) { delete g; }

int32_t graph_upload(Index& ix) {
  if (!ix.graph_) ix.graph_ = new GraphDev();
  GraphDev& g = *ix.graph_;
  g.init_L = -1;
  g.pf_strikes = 0;
  g.pf_off = false;
  g.acc0_epoch = -1;
  if (g.gens_claim.try_enter()) {   // a new graph: the stamp table of the old one is given back (it is sized by the node count; the next search decides anew)
    g.gens.release();
    g.gens_slots = g.gens_n = 0;
    g.gens_claim.leave();
  }
  const int64_t n = ix.n_indexed_;
  if (n <= 0) return EPS_OK;
  const int64_t e = ix.h_off_[n];
  int64_t maxdeg = 0;
  for (int64_t i = 0; i < n; ++i) maxdeg = std::max(maxdeg, ix.h_off_[i + 1] - ix.h_off_[i]);
  g.max_degree = maxdeg;
  hipError_t er = hipSuccess;
  if (maxdeg > 0 && maxdeg <= 64) {
    // NSG out-degree is <= 50 (+ connectivity repair): store every list at a fixed stride so the traversal
    // reads neighbours of node v at nbr[v*deg ..] without first fetching offsets ("one coalesced
    // CSR row read each")
    const int deg = (int)((maxdeg + 3) / 4 * 4);
    std::vector<u32> pad((size_t)n * deg, 0xFFFFFFFFu);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t b = ix.h_off_[i], c = ix.h_off_[i + 1] - b;
      for (int64_t j = 0; j < c; ++j) pad[(size_t)i * deg + j] = (u32)ix.h_nbr_[b + j];
    }
    if (!g.nbr.reserve(pad.size() * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "set_graph: out of device memory");
    er = hipMemcpyAsync(g.nbr.p, pad.data(), pad.size() * 4, hipMemcpyHostToDevice, ix.stream_);
    if (er == hipSuccess) er = hipStreamSynchronize(ix.stream_);
    g.fixed_deg = deg;
  } else {
    std::vector<u32> nb32((size_t)e);
    for (int64_t i = 0; i < e; ++i) nb32[i] = (u32)ix.h_nbr_[i];
    if (!g.off.reserve((size_t)(n + 1) * 8) || !g.nbr.reserve((size_t)(e > 0 ? e : 1) * 4))
      return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "set_graph: out of device memory");
    er = hipMemcpyAsync(g.off.p, ix.h_off_.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ix.stream_);
    if (er == hipSuccess && e > 0) er = hipMemcpyAsync(g.nbr.p, nb32.data(), (size_t)e * 4, hipMemcpyHostToDevice, ix.stream_);
    if (er == hipSuccess) er = hipStreamSynchronize(ix.stream_);
    g.fixed_deg = 0;
  }
  if (er != hipSuccess) return ix.hip_fail(er, "set_graph upload");
  return EPS_OK;
}

// PrepareInitIds (vec_search_executor.cpp:487-516) over the CSR list of nav (the rule: seed_list, graph_host.hpp), kept on the device per L
static int32_t prepare_init_ids(Index& ix, GraphDev& g, int64_t L) {
  if (g.init_L == L) return EPS_OK;
  std::vector<u32> init;
  seed_list(ix.h_nbr_.data() + ix.h_off_[ix.nav_], ix.h_off_[ix.nav_ + 1] - ix.h_off_[ix.nav_], ix.nav_, ix.n_indexed_, L, init);
  if (!g.init_ids.reserve((size_t)L * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory");
  hipError_t er = hipMemcpyAsync(g.init_ids.p, init.data(), (size_t)L * 4, hipMemcpyHostToDevice, ix.stream_);
  if (er == hipSuccess) er = hipStreamSynchronize(ix.stream_);
  if (er != hipSuccess) return ix.hip_fail(er, "init ids upload");
  g.init_L = L;
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------
// Search() epilogue for one query (vec_search_executor.cpp:873-927): optional merge of the brute-force tail
// into the first K slots (MergeTwoQueuesInto1stQueueSeqFixed, :150-217 — note only K slots take part),
// then the post-filter walk over the first cand_num queue entries until K results.
struct PostArgs {
  const u64* queue;   // [nq][L] traversal keys (id<<1|checked)
  int L;
  const u64* tail;    // [nq][tail_k] flat-scan keys of the un-indexed tail (plain id), or null
  int tail_k;
  int k;              // output width
  int K;              // searchLimit = min(n_indexed, limit, L_local): slots that take part in the tail merge
  int Klds;           // slots staged in LDS: K when there is a tail to merge, else 0 (the walk then reads the queue from HBM)
  int Kout;           // results wanted per query (= K for Search(); the whole walk for eps_index_search_walk)
  int cand_num_tail;  // min(L_master, n_total)
  int cand_num;       // min(L_master, n_indexed)
  FilterSpec f;
  u64* run_keys;      // [nq][k] output keys (plain id)
};

__device__ __forceinline__ bool ckey_less(u64 a, u64 b) { return a < b; }  // plain (dist,id) keys
__device__ __forceinline__ u64 plain_key(u64 v) {  // traversal key -> (dist,id) key
  return v == KEY_EMPTY ? KEY_EMPTY : ((v & 0xFFFFFFFF00000000ull) | ((v & 0xFFFFFFFFull) >> 1));
}

// One wavefront per query.  Only the first K slots of the master queue take part in the tail merge (they are staged in
// LDS); the post-filter walk reads slots >= K straight from the queue in HBM, 64 candidates per step (ballot + prefix).
__global__ __launch_bounds__(64) void post_kernel(PostArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 m[];  // [K] head of the master queue as plain keys
  __shared__ int s_cand;
  const int64_t q = blockIdx.x;
  const int L = a.L;
  const int lane = threadIdx.x;
  const u64* qu = a.queue + q * L;
  for (int i = lane; i < a.Klds; i += 64) m[i] = plain_key(qu[i]);
  if (lane == 0) s_cand = a.cand_num;
  __syncthreads();
  if (a.tail && lane == 0) {
    const u64* bf = a.tail + q * a.tail_k;
    int n2 = 0;
    while (n2 < a.tail_k && bf[n2] != KEY_EMPTY) ++n2;
    if (n2 > 0) {
      const int n1 = a.K;
      // MergeTwoQueuesInto1stQueueSeqFixed (:150-217) on m[0..n1): lower_bound of bf[0]
      int lo = 0, hi = n1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ckey_less(m[mid], bf[0])) lo = mid + 1; else hi = mid;
      }
      const int idx = lo;
      if (idx == n1) {
        // nothing merges
      } else if (idx == n1 - 1) {
        m[idx] = bf[0];
      } else {
        if (key_id(bf[0]) != key_id(m[idx])) {
          for (int j = n1 - 1; j > idx; --j) m[j] = m[j - 1];
          m[idx] = bf[0];
        }
        int i1 = idx + 1, i2 = 1;
        for (int ins = idx + 1; ins < n1; ++ins) {
          if (i1 >= n1 || i2 >= n2) break;
          if (ckey_less(m[i1], bf[i2])) {
            ++i1;
          } else if (ckey_less(bf[i2], m[i1])) {
            for (int j = n1 - 1; j > ins; --j) m[j] = m[j - 1];
            m[ins] = bf[i2++];
            ++i1;
          } else {
            ++i2;
            ++i1;
          }
        }
      }
      s_cand = a.cand_num_tail;
    }
  }
  __syncthreads();
  const int cand_num = s_cand;
  int res = 0;
  for (int base = 0; base < cand_num && res < a.Kout; base += 64) {
    const int i = base + lane;
    u64 v = KEY_EMPTY;
    if (i < cand_num) v = i < a.Klds ? m[i] : plain_key(qu[i]);
    const bool ok = v != KEY_EMPTY && row_visible(a.f, key_id(v), key_dist(v));
    const u64 mask = __ballot(ok);
    const int rank = res + __popcll(mask & ((1ull << lane) - 1ull));
    if (ok && rank < a.Kout) a.run_keys[q * a.k + rank] = v;
    res += __popcll(mask);
  }
  if (res > a.Kout) res = a.Kout;
  for (int i = res + lane; i < a.k; i += 64) a.run_keys[q * a.k + i] = KEY_EMPTY;
}

// edge constants: out[e] = acc0[nbr[e]] (0 on the padding of a list)
__global__ void edge_acc0_kernel(const u32* nbr, const int* acc0, int* out, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const u32 v = nbr[i];
    out[i] = v == 0xFFFFFFFFu ? 0 : acc0[v];
  }
}

// ------------------------------------------------------------------------------------------------ host
template <bool VEC4, int NW, bool QG, bool PF>
static void launch_trv2(const Trv2Args& a, int slots, size_t shm, hipStream_t s) {
  // (idempotent and cheap; per call so that no process-wide state is needed)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(traverse2_kernel<VEC4, NW, QG, PF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipLaunchKernelGGL((traverse2_kernel<VEC4, NW, QG, PF>), dim3((unsigned)slots), dim3(NW * 64), shm, s, a);
}

// result keys beyond the first K of every query -> empty (the reference's result-count cap)
__global__ void cap_keys_kernel(u64* run_keys, int64_t nq, int k, int K) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq * k && (int)(i % k) >= K) run_keys[i] = KEY_EMPTY;
}

// ------------------------------------------------------------------------------------------------ the steps of one search
struct TrvCall {   // what the steps share
  Index& ix;
  GraphDev& g;
  const float* dq;
  int64_t nq;
  int k;
  u64* run_keys;
  int T;
  TrvPlan pl;
  TailPlan tp;
  FilterSpec fspec;
  bool filtered, prefilter, stamps, vec4, prof;
  Quant8View q8v;
  const int* nbr_acc0;   // edge constants, or null
  const u64* tail;       // [nq][tp.tail_k] flat-scan keys of the un-indexed tail, or null
  int64_t ecap;          // filtered traversal: slots of a query's evaluation log, else 0 ...
  int64_t Kf;            // ... and its result-count cap
};

// 8-bit lower-bound prefilter of the distance phase (traverse2_kernel.hpp, step d0): pays when a mirror row is much shorter than
// the fp32 row and the table is beyond the caches; the filtered traversal logs EVERY evaluated distance, so it cannot skip any.
// EPS_TRV_PREFILTER=0/1 (pf_env) overrides (A/B, small-table tests).
static void prefilter_view(TrvCall& c, const char* pf_env) {
  c.prefilter = !c.filtered && c.ix.dim_ >= 128 && c.ix.n_indexed_ >= 65536 && !c.g.pf_off;
  if (pf_env) c.prefilter = !c.filtered && atoi(pf_env) != 0;
  if (!c.prefilter) return;
  // the prefilter is an optimisation: if its mirror (n x d bytes, a quarter of the table) cannot be had - HBM-tight tables - the
  // walk runs on the fp32 rows as it did before the prefilter existed, and stops asking for this graph
  const int32_t rc = quant8_view(c.ix, &c.q8v);
  if (rc != EPS_OK) {
    c.q8v = Quant8View();
    c.g.pf_off = true;
  }
  c.prefilter = c.q8v.x8 != nullptr;
}

// edge constants (see GraphDev): fixed-stride lists, constants that do not change per batch, and room for one more copy of the lists
static void edge_constants(TrvCall& c) {
  GraphDev& g = c.g;
  c.nbr_acc0 = nullptr;
  if (!(c.prefilter && g.fixed_deg > 0 && !c.q8v.per_batch)) return;
  const int64_t total = c.ix.n_indexed_ * g.fixed_deg;
  if (g.acc0_epoch != c.q8v.epoch8) {
    if (g.nbr_acc0.reserve((size_t)total * 4)) {
      hipLaunchKernelGGL(edge_acc0_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65536)), dim3(256), 0, c.ix.stream_, g.nbr.as<u32>(), c.q8v.acc0,
                         g.nbr_acc0.as<int>(), total);
      g.acc0_epoch = c.q8v.epoch8;
    } else {
      (void)hipGetLastError();   // (an optimisation: without it the kernel gathers acc0[id] as before)
    }
  }
  if (g.acc0_epoch == c.q8v.epoch8) c.nbr_acc0 = g.nbr_acc0.as<int>();
}

struct ClaimHold {   // while it lives the stamp table is not reclaimable (the launches of the call use it)
  ScratchClaim& c;
  bool mine;
  explicit ClaimHold(ScratchClaim& cl) : c(cl), mine(cl.enter()) {}
  ~ClaimHold() { if (mine) c.leave(); }
};

// visited set: generation stamps (one atomicMax per edge, no reset) when 4 bytes per node and slot fit comfortably - a quarter of the free HBM
// and at most 64 GB - else the bitmap with its undo log.  EPS_TRV_VISITED=bitmap|stamps overrides (A/B, tests).  The caller holds g.gens_claim.
static int32_t ensure_visited(TrvCall& c) {
  Index& ix = c.ix;
  GraphDev& g = c.g;
  const int64_t n = ix.n_indexed_, slots = c.pl.slots;
  bool stamps = false;
  const size_t need = (size_t)slots * (size_t)n * 4;
  size_t free_b = 0, total_b = 0;
  if (!g.gens.p) g.gens_slots = g.gens_n = 0;   // (taken back since the last search)
  const bool have = (g.gens_slots >= slots && g.gens_n == n && g.gens.p);
  if (have) stamps = true;
  else if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= free_b / 4 && need <= ((size_t)64 << 30)) stamps = true;
  if (const char* ve = tune_env("EPS_TRV_VISITED")) stamps = std::strcmp(ve, "stamps") == 0 ? true : (std::strcmp(ve, "bitmap") == 0 ? false : stamps);
  if (stamps && !have) {
    g.gens.release();
    if (g.gens.reserve(need)) {
      const hipError_t er = hipMemsetAsync(g.gens.p, 0, need, ix.stream_);
      if (er != hipSuccess) return ix.hip_fail(er, "memset visited stamps");
      g.gens_slots = slots;
      g.gens_n = n;
      g.gen_last = 0;
      if (const char* st0 = tune_env("EPS_TRV_STAMP_START")) g.gen_last = (uint32_t)strtoul(st0, nullptr, 0);   // (tests: the 32-bit counter's wrap-around)
    } else {
      (void)hipGetLastError();
      g.gens_slots = g.gens_n = 0;
      stamps = false;   // (no room: the bitmap)
    }
  }
  if (!stamps && g.gens.p) {   // the bitmap serves this search: a stale stamp table is not kept beside it
    g.gens.release();
    g.gens_slots = g.gens_n = 0;
  }
  c.stamps = stamps;
  return EPS_OK;
}

// the bitmap and its undo log (unless stamps serve), the result queues, the counters, HBM queues where the plan asks for them
static int32_t reserve_scratch(TrvCall& c) {
  Index& ix = c.ix;
  GraphDev& g = c.g;
  const TrvPlan& pl = c.pl;
  hipStream_t s = ix.stream_;
  if ((!c.stamps && (!g.visited.reserve((size_t)pl.slots * pl.words * 4) || !g.vlog.reserve((size_t)pl.slots * pl.vcap * 4))) ||
      !g.queue.reserve((size_t)pl.slice * pl.L * 8) || !g.counters.reserve(256) ||
      (pl.qglobal && (!g.qglobal.reserve((size_t)pl.slots * pl.qtot * 8) || !g.auxglobal.reserve((size_t)pl.slots * 2 * pl.Lq * 4))))
    return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (traversal scratch)");
  hipError_t er;
  if (!c.stamps && (g.vis_dirty || g.vis_slots < pl.slots || g.vis_words != pl.words)) {
    // (re)establish the invariant the kernel maintains: every slot's bitmap is all-zero between searches
    er = hipMemsetAsync(g.visited.p, 0, g.visited.cap, s);
    if (er != hipSuccess) return ix.hip_fail(er, "memset visited");
    g.vis_slots = (int64_t)(g.visited.cap / ((size_t)pl.words * 4));
    g.vis_words = pl.words;
  }
  if (!c.stamps) g.vis_dirty = true;   // until this search has completed (stamps need no such care: a half-finished walk leaves only old stamps behind)
  er = hipMemsetAsync(g.counters.p, 0, 256, s);
  if (er != hipSuccess) return ix.hip_fail(er, "memset");
  return EPS_OK;
}

// the kernel's arguments but for the slice (queries, q8, qstat8, nq, out_queue, elog, elog_cnt, gen_base: run_slices)
static Trv2Args trv2_args(const TrvCall& c) {
  const Index& ix = c.ix;
  const GraphDev& g = c.g;
  const TrvPlan& pl = c.pl;
  Trv2Args a;
  a.rows = ix.d_rows_;
  a.dim = (int)ix.dim_;
  a.metric = ix.metric_;
  a.off = g.fixed_deg > 0 ? nullptr : g.off.as<int64_t>();
  a.nbr = g.nbr.as<u32>();
  a.fixed_deg = g.fixed_deg;
  a.dp = pl.dp;
  a.init_ids = g.init_ids.as<u32>();
  a.L = (int)pl.L;
  a.Lq = (int)pl.Lq;
  a.Lp2 = pl.Lp2;
  a.T = c.T;
  a.I = pl.I;
  a.qtot = pl.qtot;
  a.qglobal = pl.qglobal ? g.qglobal.as<u64>() : nullptr;
  a.auxglobal = pl.qglobal ? g.auxglobal.as<int>() : nullptr;
  a.visited = g.visited.as<u32>();
  a.words = pl.words;
  a.vlog = g.vlog.as<u32>();
  a.vcap = pl.vcap;
  a.gens = c.stamps ? g.gens.as<u32>() : nullptr;
  a.gens_n = ix.n_indexed_;
  a.gen_base = 0;
  a.counters = g.counters.as<unsigned long long>();
  a.prof = c.prof ? g.counters.as<unsigned long long>() + 8 : nullptr;
  a.elog = nullptr;
  a.elog_cnt = nullptr;
  a.elog_cap = (int)c.ecap;
  a.p8 = prefilter8_args(c.q8v, c.prefilter, ix.dim_, c.vec4);
  a.nbr_acc0 = c.nbr_acc0;
  return a;
}

static PostArgs post_args(const TrvCall& c) {
  PostArgs pa;
  pa.queue = c.g.queue.as<u64>();
  pa.L = (int)c.pl.L;
  pa.k = c.k;
  pa.tail_k = c.tp.tail_k;
  pa.K = c.tp.K;
  pa.Klds = c.tp.Klds;
  pa.Kout = c.tp.Kout;
  pa.cand_num_tail = c.tp.cand_num_tail;
  pa.cand_num = c.tp.cand_num;
  pa.f = c.ix.filter_spec();
  return pa;
}

static void launch_trv2_plan(const TrvCall& c, const Trv2Args& a, int sl) {
  const bool qglobal = c.pl.qglobal, prefilter = c.prefilter;
  const size_t shm = c.pl.shm;
  const int nw = c.pl.nw;
  hipStream_t s = c.ix.stream_;
#define EPS_TRV_LAUNCH(V4, NW_)                                        \
  do {                                                                 \
    if (qglobal) {                                                     \
      if (prefilter) launch_trv2<V4, NW_, true, true>(a, sl, shm, s);  \
      else launch_trv2<V4, NW_, true, false>(a, sl, shm, s);           \
    } else {                                                           \
      if (prefilter) launch_trv2<V4, NW_, false, true>(a, sl, shm, s); \
      else launch_trv2<V4, NW_, false, false>(a, sl, shm, s);          \
    }                                                                  \
  } while (0)
  if (c.vec4) {
    if (nw == 16) EPS_TRV_LAUNCH(true, 16); else if (nw == 8) EPS_TRV_LAUNCH(true, 8); else EPS_TRV_LAUNCH(true, 4);
  } else {
    if (nw == 16) EPS_TRV_LAUNCH(false, 16); else if (nw == 8) EPS_TRV_LAUNCH(false, 8); else EPS_TRV_LAUNCH(false, 4);
  }
#undef EPS_TRV_LAUNCH
}

// per slice of queries: the traversal, then its results into run_keys (post_kernel, or the closest visible evaluated rows)
static int32_t run_slices(TrvCall& c, Trv2Args& a, PostArgs& pa) {
  Index& ix = c.ix;
  GraphDev& g = c.g;
  hipStream_t s = ix.stream_;
  const int64_t nq = c.nq, slice = c.pl.slice;
  const int k = c.k, tail_k = c.tp.tail_k;
  (void)hipEventRecord(ix.evk0_, s);
  for (int64_t q0 = 0; q0 < nq; q0 += slice) {
    const int64_t cnt = std::min(slice, nq - q0);
    a.queries = c.dq + q0 * ix.dim_;
    a.p8.q8 = c.prefilter ? g.q8.as<signed char>() + q0 * c.q8v.d_pad8 : nullptr;
    a.p8.qstat8 = c.prefilter ? g.qstat8.as<float>() + q0 * 4 : nullptr;
    a.nq = cnt;
    a.out_queue = g.queue.as<u64>();
    if (c.filtered) {
      if (!g.elog.reserve((size_t)slice * c.ecap * 8) || !g.elog_cnt.reserve((size_t)slice * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (evaluation log)");
      a.elog = g.elog.as<u64>();
      a.elog_cnt = g.elog_cnt.as<u32>();
    }
    const int sl = (int)std::min<int64_t>(c.pl.slots, cnt);
    if (c.stamps) {   // the stamps this launch hands out: one per query of a slot; a wrap-around of the 32-bit counter starts over from a zeroed table
      const uint32_t per_slot = (uint32_t)((cnt + sl - 1) / sl);
      if (g.gen_last > 0xFFFFFFF0u - per_slot) {
        const hipError_t er = hipMemsetAsync(g.gens.p, 0, (size_t)g.gens_slots * (size_t)g.gens_n * 4, s);
        if (er != hipSuccess) return ix.hip_fail(er, "memset visited stamps");
        g.gen_last = 0;
      }
      a.gen_base = g.gen_last;
      g.gen_last += per_slot;
    }
    launch_trv2_plan(c, a, sl);
    ix.stats_.main_kernel_launches += 1;
    ix.stats_.main_kernel_bits = 32;
    if (q0 + cnt >= nq) (void)hipEventRecord(ix.evk1_, s);   // (with several slices the pair spans all traversal launches and the post kernels between them)
    pa.tail = c.tail ? c.tail + q0 * tail_k : nullptr;
    pa.run_keys = c.run_keys + q0 * k;
    if (c.filtered) {
      // the k closest visible evaluated rows (+ the visible rows of the un-indexed tail, already filtered by its flat scan)
      launch_merge_lists(a.elog, (int)c.ecap, k, cnt, c.run_keys + q0 * k, false, s, a.elog_cnt, &c.fspec);
      if (c.tail) launch_merge_lists(c.tail + q0 * tail_k, tail_k, k, cnt, c.run_keys + q0 * k, true, s);
      if (c.Kf < k) hipLaunchKernelGGL(cap_keys_kernel, dim3((unsigned)((cnt * k + 255) / 256)), dim3(256), 0, s, c.run_keys + q0 * k, cnt, k, (int)c.Kf);
    } else {
      hipLaunchKernelGGL(post_kernel, dim3((unsigned)cnt), dim3(64), (size_t)pa.Klds * 8, s, pa);
    }
  }
  const hipError_t er = hipGetLastError();
  if (er != hipSuccess) return ix.hip_fail(er, "traversal launch");
  return EPS_OK;
}

// EPS_TRV_PROF: the plan, the counters per query and the kernel's phase clocks (h: the launch's counters)
static void print_profile(const TrvCall& c, const unsigned long long* h) {
  static const char* names[10] = {"seeds+sort", "scatter", "select", "gather+visited", "dedupe", "distances", "rank sort", "queue insert", "merge-all", "results+reset"};
  const int64_t nq = c.nq, L = c.pl.L;
  unsigned long long tot = 0;
  for (int i = 0; i < 10; ++i) tot += h[8 + i];
  fprintf(stderr, "[eps trv] nq=%lld T=%d L=%lld I=%d %s queues, %d wavefronts/query, %lld slots, LDS %zu B: steps/query %.1f rounds/query %.1f expansions/query %.1f evals/query %.1f\n",
          (long long)nq, c.T, (long long)L, c.pl.I, c.pl.qglobal ? "HBM" : "LDS", c.pl.nw, (long long)c.pl.slots, c.pl.shm, (double)h[2] / nq, (double)h[3] / nq, (double)h[1] / nq, (double)h[0] / nq);
  for (int i = 0; i < 10; ++i) fprintf(stderr, "[eps trv]   %-16s %5.1f %%\n", names[i], tot ? 100.0 * h[8 + i] / tot : 0.0);
  if (c.prefilter) fprintf(stderr, "[eps trv]   8-bit prefilter: %.1f of %.1f neighbour evaluations per query read the fp32 row\n", (double)h[4] / nq, (double)(h[0] - (unsigned long long)(L * nq)) / nq);
}

// The prefilter pays only where the 8-bit bound settles most neighbours (see GraphDev::pf_strikes): two consecutive searches in which it does
// not (prefilter_pays, graph_host.hpp, over the neighbour evaluations - h[0] less the seeds - and the fp32 rows they read, h[4]) switch it off
// for this graph.
static void judge_prefilter(TrvCall& c, const unsigned long long* h) {
  const unsigned long long seeds = (unsigned long long)(c.pl.L * c.nq);
  const unsigned long long nbr_evals = h[0] > seeds ? h[0] - seeds : 0;
  if (nbr_evals < 4096) return;   // (not enough evaluations to judge)
  c.g.pf_strikes = prefilter_pays((double)nbr_evals, (double)h[4]) ? 0 : c.g.pf_strikes + 1;
  if (c.g.pf_strikes >= 2) c.g.pf_off = true;
}

int32_t graph_search_impl(Index& ix, const float* dq, int64_t nq, int k, const eps_search_params& p, u64* run_keys,
                                 int64_t* evals_out, int walk_limit, int64_t ecap_min) {
  GraphDev& g = *ix.graph_;
  const int64_t n = ix.n_indexed_, n_total = ix.n_rows_;
  hipStream_t s = ix.stream_;
  TrvCall c{ix, g, dq, nq, k, run_keys, p.intra_threads, TrvPlan(), TailPlan(), ix.filter_spec(), false, false, false, false, false, Quant8View(), nullptr, nullptr, 0, 0};
  // Filtered traversal (eps_search_params::filter_in_traversal): the reference judges deleted rows and the filter on
  // the final top-L walk only (:905-927), so a filter that lets 1 % of the rows through leaves ~L/100 results.  Here every row
  // the search EVALUATES (an order of magnitude more than L) is logged with its distance and the k closest VISIBLE ones are the
  // answer; invisible rows keep their place in the queues, i.e. the walk itself is the reference's.
  c.filtered = p.filter_in_traversal != 0 && walk_limit == 0 && (c.fspec.deleted || c.fspec.column || c.fspec.prog);
  c.vec4 = rows_vec4(ix.d_rows_, ix.dim_);
  c.prof = tune_env("EPS_TRV_PROF") != nullptr;

  // ---- plan: the queue layout and every refusal, before anything is allocated or launched
  TrvIn in{n, nq, (int)ix.dim_, p.master_queue, p.local_queue, p.intra_threads, p.sync_interval, g.fixed_deg, g.max_degree, false, 0, 0, 0,
           p.filter_in_traversal != 0, c.filtered, ecap_min};
  Refusal why;
  if (trv_queues(in, &c.pl, &why) != EPS_OK) return ix.fail(why.code, why.msg, why.err_class);
  if (c.filtered && k > 1024) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, "search: filter_in_traversal returns at most 1024 rows per query", EPS_ERRCLASS_DEVICE_RANGE);
  if (tail_plan(n, n_total, c.pl.L, p.local_queue, k, walk_limit, &c.tp, &why) != EPS_OK) return ix.fail(why.code, why.msg, why.err_class);
  int32_t rc = prepare_init_ids(ix, g, c.pl.L);
  if (rc != EPS_OK) return rc;

  // ---- prefilter view and edge constants; with them and the device's CU count, the launch plan
  const char* pf_env = tune_env("EPS_TRV_PREFILTER");
  prefilter_view(c, pf_env);
  edge_constants(c);
  const char* waves_s = tune_env("EPS_TRV_WAVES");
  hipDeviceProp_t prop;
  hipError_t er = hipGetDeviceProperties(&prop, ix.device_);
  if (er != hipSuccess) return ix.hip_fail(er, "device properties");
  in.prefilter = c.prefilter;
  in.cols8 = c.q8v.cols8;
  in.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  in.waves = waves_s ? atoi(waves_s) : 0;
  if (waves_s && in.waves == 0) in.waves = -1;   // (a value like any other that is not 4, 8 or 16: 4 wavefronts)
  trv_launch(in, &c.pl);
  c.ecap = c.filtered ? c.pl.ecap_plan : 0;
  // the result-count cap min(n_indexed, limit, LocalQueueSize) (:872) WITHOUT SearchQueueSize, which the unfiltered path's cap also holds
  // (tail_plan's K): the answer is cut from the evaluated rows, not from the queue, so limit > L may return more than L rows
  c.Kf = std::min<int64_t>(std::min<int64_t>(n, walk_limit > 0 ? walk_limit : k), p.local_queue);

  // ---- visited set (not reclaimable from here to the return of this call) and scratch
  ClaimHold hold(g.gens_claim);
  if ((rc = ensure_visited(c)) != EPS_OK || (rc = reserve_scratch(c)) != EPS_OK) return rc;

  // ---- arguments: the batch on the mirror's grid, the brute-force tail over the rows the graph does not cover yet (:885-900)
  Trv2Args a = trv2_args(c);
  if (c.prefilter) {
    if (!g.q8.reserve((size_t)nq * c.q8v.d_pad8) || !g.qstat8.reserve((size_t)nq * 16)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory");
    quant8_queries(ix, c.q8v, dq, nq, g.q8.as<signed char>(), g.qstat8.as<float>());
  }
  if (n_total > n) {
    if (!g.tail.reserve((size_t)nq * c.tp.tail_k * 8)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory");
    rc = ix.flat_stream(dq, nq, c.tp.tail_k, n, n_total, g.tail.as<u64>());
    if (rc != EPS_OK) return rc;
    c.tail = g.tail.as<u64>();
  }
  PostArgs pa = post_args(c);

  // ---- the slice loop, then the launch's counters
  if ((rc = run_slices(c, a, pa)) != EPS_OK) return rc;
  unsigned long long h[24];
  std::memset(h, 0, sizeof(h));
  er = hipMemcpyAsync(h, g.counters.p, sizeof(h), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return ix.hip_fail(er, "traversal");
  if (!c.stamps) g.vis_dirty = false;
  if (c.filtered && h[5] > 0) {
    // some query evaluated more rows than its log holds; the evaluations that were dropped are the LATE ones - the closest.  Repeat
    // with a log sized for the longest walk seen (bounded by n: a walk evaluates a row at most once)
    const int64_t need = std::min<int64_t>(n, (int64_t)h[6] + (int64_t)h[6] / 4 + 1024);
    if (need > c.ecap) return graph_search_impl(ix, dq, nq, k, p, run_keys, evals_out, walk_limit, need);
  }
  ix.stats_.dist_evals += (int64_t)h[0];
  ix.stats_.expansions += (int64_t)h[1];
  if (c.prefilter) ix.stats_.rerank_rows += (int64_t)h[4];   // fp32 rows step d still read (seeds not counted)
  if (c.prefilter && !pf_env) judge_prefilter(c, h);
  if (c.prof) print_profile(c, h);
  if (evals_out) *evals_out = (int64_t)h[0];
  return EPS_OK;
}

int32_t graph_search(Index& ix, const float* dq, int64_t nq, int k, const eps_search_params& p, u64* run_keys, int64_t* evals_out, int walk_limit) {
  return graph_search_impl(ix, dq, nq, k, p, run_keys, evals_out, walk_limit, 0);
}

}  // namespace eps
