// Device traversal kernel of the graph build (graph_build.hip): NsgIndex::GetNeighbors (nsg.cpp:158-268), the best-first
// search of the Link step on the kNN graph, which logs the L closest nodes it evaluated for SyncPrune.  (The search path's
// traversal is traverse2_kernel.hpp.)
#pragma once
#include "traverse_steps.hpp"

namespace eps {

// ------------------------------------------------------------------------------------------------ kernel
struct TraverseArgs {
  const float* rows;
  int dim;
  int metric;
  const u32* nbr;       // [n][fixed_deg] neighbour lists padded with 0xFFFFFFFF
  int fixed_deg;
  const u32* init_ids;
  const float* queries;
  int L;       // queue length
  int Lp2;     // next power of two >= L
  int nseeds;  // number of init_ids (0: L)
  int Lsel;    // candidates are selected for expansion among the first Lsel queue positions only (0: L)
  int M;       // expansions per round
  u32* visited;      // BITMAP mode: [gridDim.x][words] in HBM
  int64_t words;
  unsigned long long* counters;  // [0] distance evals, [1] expansions, [2] (counters_n > 2) searches that filled the visited hash
  int counters_n;
  u32* ghash;        // HASHVIS: non-null = the visited hash lives in HBM, [gridDim.x][hslots] u32, pre-set to 0xFF bytes by the host
  int hslots;        //          (power of two); null = TRV_HASH slots in LDS
  u64* log;          // [nq][log_cap] plain (dist,id) keys: the final queue = the L closest evaluated nodes, ascending
  u32* log_cnt;      // [nq]
  int log_cap;       // >= L
  Prefilter8Args p8;   // exact 8-bit lower-bound prefilter of step 3 (traverse_steps.hpp); q8, qstat8: [gridDim.x] this launch's queries
};

// (TRV_HASH, TRV_CHUNK, TRV_MAXM, the kernel's LDS layout (TrvLds) and the slots of its scalar scratch (TrvSlot): graph_host.hpp)
constexpr u32 TRV_NONE = 0xFFFFFFFFu;

// test-and-set of the visited set; returns true when `id` was not visited before
// (HASHVIS: `open` = the table had room for a whole chunk of insertions when the chunk started - decided once per chunk from
// a count that is stable there, so that WHICH nodes a nearly full table still admits does not depend on thread timing)
template <bool HASHVIS>
__device__ __forceinline__ bool visit(u32* vis, u32* hash, int* hcount, u32 id, bool open = true, int hbits = 13) {
  if (!HASHVIS) {
    const u32 bit = 1u << (id & 31);
    const u32 old = atomicOr(&vis[id >> 5], bit);
    return !(old & bit);
  } else {
    if (!open) return false;  // table (nearly) full: stop discovering (build-time searches only)
    const u32 mask = (1u << hbits) - 1u;
    u32 h = (id * 2654435761u) >> (32 - hbits);
    for (u32 probe = 0; probe <= mask; ++probe) {
      const u32 old = atomicCAS(&hash[h], TRV_NONE, id);
      if (old == TRV_NONE) {
        atomicAdd(hcount, 1);
        return true;
      }
      if (old == id) return false;
      h = (h + 1) & mask;
    }
    return false;
  }
}

// one workgroup of 4 wavefronts per search (many searches in flight)
template <bool VEC4, bool HASHVIS>
__global__ __launch_bounds__(256) void traverse_kernel(TraverseArgs a) {
  constexpr int NW = 4, NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int dim = a.dim;
  const int qstride = lds_qstride(dim);
  const bool pf = a.p8.x8 != nullptr;
  const TrvLds l = traverse_lds(dim, a.Lp2, HASHVIS && !a.ghash, pf, a.p8.cols8);
  float* sq = reinterpret_cast<float*>(smem_raw + l.sq);
  u64* queue = reinterpret_cast<u64*>(smem_raw + l.queue);
  u64* newk = reinterpret_cast<u64*>(smem_raw + l.newk);
  u64* sorted = reinterpret_cast<u64*>(smem_raw + l.sorted);
  u32* surv = reinterpret_cast<u32*>(smem_raw + l.surv);
  u32* work = reinterpret_cast<u32*>(smem_raw + l.work);
  int* sh = reinterpret_cast<int*>(smem_raw + l.sh);
  u32* hash = (HASHVIS && a.ghash) ? a.ghash + (int64_t)blockIdx.x * a.hslots : reinterpret_cast<u32*>(smem_raw + l.hash);   // [TRV_HASH] in LDS (HASHVIS only) or [hslots] in HBM
  const int hbits = (HASHVIS && a.ghash) ? 31 - __clz(a.hslots) : 13;
  const int hlimit = (HASHVIS && a.ghash) ? (a.hslots / 4) * 3 : (TRV_HASH * 3) / 4;
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const int L = a.L;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  constexpr int U = 4;
  float* qst = reinterpret_cast<float*>(smem_raw + l.pf.qst);
  signed char* sq8 = reinterpret_cast<signed char*>(smem_raw + l.pf.sq8);
  const int q8len = q8_bytes(dim, a.p8.cols8);
  constexpr int U8 = 2, NL8 = 3;
  const int G8 = lanes_per_row8(q8len, NL8);
  const int RPW8 = 64 / G8;
  u32* vis = HASHVIS ? nullptr : a.visited + q * a.words;
  unsigned long long evals = 0, expansions = 0;
  u64* qlog = a.log + q * (int64_t)a.log_cap;
  if (HASHVIS) {
    if (!a.ghash)
      for (int i = tid; i < TRV_HASH; i += NT) hash[i] = TRV_NONE;
    if (tid == 0) sh[TRV_HFILL] = 0;
  }
  if (tid == 0) {
    sh[TRV_LOGFILL] = 0;
    sh[TRV_FP32] = 0;   // (read again by thread 0 only)
  }
  __syncthreads();

  stage_query<NT>(a.queries, q, dim, qstride, sq, pf, a.p8, q8len, sq8, qst);
  for (int i = tid; i < a.Lp2; i += NT) queue[i] = KEY_EMPTY;
  // InitializeSetLPara (:446-485): mark seeds visited, L seed distances, sort
  const int NS = a.nseeds > 0 ? a.nseeds : L;     // seeds (<= L)
  const int LS = a.Lsel > 0 ? a.Lsel : L;         // expansion window
  for (int i = tid; i < NS; i += NT) visit<HASHVIS>(vis, hash, &sh[TRV_HFILL], a.init_ids[i], true, hbits);
  __syncthreads();
  for (int c0 = wave * RPW * U; c0 < NS; c0 += NW * RPW * U) {
    const float* rp[U];
    u32 id[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ci = c0 + u * RPW + g;
      ok[u] = ci < NS;
      id[u] = a.init_ids[ok[u] ? ci : NS - 1];
      rp[u] = a.rows + (int64_t)id[u] * dim;
    }
    float acc[U][1];
    row_dists<U, 1, VEC4>(rp, sq, qstride, dim, a.metric, G, acc);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u] && t == 0) {
        const float d = finish_dist(a.metric, acc[u][0]);
        queue[c0 + u * RPW + g] = qkey(d, id[u]);
      }
  }
  evals += NS;
  __syncthreads();
  for (int size = 2; size <= a.Lp2; size <<= 1) bitonic_passes<NT>(queue, a.Lp2, 0, size, size >> 1);   // (padding sorts last)
  if (tid == 0) sh[TRV_K] = 0;
  __syncthreads();

  // ---- rounds
  while (true) {
    // 1. select the first M unchecked candidates at positions >= k, mark them checked
    if (tid == 0) sh[TRV_NSEL] = 0;
    __syncthreads();
    for (int base = sh[TRV_K]; base < LS; base += NT) {
      const int p = base + tid;
      const bool un = p < LS && !(queue[p] & 1ull);
      const u64 m = __ballot(un);
      if (lane == 0) sh[TRV_WAVE + wave] = __popcll(m);
      __syncthreads();
      int before = sh[TRV_NSEL];
      for (int w2 = 0; w2 < wave; ++w2) before += sh[TRV_WAVE + w2];
      const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
      if (un && rank < a.M) {
        sh[TRV_NODE + rank] = (int)((queue[p] >> 1) & 0x7FFFFFFFu);
        queue[p] |= 1ull;
        if (rank == 0) sh[TRV_SELPOS] = p;  // everything before the first selected candidate is checked
      }
      __syncthreads();
      if (tid == 0) {
        int tot = sh[TRV_NSEL];
        for (int w2 = 0; w2 < NW; ++w2) tot += sh[TRV_WAVE + w2];
        sh[TRV_NSEL] = tot < a.M ? tot : a.M;
      }
      __syncthreads();
      if (sh[TRV_NSEL] >= a.M) break;
    }
    const int nsel = sh[TRV_NSEL];
    if (nsel == 0) break;
    expansions += nsel;
    if (tid == 0) {
      sh[TRV_K] = sh[TRV_SELPOS];
      int acc = 0;
      for (int i = 0; i < nsel; ++i) {
        sh[TRV_EDGE0 + i] = acc;
        acc += a.fixed_deg;
      }
      sh[TRV_EDGE0 + nsel] = acc;
    }
    __syncthreads();
    const int total_edges = sh[TRV_EDGE0 + nsel];

    for (int e0 = 0; e0 < total_edges; e0 += TRV_CHUNK) {
      // 2. gather neighbour ids, test-and-set visited, compact survivors
      if (tid == 0) {
        sh[TRV_NWORK] = 0;
        sh[TRV_NNEW] = 0;
      }
      __syncthreads();
      const bool hash_open = !HASHVIS || sh[TRV_HFILL] + TRV_CHUNK <= hlimit;   // (sh[TRV_HFILL] is stable here: see visit())
      {
        const int e = e0 + tid;
        bool fresh = false;
        u32 nb = 0;
        if (tid < TRV_CHUNK && e < total_edges) {
          int i = 0;
          while (i + 1 < nsel && sh[TRV_EDGE0 + i + 1] <= e) ++i;
          const int64_t rowbase = (int64_t)sh[TRV_NODE + i] * a.fixed_deg;
          nb = a.nbr[rowbase + (e - sh[TRV_EDGE0 + i])];
          fresh = nb != TRV_NONE && visit<HASHVIS>(vis, hash, &sh[TRV_HFILL], nb, hash_open, hbits);
        }
        const u64 m = __ballot(fresh);
        int wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&sh[TRV_NWORK], __popcll(m));
        wbase = __shfl(wbase, 0);
        if (fresh) work[wbase + __popcll(m & ((1ull << lane) - 1ull))] = nb;
      }
      __syncthreads();
      int nwork = sh[TRV_NWORK];
      if (nwork == 0) continue;
      evals += nwork;

      // 3. distances; drop candidates beyond the current worst-of-queue (dist > bound, :427)
      const float bound = key_dist(queue[L - 1]);
      const u32* wk = work;
      if (pf) {
        // 3a. the 8-bit mirror row first: dot(xi, qi) + acc0[x] >= Tq(bound) is necessary for dist <= bound (device_common.hpp,
        //     stage_threshold8), so only the rows that pass are read in fp32.  While the queue is not full everything passes.
        if (tid == 0) {
          sh[TRV_TQ] = queue[L - 1] == KEY_EMPTY ? (int)0x80000000 : stage_threshold8(bound, qst, a.p8.scal8, a.metric, a.p8.u8, a.p8.slack8, 0);
          sh[TRV_NSURV] = 0;
        }
        __syncthreads();
        const int Tq = sh[TRV_TQ];
        const int g8 = lane / G8, t8 = lane & (G8 - 1);
        for (int c0 = wave * RPW8 * U8; c0 < nwork; c0 += NW * RPW8 * U8) {
          const signed char* rp8[U8];
          int slot[U8], dot[U8], a0[U8];
#pragma unroll
          for (int u = 0; u < U8; ++u) {
            const int ci = c0 + u * RPW8 + g8;
            slot[u] = ci < nwork ? ci : -1;
            const u32 id = work[ci < nwork ? ci : nwork - 1];
            rp8[u] = a.p8.x8 + (int64_t)id * a.p8.d_pad8;
            a0[u] = t8 == 0 ? a.p8.acc0[id] : 0;
          }
          mirror_dots<U8, NL8>(rp8, sq8, q8len, G8, t8, dot);
#pragma unroll
          for (int u = 0; u < U8; ++u)
            if (slot[u] >= 0 && t8 == 0 && dot[u] + a0[u] >= Tq) surv[atomicAdd(&sh[TRV_NSURV], 1)] = work[slot[u]];
        }
        __syncthreads();
        nwork = sh[TRV_NSURV];
        wk = surv;
        if (nwork == 0) continue;
        if (tid == 0) sh[TRV_FP32] += nwork;
      }
      for (int c0 = wave * RPW * U; c0 < nwork; c0 += NW * RPW * U) {
        const float* rp[U];
        u32 id[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ci = c0 + u * RPW + g;
          ok[u] = ci < nwork;
          id[u] = wk[ok[u] ? ci : nwork - 1];
          rp[u] = a.rows + (int64_t)id[u] * dim;
        }
        float acc[U][1];
        row_dists<U, 1, VEC4>(rp, sq, qstride, dim, a.metric, G, acc);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (ok[u] && t == 0) {
            const float d = finish_dist(a.metric, acc[u][0]);
            newk[c0 + u * RPW + g] = (d > bound) ? KEY_EMPTY : qkey(d, id[u]);
          }
        }
      }
      __syncthreads();
      // 4. rank-sort the survivors (nwork <= 256: one thread per key, broadcast LDS reads)
      if (tid < nwork) {
        const u64 mine = newk[tid];
        if (mine != KEY_EMPTY) {
          int rank = 0;
          for (int j = 0; j < nwork; ++j) {
            const u64 o = newk[j];
            rank += (o < mine) || (o == mine && j < tid);
          }
          sorted[rank] = mine;
          atomicAdd(&sh[TRV_NNEW], 1);
        }
      }
      __syncthreads();
      const int nnew = sh[TRV_NNEW];
      if (nnew == 0) continue;
      // 5. in-place parallel merge of sorted[0..nnew) into queue[0..L): read phase, barrier, write phase
      u64 oldv[4096 / NT];
      int oldp[4096 / NT];
#pragma unroll
      for (int i = 0; i < 4096 / NT; ++i) {  // L <= 4096; constant trip count keeps oldv/oldp in registers
        const int p = tid + i * NT;
        oldp[i] = L;
        oldv[i] = KEY_EMPTY;
        if (p < L) {
          const u64 v = queue[p];
          int lo = 0, hi = nnew;  // number of new keys ordered before v
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((sorted[mid] >> 1) < (v >> 1)) lo = mid + 1; else hi = mid;
          }
          oldv[i] = v;
          oldp[i] = p + lo;
        }
      }
      u64 nv = KEY_EMPTY;
      int np = L;
      if (tid < nnew) {
        nv = sorted[tid];
        int lo = 0, hi = L;  // number of old keys ordered before nv
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((queue[mid] >> 1) < (nv >> 1)) lo = mid + 1; else hi = mid;
        }
        np = tid + lo;
        if (tid == 0) sh[TRV_RMIN] = np;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4096 / NT; ++i)
        if (oldp[i] < L) queue[oldp[i]] = oldv[i];
      if (np < L) queue[np] = nv;
      __syncthreads();
      if (tid == 0 && sh[TRV_RMIN] < sh[TRV_K]) sh[TRV_K] = sh[TRV_RMIN];
      __syncthreads();
    }
    // first possibly-unchecked position: everything before the old k was checked and stays so unless a
    // new candidate landed there (handled via r_min above)
    __syncthreads();
  }
  // the log = the final queue: the L closest evaluated nodes in ascending (dist, id) order.  (Until r2 every evaluation was
  // appended to a global list of 3840 entries, which EVERY Link search of a 768-d table overran - what got logged were the
  // nodes met first, i.e. the far ones.)  With L >= candidate_pool_size this is all SyncPrune's depth-limited SelectEdge can see.
  int cnt = 0;
  for (int i = tid; i < L; i += NT) {
    const u64 k2 = queue[i];
    if (k2 != KEY_EMPTY) {
      qlog[i] = ((k2 >> 32) << 32) | ((k2 >> 1) & 0x7FFFFFFFull);
      ++cnt;
    }
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) atomicAdd(&sh[TRV_LOGFILL], cnt);
  __syncthreads();
  if (tid == 0) a.log_cnt[q] = (u32)sh[TRV_LOGFILL];
  if (tid == 0) {
    atomicAdd(&a.counters[0], evals);
    atomicAdd(&a.counters[1], expansions);
    if (pf && a.counters_n > 3) atomicAdd(&a.counters[3], (unsigned long long)sh[TRV_FP32]);   // fp32 rows step 3 still read
    if (HASHVIS && a.counters_n > 2 && sh[TRV_HFILL] + TRV_CHUNK > hlimit) atomicAdd(&a.counters[2], 1ull);   // searches that filled the visited hash
  }
}

}  // namespace eps

