// Windowed merge of sorted lists by rank (eps_merge_range, eps_merge_range_packed, eps_merge_select, eps_exchange_allgather_merge_range): what joins
// the answers G shards gave to the same radius search or ordered select into the answer of the unsharded table.  Per query, G <= 16 lists, each
// sorted ascending; the output is ranks [skip, skip + cap) of their merged order.  There is no serial merge and no sort: every list element finds
// its own output slot,
//     rank(e in list s at position p) = p + sum over t < s of #{x in list t : x <= e} + sum over t > s of #{x in list t : x < e}
// one binary search per other list.  `<=` towards the lists before, `<` towards the lists after breaks equal keys by shard number, so the ranks of
// sorted lists are a permutation - duplicate ids across shards included - and no two elements share a slot.  An element is written iff its rank lies
// in the window; threads indexed by output slot write -1 / +inf into the slots no element can reach; the same launch writes the query's count and
// the sum of the shards' totals.  One launch, element-parallel, no workgroup waits on another.
//   keys   radius form: (ordinal of the fp32 distance as make_key computes it - -0 folded into +0, every NaN one ordinal above +inf -, 64-bit id);
//          the distance written is the ordinal's.  Select form: the id.
//   LDS    where the lists of the queries a workgroup serves fit ML_LDS_BYTES they are staged once (12 bytes per radius key, 8 per id) and searched
//          there, several queries per workgroup when a query has fewer than 256 elements; otherwise a query's elements are spread over as many
//          workgroups as it takes and searched in global memory, where a probe reads the id only when the ordinals tie.
// Traffic: every input key read once (LDS form) or 1 + (G - 1) log2(len) probes of lists that fit L2, 12 bytes written per result slot.
#include "kernels.hpp"

namespace eps {

constexpr int ML_THREADS = 256;
constexpr size_t ML_LDS_BYTES = 60 * 1024;   // staged keys of one workgroup (next to ML_THREADS list lengths: inside the 64 KB a workgroup gets by default)

template <bool DIST>
__device__ __forceinline__ int64_t ml_len(const MergeRankArgs& a, int s, int64_t j) {
  const char* p = a.counts + (int64_t)s * a.counts_stride;
  const int64_t c = DIST ? (int64_t) reinterpret_cast<const int32_t*>(p)[j] : reinterpret_cast<const int64_t*>(p)[j];
  return c < 0 ? 0 : (c > a.L ? a.L : c);   // (a count no list can hold never moves a probe outside the list)
}
__device__ __forceinline__ int64_t ml_id(const MergeRankArgs& a, int s, int64_t at) {
  return reinterpret_cast<const int64_t*>(a.ids + (int64_t)s * a.ids_stride)[at];
}
__device__ __forceinline__ u32 ml_ord(const MergeRankArgs& a, int s, int64_t at) {
  return (u32)(make_key(reinterpret_cast<const float*>(a.dist + (int64_t)s * a.dist_stride)[at], 0u) >> 32);
}
__device__ __forceinline__ bool ml_less(u32 ao, int64_t ai, u32 bo, int64_t bi) { return ao < bo || (ao == bo && ai < bi); }

// #{x in the list : x < e} (incl = false) or #{x : x <= e} (incl = true); the list: `len` sorted keys from `at` on in shard t's arrays
template <bool DIST>
__device__ __forceinline__ int64_t ml_count_global(const MergeRankArgs& a, int t, int64_t at, int64_t len, u32 eo, int64_t ei, bool incl) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    bool right;   // x[mid] belongs to the counted prefix
    if (DIST) {
      const u32 xo = ml_ord(a, t, at + mid);
      if (xo != eo) {
        right = xo < eo;
      } else {
        const int64_t xi = ml_id(a, t, at + mid);
        right = incl ? xi <= ei : xi < ei;
      }
    } else {
      const int64_t xi = ml_id(a, t, at + mid);
      right = incl ? xi <= ei : xi < ei;
    }
    if (right) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
template <bool DIST>
__device__ __forceinline__ int ml_count_lds(const int64_t* sid, const u32* sord, int at, int len, u32 eo, int64_t ei, bool incl) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const u32 xo = DIST ? sord[at + mid] : 0u;
    const int64_t xi = sid[at + mid];
    const bool right = incl ? !ml_less(eo, ei, xo, xi) : ml_less(xo, xi, eo, ei);
    if (right) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <bool DIST>
__device__ __forceinline__ void ml_write(const MergeRankArgs& a, int64_t j, int64_t rank, u32 eo, int64_t ei) {
  if (rank >= a.skip && rank - a.skip < a.cap) {
    a.out_ids[j * a.cap + (rank - a.skip)] = ei;
    if (DIST) a.out_dist[j * a.cap + (rank - a.skip)] = ord2f(eo);
  }
}
template <bool DIST>
__device__ __forceinline__ void ml_fill(const MergeRankArgs& a, int64_t j, int64_t slot) {
  a.out_ids[j * a.cap + slot] = -1;
  if (DIST) a.out_dist[j * a.cap + slot] = __builtin_inff();
}
// `sum` = the lengths of query j's lists added up
template <bool DIST>
__device__ __forceinline__ void ml_scalars(const MergeRankArgs& a, int64_t j, int64_t sum) {
  const int64_t left = sum - a.skip;
  const int64_t count = left < 0 ? 0 : (left > a.cap ? a.cap : left);
  if (a.out_counts) {
    if (DIST) static_cast<int32_t*>(a.out_counts)[j] = (int32_t)count;
    else static_cast<int64_t*>(a.out_counts)[j] = count;
  }
  if (a.out_totals) {
    int64_t total = 0;
    for (int s = 0; s < a.shards; ++s) total += reinterpret_cast<const int64_t*>(a.totals + (int64_t)s * a.totals_stride)[j];
    a.out_totals[j] = total;
  }
}

// LDS = true: workgroup b serves queries [b * per, min(nq, (b + 1) * per)), per * shards * L keys staged; blocks = ceil(nq / per).
// LDS = false: `per` workgroups serve one query, workgroup b the elements and the output slots [c * ML_THREADS, (c + 1) * ML_THREADS) of query
// b / per, c = b % per; blocks = nq * per.
template <bool DIST, bool LDS>
__global__ __launch_bounds__(ML_THREADS) void merge_rank_kernel(MergeRankArgs a, int64_t per, int64_t blocks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ml_smem[];   // LDS form: ids int64 [per * G * L] | ordinals u32 [per * G * L]
  __shared__ int64_t slen[ML_THREADS];                                      // list lengths: [queries of the workgroup][G]
  const int G = a.shards;
  const int64_t GL = (int64_t)G * a.L;
  const int tid = threadIdx.x;
  for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    if (LDS) {
      const int64_t q0 = b * per;
      const int nqb = (int)(a.nq - q0 < per ? a.nq - q0 : per);
      const int L = (int)a.L, gl = (int)GL;
      int64_t* sid = reinterpret_cast<int64_t*>(ml_smem);
      u32* sord = reinterpret_cast<u32*>(sid + per * GL);
      for (int i = tid; i < nqb * G; i += ML_THREADS) slen[i] = ml_len<DIST>(a, i % G, q0 + i / G);
      __syncthreads();
      const int ne = nqb * gl;
      for (int e = tid; e < ne; e += ML_THREADS) {
        const int q = e / gl, r = e - q * gl, s = r / L, p = r - s * L;
        if (p < (int)slen[q * G + s]) {
          const int64_t at = (q0 + q) * a.L + p;
          sid[e] = ml_id(a, s, at);
          if (DIST) sord[e] = ml_ord(a, s, at);
        }
      }
      __syncthreads();
      for (int e = tid; e < ne; e += ML_THREADS) {
        const int q = e / gl, r = e - q * gl, s = r / L, p = r - s * L;
        if (p >= (int)slen[q * G + s]) continue;
        const u32 eo = DIST ? sord[e] : 0u;
        const int64_t ei = sid[e];
        int64_t rank = p;
        for (int t = 0; t < G; ++t)
          if (t != s) rank += ml_count_lds<DIST>(sid, sord, q * gl + t * L, (int)slen[q * G + t], eo, ei, t < s);
        ml_write<DIST>(a, q0 + q, rank, eo, ei);
      }
      for (int64_t o = tid; o < nqb * a.cap; o += ML_THREADS) {
        const int q = (int)(o / a.cap);
        const int64_t slot = o - q * a.cap;
        int64_t sum = 0;
        for (int t = 0; t < G; ++t) sum += slen[q * G + t];
        if (slot >= sum - a.skip) ml_fill<DIST>(a, q0 + q, slot);
      }
      for (int q = tid; q < nqb; q += ML_THREADS) {
        int64_t sum = 0;
        for (int t = 0; t < G; ++t) sum += slen[q * G + t];
        ml_scalars<DIST>(a, q0 + q, sum);
      }
      __syncthreads();   // (the next round stages over these keys and lengths)
    } else {
      const int64_t j = b / per, c = b - j * per;
      if (tid < G) slen[tid] = ml_len<DIST>(a, tid, j);
      __syncthreads();
      int64_t sum = 0;
      for (int t = 0; t < G; ++t) sum += slen[t];
      const int64_t e = c * ML_THREADS + tid;
      if (e < GL) {
        const int s = (int)(e / a.L);
        const int64_t p = e - s * a.L;
        if (p < slen[s]) {
          const int64_t at = j * a.L + p;
          const u32 eo = DIST ? ml_ord(a, s, at) : 0u;
          const int64_t ei = ml_id(a, s, at);
          int64_t rank = p;
          for (int t = 0; t < G; ++t)
            if (t != s) rank += ml_count_global<DIST>(a, t, j * a.L, slen[t], eo, ei, t < s);
          ml_write<DIST>(a, j, rank, eo, ei);
        }
      }
      if (e < a.cap && e >= sum - a.skip) ml_fill<DIST>(a, j, e);
      if (c == 0 && tid == 0) ml_scalars<DIST>(a, j, sum);
      __syncthreads();   // (the next round's lengths)
    }
  }
}

void launch_merge_rank(const MergeRankArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.shards <= 0 || a.shards > 16) return;
  const bool dist = a.dist != nullptr;
  const int64_t GL = (int64_t)a.shards * a.L;
  const int64_t key_bytes = dist ? 12 : 8;
  const bool lds = GL * key_bytes <= (int64_t)ML_LDS_BYTES;
  int64_t per, blocks;
  size_t shm = 0;
  if (lds) {
    per = GL > 0 ? ML_THREADS / GL : ML_THREADS;   // queries per workgroup: as many as give every thread an element (per * G <= ML_THREADS: slen holds them)
    if (per < 1) per = 1;
    if (per * a.shards > ML_THREADS) per = ML_THREADS / a.shards;
    if (per > a.nq) per = a.nq;
    blocks = (a.nq + per - 1) / per;
    shm = (size_t)(per * GL * key_bytes);
  } else {
    const int64_t items = GL > a.cap ? GL : a.cap;   // elements to place, slots to fill
    per = (items + ML_THREADS - 1) / ML_THREADS;
    blocks = a.nq * per;
  }
  const unsigned grid = (unsigned)(blocks < (int64_t)1 << 30 ? blocks : (int64_t)1 << 30);   // (beyond: the kernel's loop)
  if (dist) {
    if (lds) hipLaunchKernelGGL((merge_rank_kernel<true, true>), dim3(grid), dim3(ML_THREADS), shm, s, a, per, blocks);
    else hipLaunchKernelGGL((merge_rank_kernel<true, false>), dim3(grid), dim3(ML_THREADS), 0, s, a, per, blocks);
  } else {
    if (lds) hipLaunchKernelGGL((merge_rank_kernel<false, true>), dim3(grid), dim3(ML_THREADS), shm, s, a, per, blocks);
    else hipLaunchKernelGGL((merge_rank_kernel<false, false>), dim3(grid), dim3(ML_THREADS), 0, s, a, per, blocks);
  }
}

}  // namespace eps
