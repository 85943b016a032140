// Diverse search (eps_index_search_diverse): k rows of a query's pool by maximal marginal relevance - greedy, each step taking the row with the
// smallest lam * d(row, query) - mu * min over the selected rows s of D(row, s).  The reference has no relative; a caller of eps_index_search
// copies fetch_k rows per query to the host and runs this loop there.
//
// diverse_select_kernel: one workgroup of 256 threads per query, no workgroup waits on another.  The pool - fetch_k keys in ascending order, as a
// flat search or search_among left them - stays in LDS with m (the smallest distance to a selected row so far) and a taken mark per position
// (layout: diverse_lds, diverse_host.hpp).  A step stages the row selected last in LDS as the QUERY and lets the four wavefronts stride over the
// pool with among_gather_kernel's blocking - G lanes per row, U = 4 rows in flight per group, row pointers from the keys - so D(c, s) is, bit for
// bit, what a search among the pool returns for row c when the query is row s; the lane that ends a row's sum updates m by IEEE `<`, scores
// the row with two rounded multiplies and a rounded subtract, and keeps the smallest (score ordinal, position) key it has seen; a wave
// reduction and four words through LDS give the step's row.  The last step gathers nothing.
// Row reads: (min(k, np) - 1) x np x dim x 4 bytes per query - QUADRATIC in k = fetch_k - re-read every step, from L2 where a pool fits.
#include "kernels.hpp"

namespace eps {

__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u32 lo = __shfl_xor((u32)v, o), hi = __shfl_xor((u32)(v >> 32), o);
    const u64 other = ((u64)hi << 32) | lo;
    v = other < v ? other : v;
  }
  return v;
}
// a float as every key of the library holds it: -0 as +0, any NaN as the one quiet NaN
__device__ __forceinline__ float key_float(float x) { return key_dist(make_key(x, 0u)); }

template <bool VEC4>
__global__ __launch_bounds__(DIVERSE_THREADS) void diverse_select_kernel(DiverseArgs a, int64_t q0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int U = 4;
  const int dim = a.dim, fetch_k = a.fetch_k, k = a.k;
  const int qstride = (dim + 3) & ~3;
  const DiverseLds L = diverse_lds(fetch_k, dim);
  float* const srow = reinterpret_cast<float*>(lds + L.row);
  u64* const keys = reinterpret_cast<u64*>(lds + L.keys);
  u64* const red = reinterpret_cast<u64*>(lds + L.red);
  float* const m = reinterpret_cast<float*>(lds + L.m);
  unsigned char* const taken = lds + L.taken;

  const int tid = threadIdx.x;
  const int64_t j = q0 + blockIdx.x;
  const u64* pool = a.pool + j * fetch_k;
  for (int i = tid; i < fetch_k; i += DIVERSE_THREADS) {
    keys[i] = pool[i];
    m[i] = 0.f;
    taken[i] = 0;
  }
  __syncthreads();
  int np = 0;   // the pool's size: its keys are ascending, KEY_EMPTY behind them
  for (int hi = fetch_k; np < hi;) {
    const int mid = (np + hi) >> 1;
    if (keys[mid] != KEY_EMPTY) np = mid + 1; else hi = mid;
  }
  const int sel = k < np ? k : np;
  u64* const out_keys = a.sel_keys + j * k;
  float* const out_score = a.score ? a.score + j * k : nullptr;
  for (int i = sel + tid; i < k; i += DIVERSE_THREADS) {
    out_keys[i] = KEY_EMPTY;
    if (out_score) out_score[i] = __builtin_inff();
  }
  if (sel == 0) return;

  int cur = 0;   // step 1: position 0
  if (tid == 0) {
    out_keys[0] = keys[0];
    if (out_score) out_score[0] = key_float(__fmul_rn(a.lam, key_dist(keys[0])));
    taken[0] = 1;
  }
  const int lane = lane_id();
  const int wave = tid >> 6;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);

  for (int step = 1; step < sel; ++step) {
    const float* src = a.rows + (int64_t)key_id(keys[cur]) * dim;
    for (int i = tid; i < qstride; i += DIVERSE_THREADS) srow[i] = i < dim ? src[i] : 0.f;
    __syncthreads();   // (and the mark of `cur`)
    u64 best = KEY_EMPTY;
    for (int c0 = wave * RPW * U; c0 < np; c0 += DIVERSE_WAVES * RPW * U) {
      const float* rp[U];
      int pos[U];
      bool ok[U], any = false;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ci = c0 + u * RPW + g;
        ok[u] = ci < np && !taken[ci];
        pos[u] = ok[u] ? ci : cur;   // a selected position or one beyond the pool: the staged row's pointer (row_dists' shuffles need every lane)
        rp[u] = a.rows + (int64_t)key_id(keys[pos[u]]) * dim;
        any |= ok[u];
      }
      if (__ballot(any) == 0ull) continue;   // (wave-uniform)
      float acc[U][1];
      row_dists<U, 1, VEC4>(rp, srow, qstride, dim, a.metric, G, acc);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t == 0 && ok[u]) {
          const int ci = pos[u];
          const float D = key_float(finish_dist(a.metric, acc[u][0]));
          float mm = m[ci];
          if (step == 1 || D < mm) {   // (a NaN never replaces a value, a NaN m is never replaced)
            mm = D;
            m[ci] = D;
          }
          const float score = __fsub_rn(__fmul_rn(a.lam, key_dist(keys[ci])), __fmul_rn(a.mu, mm));
          const u64 key = make_key(score, (u32)ci);
          best = key < best ? key : best;
        }
      }
    }
    best = wave_min64(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    u64 b = red[0];
#pragma unroll
    for (int w = 1; w < DIVERSE_WAVES; ++w) b = red[w] < b ? red[w] : b;
    if (b == KEY_EMPTY) break;   // (np - step > 0 positions are unselected and a score's ordinal is below KEY_EMPTY's: not reached)
    cur = (int)key_id(b);
    if (tid == 0) {
      out_keys[step] = keys[cur];
      if (out_score) out_score[step] = ord2f((u32)(b >> 32));
      taken[cur] = 1;
    }
    __syncthreads();   // red, the row and the marks are the next step's
  }
  if (tid == 0 && sel > 1)   // the (row, selected row) pairs given a distance: np - step of them in step `step`
    atomicAdd(a.evals, (unsigned long long)(sel - 1) * (unsigned long long)np - (unsigned long long)sel * (unsigned long long)(sel - 1) / 2ull);
}

void launch_diverse_select(const DiverseArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  const size_t shm = (size_t)diverse_lds(a.fetch_k, a.dim).bytes;
  const bool vec4 = rows_vec4(a.rows, a.dim);
  for (int64_t q0 = 0; q0 < a.nq; q0 += DIVERSE_GRID) {
    const dim3 grid((unsigned)(a.nq - q0 < DIVERSE_GRID ? a.nq - q0 : DIVERSE_GRID));
    if (vec4)
      hipLaunchKernelGGL((diverse_select_kernel<true>), grid, dim3(DIVERSE_THREADS), shm, s, a, q0);
    else
      hipLaunchKernelGGL((diverse_select_kernel<false>), grid, dim3(DIVERSE_THREADS), shm, s, a, q0);
  }
}

}  // namespace eps
