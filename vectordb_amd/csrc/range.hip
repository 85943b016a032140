// Radius search (eps_index_search_range): every visible row whose exact fp32 distance to the query is <= the query's radius - the count of them, and
// the `cap` closest in (distance, id) order.  The threshold is known before the first row is read, so there is nothing to stage: ONE pass finds the
// survivors, one launch orders them.  Ordinary launches on the index's stream; no workgroup ever waits on another.
//   range_rerank_kernel  the tail of the matrix form: the candidates one launch of the lower-bound filter (mfma_filter.hip) let through get their
//                        exact distance - row_dists and its lane tree, as rerank_kernel / flat_scan_kernel: the bits of a flat search - and are
//                        tested: dist <= r and row_visible(f, row, dist), so a program's @distance reads the exact value.
//   range_scan_kernel    the stream form: flat_scan_kernel's row and query blocking over the fp32 rows, the same test, no top-k registers.
//   survivors            append their (distance, row) key to the query's list through a per-query counter, which keeps counting beyond the list's
//                        capacity: the counter is the total, the list holds every survivor iff total <= cap.
//   range_order_kernel   one workgroup per query: min(total, cap) keys into LDS, padded with KEY_EMPTY to a power of two, bitonic sort, ids through
//                        the id map, distances, the -1 / +inf tail, count and total.  A query whose total exceeds cap is left to the host, which
//                        takes its cap closest from flat_stream and hands them back to this kernel (a.topk) for the cut and the conversion.
// HBM traffic: stream form n x d x 4 bytes per 4 queries; matrix form the mirror once per <= 2048 queries + d x 4 bytes per candidate; 8 bytes per
// survivor written and read once; 12 bytes per result slot.
#include "kernels.hpp"

namespace eps {

__device__ __forceinline__ void range_offer(const RangeLists& L, int64_t j, float r, float dist, u32 row, const FilterSpec& f) {
  if (dist <= r && row_visible(f, row, dist)) {   // (a NaN distance is within no radius)
    const u32 slot = atomicAdd(L.cnt + j, 1u);
    if (slot < (u32)L.cap) L.keys[j * L.cap + slot] = make_key(dist, row);
  }
}

template <bool VEC4>
__global__ __launch_bounds__(256) void range_rerank_kernel(RangeRerankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [qstride] the query
  constexpr int NT = 256, NW = 4, U = 4;
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  const int64_t q = blockIdx.x;
  const u32 cnt = a.cand_count[q];
  if (cnt > (u32)a.cand_cap) {   // rows were lost to a full candidate list: the host repeats this query on the stream form
    if (threadIdx.x == 0) a.L.cnt[q] = RANGE_CNT_RESCAN;
    return;
  }
  for (int i = threadIdx.x; i < qstride; i += NT) smem[i] = i < dim ? a.queries[q * dim + i] : 0.f;
  __syncthreads();
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const float r = a.L.radius[q];
  const u32* cand = a.cand + q * (int64_t)a.cand_cap;
  for (u32 c0 = wave * RPW * U; c0 < cnt; c0 += NW * RPW * U) {   // (wave-uniform bounds: every lane takes part in row_dists' shuffles)
    const float* rp[U];
    u32 id[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const u32 ci = c0 + u * RPW + g;
      ok[u] = ci < cnt;
      id[u] = cand[ok[u] ? ci : cnt - 1];
      rp[u] = a.rows + (int64_t)id[u] * dim;
    }
    float acc[U][1];
    row_dists<U, 1, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u] && t == 0) range_offer(a.L, q, r, finish_dist(a.metric, acc[u][0]), id[u], a.f);
  }
  if (threadIdx.x == 0) atomicAdd(a.cand_total, (unsigned long long)cnt);
}

void launch_range_rerank(const RangeRerankArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  const bool vec4 = (a.dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.rows) & 15) == 0);
  const size_t shm = (size_t)((a.dim + 3) & ~3) * sizeof(float);
  if (vec4) hipLaunchKernelGGL((range_rerank_kernel<true>), dim3((unsigned)a.nq), dim3(256), shm, s, a);
  else hipLaunchKernelGGL((range_rerank_kernel<false>), dim3((unsigned)a.nq), dim3(256), shm, s, a);
}

// flat_scan_kernel's blocking: NQ queries staged in LDS per workgroup, the rows split into one chunk per wavefront, G lanes per row, U rows in flight
template <int NQ, bool VEC4, int U>
__global__ __launch_bounds__(256) void range_scan_kernel(RangeScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  const int64_t q0 = (int64_t)blockIdx.y * NQ;
  int64_t qj[NQ];   // query numbers of this block's queries (beyond the launch's last: a copy of it, never offered)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int64_t i = (q0 + q < a.nq) ? q0 + q : a.nq - 1;
    qj[q] = a.qsel ? (int64_t)a.qsel[i] : i;
  }
  for (int i = threadIdx.x; i < NQ * qstride; i += 256) {
    const int q = i / qstride, c = i - q * qstride;
    int64_t j = qj[0];
#pragma unroll
    for (int e = 1; e < NQ; ++e) j = q == e ? qj[e] : j;
    smem[i] = c < dim ? a.queries[j * dim + c] : 0.f;
  }
  __syncthreads();
  float rad[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) rad[q] = a.L.radius[qj[q]];

  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const int64_t W = (int64_t)gridDim.x * 4;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  const int64_t chunk = (a.n + W - 1) / W;
  const int64_t begin = w * chunk;
  const int64_t end = begin + chunk < a.n ? begin + chunk : a.n;
  for (int64_t r0 = begin; r0 < end; r0 += RPW * U) {
    const float* rp[U];
    int64_t row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      row[u] = r0 + u * RPW + g;
      const int64_t rc = row[u] < end ? row[u] : end - 1;
      rp[u] = a.rows + rc * dim;
    }
    float acc[U][NQ];
    row_dists<U, NQ, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t != 0 || row[u] >= end) continue;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (q0 + q < a.nq) range_offer(a.L, qj[q], rad[q], finish_dist(a.metric, acc[u][q]), (u32)row[u], a.f);
    }
  }
}

void launch_range_scan(const RangeScanArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
  const bool vec4 = (a.dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.rows) & 15) == 0);
  const size_t qbytes = (size_t)((a.dim + 3) & ~3) * sizeof(float);
  const int nq = 4 * qbytes <= 65536 ? 4 : 2;   // the block's queries are staged in LDS (dim <= 8192: two always fit)
  const dim3 grid((unsigned)(flat_scan_waves(a.n, a.nq, a.dim) / 4), (unsigned)((a.nq + nq - 1) / nq));
  if (nq == 4) {
    if (vec4) hipLaunchKernelGGL((range_scan_kernel<4, true, 4>), grid, dim3(256), 4 * qbytes, s, a);
    else hipLaunchKernelGGL((range_scan_kernel<4, false, 4>), grid, dim3(256), 4 * qbytes, s, a);
  } else {
    if (vec4) hipLaunchKernelGGL((range_scan_kernel<2, true, 4>), grid, dim3(256), 2 * qbytes, s, a);
    else hipLaunchKernelGGL((range_scan_kernel<2, false, 4>), grid, dim3(256), 2 * qbytes, s, a);
  }
}

constexpr int RANGE_ORDER_THREADS = 1024;
__global__ __launch_bounds__(RANGE_ORDER_THREADS) void range_order_kernel(RangeOrderArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 skey[];   // [cap rounded up to a power of two]
  constexpr int NT = RANGE_ORDER_THREADS;
  const int64_t i = blockIdx.x;
  const int64_t j = a.qsel ? (int64_t)a.qsel[i] : i;
  const int cap = a.L.cap;
  const u32 total = a.L.cnt[j];
  const u64* src;
  int m;   // keys to order (uniform over the workgroup)
  if (a.topk) {
    src = a.topk + i * (int64_t)cap;
    m = cap;
  } else {
    if (total == RANGE_CNT_RESCAN || total > (u32)cap) {   // the list does not hold every survivor
      if (threadIdx.x == 0) a.status[j] = total == RANGE_CNT_RESCAN ? RANGE_RESCAN : RANGE_TOPK;
      return;
    }
    src = a.L.keys + j * (int64_t)cap;
    m = (int)total;
  }
  int P = 2;
  while (P < m) P <<= 1;   // (<= cap rounded up to a power of two: what the launch reserved)
  const float r = a.L.radius[j];
  for (int e = threadIdx.x; e < P; e += NT) {
    u64 key = e < m ? src[e] : KEY_EMPTY;
    if (a.topk && key != KEY_EMPTY && !(key_dist(key) <= r)) key = KEY_EMPTY;   // the cut: beyond the radius (they sort last)
    skey[e] = key;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int h = k >> 1; h > 0; h >>= 1) {
      for (int e = threadIdx.x; e < P; e += NT) {
        const int o = e ^ h;
        if (o > e) {
          const u64 x = skey[e], y = skey[o];
          if ((x > y) == ((e & k) == 0)) {
            skey[e] = y;
            skey[o] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int e = threadIdx.x; e < cap; e += NT) {
    const u64 key = e < P ? skey[e] : KEY_EMPTY;
    const bool valid = key != KEY_EMPTY;
    a.ids_out[j * cap + e] = valid ? (int64_t)key_id(key) * a.id_stride + a.id_base : -1;
    a.dist_out[j * cap + e] = valid ? key_dist(key) : __builtin_inff();
    // the count: the sorted keys' first empty slot (keys beyond P or cap: none)
    if (a.counts_out && valid && (e + 1 >= P || e + 1 >= cap || skey[e + 1] == KEY_EMPTY)) a.counts_out[j] = e + 1;
  }
  if (threadIdx.x == 0) {
    if (a.counts_out && skey[0] == KEY_EMPTY) a.counts_out[j] = 0;
    if (a.totals_out) a.totals_out[j] = (int64_t)total;
    a.status[j] = RANGE_DONE;
  }
}

void launch_range_order(const RangeOrderArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  int P = 2;
  while (P < a.L.cap) P <<= 1;
  hipLaunchKernelGGL(range_order_kernel, dim3((unsigned)a.nq), dim3(RANGE_ORDER_THREADS), (size_t)P * sizeof(u64), s, a);
}

__global__ __launch_bounds__(256) void range_gather_kernel(const float* queries, int dim, const int32_t* qsel, float* out, u32* cnt, int zero_cnt) {
  const int64_t i = blockIdx.x;
  const int64_t j = qsel[i];
  if (out)
    for (int c = threadIdx.x; c < dim; c += 256) out[i * dim + c] = queries[j * dim + c];
  if (zero_cnt && threadIdx.x == 0) cnt[j] = 0;
}

void launch_range_gather(const float* queries, int dim, const int32_t* qsel, int64_t m, float* out, u32* cnt, bool zero_cnt, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(range_gather_kernel, dim3((unsigned)m), dim3(256), 0, s, queries, dim, qsel, out, cnt, zero_cnt ? 1 : 0);
}

}  // namespace eps
