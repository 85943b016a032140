// Grouped search (eps_index_search_groups): per query the k closest GROUPS of rows, each by its closest visible row.  The reference groups answers
// by an attribute on the host, after the search (FacetExecutor, engine/db/execution/aggregation.hpp); it has no call that searches by group.
//
// Two engines, the same bits (plan and limits: groups_host.hpp; the host loops: Index::search_groups).
//  * Pages.  The table's keys in ascending order, a page at a time (the flat engines, then flat_stream_page's continuation).  groups_first_kernel,
//    one workgroup per query, keeps a page entry iff it is the first of its label - in the page, and among the representatives of earlier pages: an
//    LDS open-addressing table claimed by label (atomicCAS) holds the smallest position per label (atomicMin), the carried representatives seeded
//    at position -1.  The kept entries are appended in order (ballot + mbcnt rank, as select.hip scatters), so the result stays sorted.
//  * Scan.  groups_min_scan_kernel has flat_scan_kernel's blocking - 4 queries staged in LDS, a chunk of rows per wavefront, G lanes per row,
//    row_dists and its lane tree, so the sums are the flat scan's bit for bit - but keeps no list: a visible row offers make_key(dist, row) to
//    best[query][label[row]] with a 64-bit atomicMin.  The minimum of a set does not depend on the order of its offers.  A plain load of the slot
//    goes first: the slot only decreases, so a stale value costs an atomic, never a result.  groups_table_topk_kernel then reads the G slots back,
//    a contiguous slice per wavefront into a WaveTopK list; launch_among_merge and launch_finalize do the rest.
// HBM traffic of the scan: n * dim * 4 bytes of rows and n * 4 of labels per 4 queries, 16 * G bytes per query of table fill and read-back.
// No workgroup waits on another.
#include "kernels.hpp"

namespace eps {

// ------------------------------------------------------------------------------------------------ pages
// the slot of `lab` (claimed if it has none yet), its position lowered to `pos`.  At most 2048 labels meet in 4096 slots: the probe ends
__device__ __forceinline__ int groups_claim(int* t_label, int* t_pos, int lab, int pos) {
  int h = lab & (GROUPS_LDS_SLOTS - 1);
  for (;;) {
    const int old = atomicCAS(&t_label[h], -1, lab);
    if (old == -1 || old == lab) break;
    h = (h + 1) & (GROUPS_LDS_SLOTS - 1);
  }
  atomicMin(&t_pos[h], pos);
  return h;
}

__global__ __launch_bounds__(256) void groups_first_kernel(GroupsFirstArgs a) {
  __shared__ int t_label[GROUPS_LDS_SLOTS];
  __shared__ int t_pos[GROUPS_LDS_SLOTS];
  __shared__ u32 wave_cnt[4];
  constexpr int PER = GROUPS_MAX_PAGE / 256;   // page entries per thread
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = tid >> 6;
  const int64_t i = blockIdx.x;
  const int64_t q = a.qsel ? a.qsel[i] : i;
  const u64* page = a.page + i * a.P;
  u64* res = a.res_keys + q * a.k;
  const u32 have = a.res_cnt[q];   // (< k: a query that holds k representatives is finished)

  for (int s = tid; s < GROUPS_LDS_SLOTS; s += 256) {
    t_label[s] = -1;
    t_pos[s] = 0x7FFFFFFF;
  }
  __syncthreads();
  for (u32 e = tid; e < have; e += 256) groups_claim(t_label, t_pos, a.label[key_id(res[e])], -1);   // the labels earlier rounds have answered
  __syncthreads();
  u64 key[PER];
  int slot[PER];
#pragma unroll
  for (int c = 0; c < PER; ++c) {
    const int e = c * 256 + tid;
    key[c] = e < a.P ? page[e] : KEY_EMPTY;
    slot[c] = key[c] != KEY_EMPTY ? groups_claim(t_label, t_pos, a.label[key_id(key[c])], e) : -1;
  }
  __syncthreads();
  u32 base = have;   // (block-uniform)
#pragma unroll
  for (int c = 0; c < PER; ++c) {
    const int e = c * 256 + tid;
    const bool keep = slot[c] >= 0 && t_pos[slot[c]] == e;
    const u64 m = __ballot(keep);
    const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
    if (lane == 0) wave_cnt[wave] = (u32)__popcll(m);
    __syncthreads();
    u32 before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wave_cnt[w] : 0u;
      total += wave_cnt[w];
    }
    const u32 dst = base + before + rank;
    if (keep && dst < (u32)a.k) res[dst] = key[c];
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    const u64 last = page[a.P - 1];
    const u32 cnt = base < (u32)a.k ? base : (u32)a.k;
    a.res_cnt[q] = cnt;
    a.status[q] = (cnt < (u32)a.k && last != KEY_EMPTY) ? GROUPS_UNFINISHED : 0u;   // a short page: the table has no further key
    a.lo[q] = last;
  }
}

void launch_groups_first(const GroupsFirstArgs& a, hipStream_t s) {
  if (a.m <= 0) return;
  hipLaunchKernelGGL(groups_first_kernel, dim3((unsigned)a.m), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(256) void groups_compact_kernel(const u32* status, int64_t nq, int32_t* qsel, u32* m_out) {
  __shared__ u32 wave_cnt[4];
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = tid >> 6;
  u32 base = 0;
  for (int64_t i0 = 0; i0 < nq; i0 += 256) {
    const int64_t i = i0 + tid;
    const bool un = i < nq && status[i] == GROUPS_UNFINISHED;
    const u64 m = __ballot(un);
    const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
    if (lane == 0) wave_cnt[wave] = (u32)__popcll(m);
    __syncthreads();
    u32 before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wave_cnt[w] : 0u;
      total += wave_cnt[w];
    }
    if (un) qsel[base + before + rank] = (int32_t)i;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    *m_out = base;
    __threadfence_system();
  }
}

void launch_groups_compact(const u32* status, int64_t nq, int32_t* qsel, u32* m_out, hipStream_t s) {
  hipLaunchKernelGGL(groups_compact_kernel, dim3(1), dim3(256), 0, s, status, nq, qsel, m_out);
}

__global__ __launch_bounds__(256) void groups_gather_kernel(const float* queries, int dim, const u64* lo, const int32_t* qsel, float* q_out, u64* lo_out) {
  const int64_t i = blockIdx.x;
  const int64_t q = qsel[i];
  for (int c = threadIdx.x; c < dim; c += 256) q_out[i * dim + c] = queries[q * dim + c];
  if (threadIdx.x == 0) lo_out[i] = lo[q];
}

void launch_groups_gather(const float* queries, int dim, const u64* lo, const int32_t* qsel, int64_t m, float* q_out, u64* lo_out, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(groups_gather_kernel, dim3((unsigned)m), dim3(256), 0, s, queries, dim, lo, qsel, q_out, lo_out);
}

// ------------------------------------------------------------------------------------------------ scan
template <bool VEC4, int U>
__global__ __launch_bounds__(256) void groups_min_scan_kernel(GroupsScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NQ = GROUPS_SCAN_NQ;
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  const int64_t q0 = (int64_t)blockIdx.y * NQ;
  for (int i = threadIdx.x; i < NQ * qstride; i += 256) {
    const int q = i / qstride, c = i - q * qstride;
    const int64_t qq = (q0 + q < a.m) ? q0 + q : a.m - 1;
    const int64_t qn = a.qsel ? a.qsel[qq] : qq;
    smem[i] = c < dim ? a.queries[qn * dim + c] : 0.f;
  }
  __syncthreads();

  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const int64_t W = (int64_t)gridDim.x * GROUPS_BLOCK_WAVES;
  const int64_t w = (int64_t)blockIdx.x * GROUPS_BLOCK_WAVES + wave;
  const int64_t chunk = (a.n + W - 1) / W;
  const int64_t begin = w * chunk < a.n ? w * chunk : a.n;
  const int64_t end = a.n - begin < chunk ? a.n : begin + chunk;

  for (int64_t r0 = begin; r0 < end; r0 += RPW * U) {
    const float* rp[U];
    int64_t row[U];
    int lab[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      row[u] = r0 + u * RPW + g;
      const int64_t rc = row[u] < end ? row[u] : end - 1;
      rp[u] = a.rows + rc * dim;
      lab[u] = a.label[rc];
    }
    float acc[U][NQ];
    row_dists<U, NQ, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = (t == 0) && row[u] < end;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (valid && q0 + q < a.m) {
          const float dist = finish_dist(a.metric, acc[u][q]);
          const u64 key = make_key(dist, (u32)row[u]);
          u64* slot = a.best + (q0 + q) * a.G + lab[u];
          if (key < *slot && row_visible(a.f, (u32)row[u], key_dist(key))) atomicMin(slot, key);
        }
      }
    }
  }
}

void launch_groups_min_scan(const GroupsScanArgs& a, hipStream_t s) {
  if (a.m <= 0 || a.n <= 0) return;
  const dim3 grid((unsigned)(a.W / GROUPS_BLOCK_WAVES), (unsigned)((a.m + GROUPS_SCAN_NQ - 1) / GROUPS_SCAN_NQ));
  const size_t shm = (size_t)GROUPS_SCAN_NQ * ((a.dim + 3) & ~3) * sizeof(float);
  if (rows_vec4(a.rows, a.dim))
    hipLaunchKernelGGL((groups_min_scan_kernel<true, 4>), grid, dim3(256), shm, s, a);
  else
    hipLaunchKernelGGL((groups_min_scan_kernel<false, 4>), grid, dim3(256), shm, s, a);
}

// Wavefront w of query i: slots [w * slice, (w + 1) * slice) of the query's G, the k smallest of them into partial[i][w][k]
template <int KPL>
__global__ __launch_bounds__(256) void groups_table_topk_kernel(const u64* best, int64_t G, int k, int W, int64_t slice, u64* partial) {
  const int64_t i = blockIdx.y;
  const int lane = lane_id();
  const int64_t w = (int64_t)blockIdx.x * GROUPS_BLOCK_WAVES + (threadIdx.x >> 6);
  const int64_t begin = w * slice < G ? w * slice : G;
  const int64_t end = G - begin < slice ? G : begin + slice;
  const u64* src = best + i * G;
  WaveTopK<KPL> L[1];
  u64 thr[1];
  L[0].init();
  thr[0] = KEY_EMPTY;
  const FilterSpec nof = no_filter();   // (the scan judged every key it offered)
  for (int64_t s0 = begin; s0 < end; s0 += 64) {
    const int64_t sl = s0 + lane;
    const u64 key = sl < end ? src[sl] : KEY_EMPTY;
    offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, k, false);
  }
  L[0].store(partial + (i * W + w) * k, k);
}

void launch_groups_table_topk(const u64* best, int64_t G, int64_t m, int k, const GroupsScanPlan& plan, u64* partial, hipStream_t s) {
  if (m <= 0) return;
  const int kpl = pick_kpl(k);
  const dim3 grid((unsigned)(plan.W / GROUPS_BLOCK_WAVES), (unsigned)m);
#define EPS_CASE(KPL_)                                                                                                       \
  if (kpl == KPL_) {                                                                                                         \
    hipLaunchKernelGGL((groups_table_topk_kernel<KPL_>), grid, dim3(256), 0, s, best, G, k, plan.W, plan.slice, partial);   \
    return;                                                                                                                  \
  }
  EPS_CASE(1) EPS_CASE(2) EPS_CASE(4) EPS_CASE(8) EPS_CASE(16)
#undef EPS_CASE
}

__global__ __launch_bounds__(256) void groups_scatter_kernel(const u64* run_keys, int k, const int32_t* qsel, u64* res_keys) {
  const int64_t i = blockIdx.x;
  const int64_t q = qsel ? qsel[i] : i;
  for (int e = threadIdx.x; e < k; e += 256) res_keys[q * k + e] = run_keys[i * k + e];
}

void launch_groups_scatter(const u64* run_keys, int k, const int32_t* qsel, int64_t m, u64* res_keys, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(groups_scatter_kernel, dim3((unsigned)m), dim3(256), 0, s, run_keys, k, qsel, res_keys);
}

__global__ void groups_keys_kernel(const u64* res_keys, int64_t total, const int32_t* label, const int64_t* key_of_label, int64_t* group_keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const u64 key = res_keys[i];
  group_keys[i] = key != KEY_EMPTY ? key_of_label[label[key_id(key)]] : 0;
}

void launch_groups_keys(const u64* res_keys, int64_t nq, int k, const int32_t* label, const int64_t* key_of_label, int64_t* group_keys, hipStream_t s) {
  const int64_t total = nq * k;
  if (total <= 0) return;
  hipLaunchKernelGGL(groups_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, res_keys, total, label, key_of_label, group_keys);
}

}  // namespace eps
