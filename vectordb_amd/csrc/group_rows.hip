// Grouped search, m rows per group (eps_index_search_group_rows): per query the k closest groups as eps_index_search_groups finds them, and of each
// its m closest visible rows and the number of its visible rows.  The reference has no such call (see groups.hip).
//
// Set-up, once per set_groups and only when this call is used: the rows of every label next to each other - group_rows_hist_kernel counts the
// rows per label (atomicAdd), group_rows_offsets_kernel scans the counts in one workgroup, group_rows_scatter_kernel places every row through
// its label's cursor.  The order inside a group depends on the schedule; nothing below depends on it: a top-m by key does not depend on the order
// of its offers.
// The call, after the first phase has left up to k representative keys per query on the device (plan: group_rows_host.hpp):
//  * group_rows_worklist_kernel, one workgroup: per (query, slot) pair the chunks of its group, ceil(size / chunk), as an exclusive prefix with
//    the total behind it.  The host never reads it: the call has no sync of its own.
//  * group_rows_gather_kernel, a fixed grid of one-wavefront workgroups striding over the work items: an item finds its (pair, chunk) by binary
//    search in the prefix, stages its query in LDS and walks its <= chunk rows with among_gather_kernel's blocking at NQ = 1 - G lanes per row, U
//    rows in flight, row_dists and its lane tree, so the sums are the flat scan's bit for bit - into a WaveTopK of m keys, stored as the item's
//    partial list.  Every row gets its verdict (row_visible, the function offer calls): the item adds the number of its visible rows to the pair's
//    counter with an integer atomicAdd, and only visible rows are offered.  A group larger than a chunk is spread over many wavefronts.
//  * group_rows_merge_kernel, one workgroup per pair: its partial lists into run_keys[pair][m] (among_merge_kernel's scheme).
//  * group_rows_finalize_kernel: ids through the id map, distances, row counts, sizes, the queries' group counts and the padding.
// HBM traffic of the gather: rows gathered * dim * 4 bytes, 4 bytes of row number per row, dim * 4 bytes of query per item (from L2 mostly).
// No workgroup waits on another.
#include "kernels.hpp"

namespace eps {

// exclusive prefix of v over the workgroup's 256 threads, *total = their sum (block-uniform); wave_sum: 4 words of LDS
__device__ __forceinline__ u32 group_rows_block_scan(u32 v, u32* wave_sum, u32* total) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  u32 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  u32 before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? wave_sum[w] : 0u;
    all += wave_sum[w];
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

// ------------------------------------------------------------------------------------------------ rows by group
__global__ void group_rows_hist_kernel(const int32_t* label, int64_t n, u32* cursor) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&cursor[label[i]], 1u);
}

// offsets[g] = rows of the labels below g, offsets[G] = n; cursor[g]: the count on entry, offsets[g] on exit (n < 2^31)
__global__ __launch_bounds__(256) void group_rows_offsets_kernel(u32* cursor, int64_t G, int64_t* offsets) {
  __shared__ u32 wave_sum[4];
  u32 base = 0;
  for (int64_t g0 = 0; g0 < G; g0 += 256) {
    const int64_t g = g0 + threadIdx.x;
    u32 total;
    const u32 before = group_rows_block_scan(g < G ? cursor[g] : 0u, wave_sum, &total);
    if (g < G) {
      offsets[g] = (int64_t)(base + before);
      cursor[g] = base + before;
    }
    base += total;
  }
  if (threadIdx.x == 0) offsets[G] = (int64_t)base;
}

__global__ void group_rows_scatter_kernel(const int32_t* label, int64_t n, u32* cursor, int32_t* group_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) group_rows[atomicAdd(&cursor[label[i]], 1u)] = (int32_t)i;
}

void launch_group_rows_build(const int32_t* label, int64_t n, int64_t G, u32* cursor, int64_t* offsets, int32_t* group_rows, hipStream_t s) {
  if (n <= 0 || G <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(group_rows_hist_kernel, grid, dim3(256), 0, s, label, n, cursor);
  hipLaunchKernelGGL(group_rows_offsets_kernel, dim3(1), dim3(256), 0, s, cursor, G, offsets);
  hipLaunchKernelGGL(group_rows_scatter_kernel, grid, dim3(256), 0, s, label, n, cursor, group_rows);
}

// ------------------------------------------------------------------------------------------------ the work list
__global__ __launch_bounds__(256) void group_rows_worklist_kernel(GroupRowsArgs a) {
  __shared__ u32 wave_sum[4];
  u32 base = 0;
  for (int64_t p0 = 0; p0 < a.pairs; p0 += 256) {
    const int64_t p = p0 + threadIdx.x;
    u32 chunks = 0;
    if (p < a.pairs) {
      const u64 key = a.res_keys[p];
      if (key != KEY_EMPTY) {
        const int lab = a.label[key_id(key)];
        chunks = (u32)((a.offsets[lab + 1] - a.offsets[lab] + a.chunk - 1) / a.chunk);
      }
    }
    u32 total;
    const u32 before = group_rows_block_scan(chunks, wave_sum, &total);
    if (p < a.pairs) a.prefix[p] = base + before;
    base += total;
  }
  if (threadIdx.x == 0) a.prefix[a.pairs] = base;
}

// ------------------------------------------------------------------------------------------------ the gather
template <int KPL, bool VEC4, int U>
__global__ __launch_bounds__(64) void group_rows_gather_kernel(GroupRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  const int lane = lane_id();
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const FilterSpec nof = no_filter();   // (every row is judged below, before it is offered)
  int64_t total = a.prefix[a.pairs];
  total = total < a.items ? total : a.items;   // (the plan's bound holds: the partial lists end there)

  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    int64_t lo = 0, hi = a.pairs;   // prefix[lo] <= item < prefix[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.prefix[mid] <= item) lo = mid; else hi = mid;
    }
    const int64_t pair = lo;   // (the last pair that starts at or before the item: it has chunks)
    const int64_t q = pair / a.k;
    __syncthreads();   // (one wavefront: the previous item's reads of the query are done)
    for (int i = lane; i < qstride; i += 64) smem[i] = i < dim ? a.queries[q * dim + i] : 0.f;
    __syncthreads();
    const int lab = a.label[key_id(a.res_keys[pair])];
    const int64_t last = a.offsets[lab + 1];
    const int64_t begin = a.offsets[lab] + (item - (int64_t)a.prefix[pair]) * a.chunk;   // (< last: the item is one of the group's chunks)
    const int64_t end = last - begin < a.chunk ? last : begin + a.chunk;

    WaveTopK<KPL> list[1];
    u64 thr[1];
    list[0].init();
    thr[0] = KEY_EMPTY;
    u32 seen = 0;   // visible rows of this chunk

    for (int64_t r0 = begin; r0 < end; r0 += RPW * U) {
      const float* rp[U];
      u32 row[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t ci = r0 + u * RPW + g;
        ok[u] = ci < end;
        row[u] = (u32)a.group_rows[ok[u] ? ci : end - 1];
        rp[u] = a.rows + (int64_t)row[u] * dim;
      }
      float acc[U][1];
      row_dists<U, 1, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u64 key = make_key(finish_dist(a.metric, acc[u][0]), row[u]);
        const bool vis = (t == 0) && ok[u] && row_visible(a.f, row[u], key_dist(key));
        seen += (u32)__popcll(__ballot(vis));
        offer<1, KPL>(list, thr, 0, key, vis, nof, a.m, false);
      }
    }
    list[0].store(a.partial + item * a.m, a.m);
    if (lane == 0) {
      if (seen) atomicAdd(&a.sizes[pair], seen);
      atomicAdd(a.evals, (unsigned long long)(end - begin));
    }
  }
}

// One workgroup per pair: its partial lists (consecutive work items) into run_keys[pair][m].  A pair without a group: an empty list
template <int KPL>
__global__ __launch_bounds__(256) void group_rows_merge_kernel(GroupRowsArgs a) {
  __shared__ u64 sh[4][KPL * 64];
  const int64_t pair = blockIdx.x;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  int64_t first = a.prefix[pair], behind = a.prefix[pair + 1];
  first = first < a.items ? first : a.items;
  behind = behind < a.items ? behind : a.items;
  const u64* src = a.partial + first * a.m;
  const int slots = (int)((behind - first) * a.m);   // (<= GROUPS_MERGE_KEYS + m by the plan's chunk)
  WaveTopK<KPL> L[1];
  u64 thr[1];
  L[0].init();
  thr[0] = KEY_EMPTY;
  const FilterSpec nof = no_filter();
  const int rounded = (slots + 255) / 256 * 256;
  for (int i = threadIdx.x; i < rounded; i += 256) {
    const u64 key = i < slots ? src[i] : KEY_EMPTY;
    offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, a.m, true);
  }
  L[0].store(&sh[wave][0], a.m);
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < 4; ++w) {
    for (int e0 = 0; e0 < a.m; e0 += 64) {
      const int e = e0 + lane;
      const u64 key = e < a.m ? sh[w][e] : KEY_EMPTY;
      offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, a.m, true);
    }
  }
  L[0].store(a.run_keys + pair * a.m, a.m);
}

void launch_group_rows_gather(const GroupRowsArgs& a, hipStream_t s) {
  if (a.pairs <= 0) return;
  hipLaunchKernelGGL(group_rows_worklist_kernel, dim3(1), dim3(256), 0, s, a);
  const size_t shm = (size_t)((a.dim + 3) & ~3) * sizeof(float);
  const bool vec4 = rows_vec4(a.rows, a.dim);
  const int kpl = pick_kpl(a.m);
  const dim3 grid((unsigned)a.waves);
#define EPS_CASE(KPL_)                                                                                      \
  if (kpl == KPL_) {                                                                                        \
    if (vec4)                                                                                               \
      hipLaunchKernelGGL((group_rows_gather_kernel<KPL_, true, 4>), grid, dim3(64), shm, s, a);             \
    else                                                                                                    \
      hipLaunchKernelGGL((group_rows_gather_kernel<KPL_, false, 4>), grid, dim3(64), shm, s, a);            \
  }
  EPS_CASE(1) EPS_CASE(2) EPS_CASE(4) EPS_CASE(8) EPS_CASE(16)
#undef EPS_CASE
}

void launch_group_rows_merge(const GroupRowsArgs& a, hipStream_t s) {
  if (a.pairs <= 0) return;
  const int kpl = pick_kpl(a.m);
#define EPS_CASE(KPL_) \
  if (kpl == KPL_) hipLaunchKernelGGL((group_rows_merge_kernel<KPL_>), dim3((unsigned)a.pairs), dim3(256), 0, s, a);
  EPS_CASE(1) EPS_CASE(2) EPS_CASE(4) EPS_CASE(8) EPS_CASE(16)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------ the answer
__global__ void group_rows_finalize_kernel(GroupRowsArgs a, int64_t id_base, int64_t id_stride, int64_t* ids, float* dist, int32_t* row_counts,
                                           int64_t* group_sizes, int32_t* counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.pairs * a.m) return;
  const u64 key = a.run_keys[i];
  const bool valid = key != KEY_EMPTY;
  ids[i] = valid ? (int64_t)key_id(key) * id_stride + id_base : -1;
  dist[i] = valid ? key_dist(key) : __builtin_inff();
  if (i % a.m) return;
  const int64_t pair = i / a.m;
  int c = 0;
  while (c < a.m && a.run_keys[i + c] != KEY_EMPTY) ++c;   // (sorted: the empty slots are behind the keys)
  row_counts[pair] = c;
  if (group_sizes) group_sizes[pair] = (int64_t)a.sizes[pair];
  if (counts && pair % a.k == 0) {
    int gc = 0;
    while (gc < a.k && a.res_keys[pair + gc] != KEY_EMPTY) ++gc;
    counts[pair / a.k] = gc;
  }
}

void launch_group_rows_finalize(const GroupRowsArgs& a, int64_t id_base, int64_t id_stride, int64_t* ids, float* dist, int32_t* row_counts,
                                int64_t* group_sizes, int32_t* counts, hipStream_t s) {
  const int64_t total = a.pairs * a.m;
  if (total <= 0) return;
  hipLaunchKernelGGL(group_rows_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, id_base, id_stride, ids, dist, row_counts,
                     group_sizes, counts);
}

}  // namespace eps
