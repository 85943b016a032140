// Multi-vector search (eps_index_search_multi): a query is a bag of vectors, a group scores by the sum over the bag's vectors of the distance to its
// closest visible row - the late-interaction score (negated MaxSim under DOT_PRODUCT, a one-sided Chamfer distance under L2) - and the call returns
// the k groups with the smallest sums.  The reference has no such call (see groups.hip).  The rule is in include/epsilla_gfx950.h.
//
// Two forms, the same bits (plan and limits: multi_host.hpp; the host loops: Index::search_multi).  Both fill a table of minimum keys per (vector,
// group), KEY_EMPTY where the group has no visible row for the vector, and share what reads it:
//  * multi_sum_topk_kernel, per bag W wavefronts with a slice of the table's columns each, one lane per column: the lane walks the bag's t rows
//    of the table, drops its column at the first KEY_EMPTY, adds key_dist in bag order - s = s + d from +0.0f, nothing reassociated - and offers
//    make_key(s, label) to a WaveTopK; launch_among_merge makes the bag's sorted list of them.
//  * multi_finalize_kernel, one wavefront per (bag, slot): group key, score, count, padding, and the matches read back from the table.
// Whole table: the vectors of as many whole bags as fit are the m pseudo-queries of launch_groups_min_scan, as it stands; the columns are the G
// labels (stride G between a bag's rows, 1 between columns).  HBM traffic: n * dim * 4 + n * 4 bytes per 4 vectors, 8 * t * G per bag to read back.
// Candidates: the caller names group keys.  multi_labels_kernel finds each key's label by binary search (-1: none); multi_worklist_kernel, one
// workgroup, writes per (bag, candidate) pair the exclusive prefix of its ceil(size / 256) * ceil(t / 4) work items - the host never reads it;
// multi_gather_kernel, a fixed grid of one-wavefront workgroups striding over the items: an item finds its (pair, chunk, quad of vectors) by binary
// search, stages its <= 4 vectors in LDS, walks its <= 256 rows through the rows by group with the flat scan's sums (row_dists at NQ = 4), keeps
// per vector the smallest visible key, reduces over the wavefront and issues ONE atomicMin per (item, vector) into pair_best[pair][t] - a hot group
// named by many bags meets at different addresses, and a large one arrives as one atomic per 256 rows.  The columns are then a bag's candidates
// (stride 1 between a bag's rows, t between columns); a candidate named twice gives the same key twice and among_merge keeps one.  Traffic: the
// rows of the candidate groups once per 4 vectors per bag that names them.
// No workgroup waits on another.
#include "kernels.hpp"

namespace eps {

__device__ __forceinline__ int64_t multi_cand_begin(const MultiArgs& a, int64_t j) { return a.cand_off ? a.cand_off[j] : 0; }
__device__ __forceinline__ int64_t multi_cand_count(const MultiArgs& a, int64_t j) { return a.cand_off ? a.cand_off[j + 1] - a.cand_off[j] : a.n_cand; }

// pair p of the pass -> its bag j, the candidate's place c in the bag's list and its place ci in cand_label
__device__ __forceinline__ void multi_pair(const MultiArgs& a, int64_t p, int64_t* j, int64_t* c, int64_t* ci) {
  if (!a.cand_off) {   // one list for every bag
    *j = a.j0 + p / a.n_cand;
    *c = *ci = p % a.n_cand;
    return;
  }
  const int64_t gp = a.cand_off[a.j0] + p;
  int64_t lo = a.j0, hi = a.j0 + a.bags;   // cand_off[lo] <= gp < cand_off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.cand_off[mid] <= gp) lo = mid; else hi = mid;
  }
  *j = lo;   // (the last bag whose list starts at or before the pair: the one that holds it)
  *c = gp - a.cand_off[lo];
  *ci = gp;
}

// ------------------------------------------------------------------------------------------------ the candidates' labels
__global__ void multi_labels_kernel(const int64_t* cand_keys, int64_t n_cand, const int64_t* key_of_label, int64_t G, int32_t* cand_label) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cand) return;
  const int64_t key = cand_keys[i];
  int64_t lo = 0, hi = G;   // the first label whose key is >= key
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key_of_label[mid] < key) lo = mid + 1; else hi = mid;
  }
  cand_label[i] = (lo < G && key_of_label[lo] == key) ? (int32_t)lo : -1;
}

void launch_multi_labels(const int64_t* cand_keys, int64_t n_cand, const int64_t* key_of_label, int64_t G, int32_t* cand_label, hipStream_t s) {
  if (n_cand <= 0) return;
  hipLaunchKernelGGL(multi_labels_kernel, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, s, cand_keys, n_cand, key_of_label, G, cand_label);
}

// ------------------------------------------------------------------------------------------------ the work list
// exclusive prefix of v over the workgroup's 256 threads, *total = their sum (block-uniform); wave_sum: 4 words of LDS
__device__ __forceinline__ unsigned long long multi_block_scan(unsigned long long v, unsigned long long* wave_sum, unsigned long long* total) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = shfl_up64(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? wave_sum[w] : 0ull;
    all += wave_sum[w];
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(256) void multi_worklist_kernel(MultiArgs a) {
  __shared__ unsigned long long wave_sum[4];
  unsigned long long base = 0;
  for (int64_t p0 = 0; p0 < a.pairs; p0 += 256) {
    const int64_t p = p0 + threadIdx.x;
    unsigned long long items = 0;
    if (p < a.pairs) {
      int64_t j, c, ci;
      multi_pair(a, p, &j, &c, &ci);
      const int lab = a.cand_label[ci];
      if (lab >= 0) items = (unsigned long long)multi_pair_items(a.offsets[lab + 1] - a.offsets[lab], a.q_off[j + 1] - a.q_off[j]);
    }
    unsigned long long total;
    const unsigned long long before = multi_block_scan(items, wave_sum, &total);
    if (p < a.pairs) a.prefix[p] = base + before;
    base += total;
  }
  if (threadIdx.x == 0) a.prefix[a.pairs] = base;
}

// ------------------------------------------------------------------------------------------------ the gather
template <bool VEC4, int U>
__global__ __launch_bounds__(64) void multi_gather_kernel(MultiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NQ = MULTI_QUAD;
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  const int lane = lane_id();
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int tl = lane & (G - 1);
  const int64_t total = (int64_t)a.prefix[a.pairs];

  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    int64_t lo = 0, hi = a.pairs;   // prefix[lo] <= item < prefix[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.prefix[mid] <= item) lo = mid; else hi = mid;
    }
    int64_t j, c, ci;   // (the last pair that starts at or before the item: it has items, so a label and vectors)
    multi_pair(a, lo, &j, &c, &ci);
    const int64_t v_first = a.q_off[j];
    const int64_t t = a.q_off[j + 1] - v_first;
    const int64_t quads = (t + NQ - 1) / NQ;
    const int64_t r = item - (int64_t)a.prefix[lo];
    const int64_t chunk = r / quads;
    const int64_t v0 = (r - chunk * quads) * NQ;   // the quad's first vector (< t)
    const int nv = t - v0 < NQ ? (int)(t - v0) : NQ;
    __syncthreads();   // (one wavefront: the previous item's reads of its vectors are done)
    for (int i = lane; i < NQ * qstride; i += 64) {
      const int q = i / qstride, col = i - q * qstride;
      const int64_t v = v_first + v0 + (q < nv ? q : nv - 1);   // (beyond the bag's end: its last vector again, the sums unused)
      smem[i] = col < dim ? a.vectors[v * dim + col] : 0.f;
    }
    __syncthreads();
    const int lab = a.cand_label[ci];
    const int64_t last = a.offsets[lab + 1];
    const int64_t begin = a.offsets[lab] + chunk * MULTI_CHUNK;   // (< last: the item is one of the group's chunks)
    const int64_t end = last - begin < MULTI_CHUNK ? last : begin + MULTI_CHUNK;

    u64 mn[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) mn[q] = KEY_EMPTY;
    for (int64_t r0 = begin; r0 < end; r0 += RPW * U) {
      const float* rp[U];
      u32 row[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t ri = r0 + u * RPW + g;
        ok[u] = ri < end;
        row[u] = (u32)a.group_rows[ok[u] ? ri : end - 1];
        rp[u] = a.rows + (int64_t)row[u] * dim;
      }
      float acc[U][NQ];
      row_dists<U, NQ, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const u64 key = make_key(finish_dist(a.metric, acc[u][q]), row[u]);
          // (a key at or above the lane's minimum cannot lower it: its verdict is not needed)
          if (tl == 0 && ok[u] && q < nv && key < mn[q] && row_visible(a.f, row[u], key_dist(key))) mn[q] = key;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const u64 other = shfl64(mn[q], lane ^ o);
        mn[q] = other < mn[q] ? other : mn[q];
      }
    }
    if (lane == 0) {
      u64* slot = a.table + (a.base_off[j] - a.base_off[a.j0]) + c * t + v0;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (q < nv && mn[q] < slot[q]) atomicMin(&slot[q], mn[q]);   // (the slot only decreases: a stale read costs an atomic, never a result)
      atomicAdd(a.evals, (unsigned long long)((end - begin) * nv));
    }
  }
}

void launch_multi_gather(const MultiArgs& a, hipStream_t s) {
  if (a.pairs <= 0) return;
  hipLaunchKernelGGL(multi_worklist_kernel, dim3(1), dim3(256), 0, s, a);
  const size_t shm = (size_t)MULTI_QUAD * ((a.dim + 3) & ~3) * sizeof(float);
  const dim3 grid((unsigned)a.waves);
  if (rows_vec4(a.rows, a.dim))
    hipLaunchKernelGGL((multi_gather_kernel<true, 4>), grid, dim3(64), shm, s, a);
  else
    hipLaunchKernelGGL((multi_gather_kernel<false, 4>), grid, dim3(64), shm, s, a);
}

// ------------------------------------------------------------------------------------------------ sums and their top-k
// Wavefront w of the pass's bag i: columns [w * slice, (w + 1) * slice) of the bag's part of the table, the k smallest sums into partial[i][w][k]
template <int KPL, bool CAND>
__global__ __launch_bounds__(256) void multi_sum_topk_kernel(MultiArgs a) {
  const int64_t i = blockIdx.y;
  const int64_t j = a.j0 + i;
  const int lane = lane_id();
  const int64_t w = (int64_t)blockIdx.x * GROUPS_BLOCK_WAVES + (threadIdx.x >> 6);
  const int64_t t = a.q_off[j + 1] - a.q_off[j];
  const int64_t cols = t > 0 ? (CAND ? multi_cand_count(a, j) : a.G) : 0;   // (an empty bag: no group qualifies)
  const int64_t cand0 = CAND ? multi_cand_begin(a, j) : 0;
  const int64_t su = CAND ? 1 : a.G, sx = CAND ? t : 1;
  const u64* tab = a.table + (a.base_off[j] - a.base_off[a.j0]) * (CAND ? 1 : a.G);
  const int64_t begin = w * a.plan.slice < cols ? w * a.plan.slice : cols;
  const int64_t end = cols - begin < a.plan.slice ? cols : begin + a.plan.slice;
  WaveTopK<KPL> L[1];
  u64 thr[1];
  L[0].init();
  thr[0] = KEY_EMPTY;
  const FilterSpec nof = no_filter();   // (the table holds visible rows only)
  for (int64_t x0 = begin; x0 < end; x0 += 64) {
    const int64_t x = x0 + lane;
    int lab = -1;
    if (x < end) lab = CAND ? a.cand_label[cand0 + x] : (int)x;
    bool ok = lab >= 0;
    float s = 0.0f;
    for (int64_t u = 0; u < t && ok; ++u) {
      const u64 key = tab[u * su + x * sx];
      ok = key != KEY_EMPTY;          // (no visible row for this vector: the group does not qualify)
      if (ok) s = s + key_dist(key);  // in bag order, one add after the other
    }
    offer<1, KPL>(L, thr, 0, make_key(s, (u32)lab), ok, nof, a.k, CAND);   // (CAND: a candidate named twice offers one key twice)
  }
  L[0].store(a.partial + (i * a.plan.W + w) * a.k, a.k);
}

void launch_multi_sum_topk(const MultiArgs& a, hipStream_t s) {
  if (a.bags <= 0) return;
  const int kpl = pick_kpl(a.k);
  const dim3 grid((unsigned)(a.plan.W / GROUPS_BLOCK_WAVES), (unsigned)a.bags);
  const bool cand = a.cand_label != nullptr;
#define EPS_CASE(KPL_)                                                                                   \
  if (kpl == KPL_) {                                                                                     \
    if (cand)                                                                                            \
      hipLaunchKernelGGL((multi_sum_topk_kernel<KPL_, true>), grid, dim3(256), 0, s, a);                 \
    else                                                                                                 \
      hipLaunchKernelGGL((multi_sum_topk_kernel<KPL_, false>), grid, dim3(256), 0, s, a);                \
    return;                                                                                              \
  }
  EPS_CASE(1) EPS_CASE(2) EPS_CASE(4) EPS_CASE(8) EPS_CASE(16)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------ the answer
// One wavefront per (bag, slot) of the pass
__global__ __launch_bounds__(64) void multi_finalize_kernel(MultiArgs a, const int64_t* key_of_label, int64_t id_base, int64_t id_stride, int64_t* group_keys,
                                                            float* score, int32_t* counts, int64_t* match_ids, float* match_dist) {
  const int lane = lane_id();
  const int64_t i = blockIdx.x / a.k;
  const int s = (int)(blockIdx.x - i * a.k);
  const int64_t j = a.j0 + i;
  const u64 key = a.run_keys[blockIdx.x];
  const bool valid = key != KEY_EMPTY;
  const int lab = (int)key_id(key);
  if (lane == 0) {
    group_keys[j * a.k + s] = valid ? key_of_label[lab] : 0;
    score[j * a.k + s] = valid ? key_dist(key) : __builtin_inff();
    if (counts) {   // (sorted: the empty slots are behind the keys)
      if (s == 0 && !valid) counts[j] = 0;
      if (valid && (s == a.k - 1 || a.run_keys[blockIdx.x + 1] == KEY_EMPTY)) counts[j] = s + 1;
    }
  }
  if (!match_ids) return;
  const bool cand = a.cand_label != nullptr;
  const int64_t v_first = a.q_off[j];
  const int64_t t = a.q_off[j + 1] - v_first;
  int64_t x = lab;   // the group's column of the table
  if (valid && cand) {   // the first candidate of the bag that names the group (every one of them holds the same keys)
    const int64_t cand0 = multi_cand_begin(a, j), nc = multi_cand_count(a, j);
    x = 0;
    for (int64_t c0 = 0; c0 < nc; c0 += 64) {
      const int64_t c = c0 + lane;
      const u64 hit = __ballot(c < nc && a.cand_label[cand0 + c] == lab);
      if (hit) {
        x = c0 + (__ffsll((long long)hit) - 1);
        break;
      }
    }
  }
  const int64_t su = cand ? 1 : a.G, sx = cand ? t : 1;
  const u64* tab = a.table + (a.base_off[j] - a.base_off[a.j0]) * (cand ? 1 : a.G);
  const int64_t out = (int64_t)a.k * v_first + (int64_t)s * t;
  for (int64_t u = lane; u < t; u += 64) {
    const u64 b = valid ? tab[u * su + x * sx] : KEY_EMPTY;   // (a slot in use: every vector of the bag has its key)
    match_ids[out + u] = valid ? (int64_t)key_id(b) * id_stride + id_base : -1;
    match_dist[out + u] = valid ? key_dist(b) : __builtin_inff();
  }
}

void launch_multi_finalize(const MultiArgs& a, const int64_t* key_of_label, int64_t id_base, int64_t id_stride, int64_t* group_keys, float* score,
                           int32_t* counts, int64_t* match_ids, float* match_dist, hipStream_t s) {
  const int64_t total = a.bags * a.k;
  if (total <= 0) return;
  hipLaunchKernelGGL(multi_finalize_kernel, dim3((unsigned)total), dim3(64), 0, s, a, key_of_label, id_base, id_stride, group_keys, score, counts, match_ids,
                     match_dist);
}

}  // namespace eps
