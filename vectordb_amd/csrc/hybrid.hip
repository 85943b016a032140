// Hybrid search (eps_index_search_hybrid): the k rows with the smallest  (w_dense * d_dense) + (w_sparse * d_sparse)  over a dense table and a
// sparse table whose rows are the same records - an embedding next to a BM25 / SPLADE-style vector.  Both terms keep the bits their own searches
// return: d_dense is the flat scan's row_dists sum (device_common.hpp), d_sparse the term-at-a-time sum of sparse_inverted.hip with its epilogue
// statement for statement.  The score is two rounded multiplies and one rounded add; `#pragma clang fp contract(off)` stands at file scope and
// again in every kernel, because hipcc would otherwise fuse them (and the sparse products) into v_fma_f32.
//
// hybrid_tile_kernel is ONE pass over both tables: no [nq][n] array of sparse distances ever exists in HBM.  A workgroup stages NQ dense queries and
// the NQ sparse queries' (index, value) pairs in LDS once; each of its four wavefronts owns the rows sparse_wave_rows gives it and walks them in
// tiles of HYB_TILE_ROWS.  Per tile:
//   sparse  for each staged query the match and sum of sparse_inverted_kernel - 64 terms per round, one per lane, the lane binary-searching ITS
//           column's postings for the tile's rows (bounds from the directory only); the terms with postings are then taken in ascending index
//           order and the lanes stride over the postings into acc[q][row - t0], the wavefront's own LDS slice (rows of one column are distinct,
//           one wavefront's LDS operations complete in program order, a wavefront-scope fence stands between terms)
//   dense   the tile's rows through row_dists<4, NQ, VEC4> in the flat scan's geometry - G lanes per row, four rows in flight per group
//   finish  the first lane of each group reads the row's NQ sparse sums (and leaves 0.0f for the next tile), applies the sparse metric's epilogue
//           and finish_dist, forms the score and offers make_key(score, row) to the query's WaveTopK - only a key that would enter the list is
//           judged against the dense handle's standing state; the sparse handle's bitset is part of `valid`
// The per-wavefront lists go out as partial[q][w][k]; launch_among_merge joins them.  HBM traffic: n * dim * 4 bytes of rows per NQ queries, the
// postings of the queries' terms, a byte of bitset and (COSINE) four bytes of norm per row.
//
// hybrid_parts_kernel gives the nq * k winners their two terms again: d_dense by row_dists in the same geometry, d_sparse by the scan's sequential
// two-pointer merge over the winner's CSR row - the same additions in the same order as the term-at-a-time sum.
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace eps {

// first posting of [lo, hi) whose row is >= `row` (hi if none): every probe lies inside [lo, hi)
__device__ __forceinline__ int64_t hybrid_lower_bound(const SparsePosting* p, int64_t lo, int64_t hi, int64_t row) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)p[mid].row < row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the sparse metric's epilogue on a finished sum, as sparse_inverted_kernel has it
__device__ __forceinline__ float hybrid_sparse_finish(int sp_metric, float s, float v1_prod, float v2_prod) {
#pragma clang fp contract(off)
  if (sp_metric == 1) {
    const float pp = v1_prod * v2_prod;
    const float root = sqrtf(pp);
    const float quot = s / root;
    return 1.0f - quot;
  }
  return -s;
}

template <int NQ, int KPL, bool VEC4>
__global__ __launch_bounds__(256) void hybrid_tile_kernel(HybridArgs a, int64_t tile0) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float hyb_lds[];   // hybrid_host.hpp has the layout
  constexpr int U = 4;
  constexpr int T = HYB_TILE_ROWS;
  const int dim = a.dim;
  const int qstride = a.plan.qstride;
  const int qcap = (int)a.plan.rows.qcap;
  char* const lds = reinterpret_cast<char*>(hyb_lds);
  float* const dq = hyb_lds;
  int* const q_idx = reinterpret_cast<int*>(lds + a.plan.idx_offset);
  float* const q_val = reinterpret_cast<float*>(lds + a.plan.val_offset);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  float* const acc = reinterpret_cast<float*>(lds + a.plan.acc_offset) + wave * (NQ * T);
  const int64_t q0 = (tile0 + blockIdx.y) * NQ;
  const int sp_metric = a.sp_metric;

  // ---- the tile's queries, once per workgroup; every wavefront clears its own accumulators
  for (int i = threadIdx.x; i < NQ * qstride; i += 256) {
    const int q = i / qstride, c = i - q * qstride;
    const int64_t qq = (q0 + q < a.nq) ? q0 + q : a.nq - 1;
    dq[i] = c < dim ? a.queries[qq * dim + c] : 0.f;
  }
  int qlen[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const bool have = q0 + q < a.nq;
    const int64_t qb = have ? a.q_offsets[q0 + q] : 0;
    int64_t len = have ? a.q_offsets[q0 + q + 1] - qb : 0;
    len = len < qcap ? len : qcap;   // (the host refused a longer query)
    qlen[q] = (int)len;
    for (int i = threadIdx.x; i < qlen[q]; i += 256) {
      q_idx[q * qcap + i] = a.q_indices[qb + i];
      q_val[q * qcap + i] = a.q_values[qb + i];
    }
  }
  for (int i = lane; i < NQ * T; i += 64) acc[i] = 0.0f;
  __syncthreads();
  float v2_prod[NQ];   // the queries' squares in stored order (every lane takes the same sums: the reads are broadcasts)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    float sum = 0.0f;
    if (sp_metric == 1) {
      for (int i = 0; i < qlen[q]; ++i) {
        const float v = q_val[q * qcap + i];
        const float sq = v * v;
        sum = sum + sq;
      }
    }
    v2_prod[q] = sum;
  }

  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const int W = a.plan.rows.W;
  const int64_t w = (int64_t)blockIdx.x * HYB_BLOCK_WAVES + wave;
  int64_t row_begin, row_end;
  sparse_wave_rows(a.plan.rows, a.n, w, &row_begin, &row_end);
  const float wd = a.w_dense, ws = a.w_sparse;

  WaveTopK<KPL> list[NQ];
  u64 thr[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    list[q].init();
    thr[q] = KEY_EMPTY;
  }

  for (int64_t t0 = row_begin; t0 < row_end; t0 += T) {
    const int64_t t1 = row_end - t0 < T ? row_end : t0 + T;
    // ---- sparse: every staged query's terms into the tile's accumulators
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float* const accq = acc + q * T;
      for (int base = 0; base < qlen[q]; base += SPARSE_INV_TERMS) {
        const int term = base + lane;
        int64_t lo = 0, hi = 0;
        float qv = 0.0f;
        if (term < qlen[q]) {
          const int64_t c = q_idx[q * qcap + term];   // (validated: 0 <= c < the sparse table's dim, and the directory has dim + 1 entries)
          qv = q_val[q * qcap + term];
          const int64_t cb = a.col_offsets[c], ce = a.col_offsets[c + 1];
          lo = hybrid_lower_bound(a.postings, cb, ce, t0);
          hi = hybrid_lower_bound(a.postings, lo, ce, t1);
        }
        u64 m = __ballot(hi > lo);   // the terms that have postings in this tile, in ascending index order
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          const int64_t b = (int64_t)shfl64((u64)lo, l), e = (int64_t)shfl64((u64)hi, l);
          const float v = __shfl(qv, l);
          for (int64_t i = b + lane; i < e; i += 64) {
            const SparsePosting p = a.postings[i];
            const int slot = (int)((int64_t)p.row - t0);   // (t0 <= row < t1: the two searches above)
            const float pr = p.value * v;
            const float s = accq[slot];
            accq[slot] = s + pr;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the next term's lanes read what this term's lanes wrote)
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // ---- dense and finish: the tile's rows in the flat scan's geometry
    for (int64_t r0 = t0; r0 < t1; r0 += RPW * U) {
      const float* rp[U];
      int64_t row[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        row[u] = r0 + u * RPW + g;
        const int64_t rc = row[u] < t1 ? row[u] : t1 - 1;
        rp[u] = a.rows + rc * dim;
      }
      float dacc[U][NQ];
      row_dists<U, NQ, VEC4>(rp, dq, qstride, dim, a.metric, G, dacc);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool fin = (t == 0) && row[u] < t1;   // this lane finishes the row: it reads and clears the row's sums
        const int64_t rr = fin ? row[u] : t0;
        const int slot = (int)(rr - t0);
        bool valid = fin;
        if (fin && a.sp_deleted) valid = !((a.sp_deleted[rr >> 3] >> (rr & 7)) & 1);
        const float v1_prod = (fin && sp_metric == 1) ? a.norms[rr] : 0.0f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float s = 0.0f;
          if (fin) {
            s = acc[q * T + slot];
            acc[q * T + slot] = 0.0f;
          }
          const float ds = hybrid_sparse_finish(sp_metric, s, v1_prod, v2_prod[q]);
          const float dd = finish_dist(a.metric, dacc[u][q]);
          const float pd = wd * dd;
          const float ps = ws * ds;
          const float score = pd + ps;
          const u64 key = make_key(score, (u32)rr);
          offer<NQ, KPL>(list, thr, q, key, valid && q0 + q < a.nq, a.f, a.k, false);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the next tile's sums start from the zeros written here)
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q0 + q < a.nq) list[q].store(a.partial + ((q0 + q) * W + w) * a.k, a.k);   // (a wavefront beyond the table: an empty list)
}

template <int NQ, int KPL>
static void launch_hybrid_tiles_t(const HybridArgs& a, bool vec4, hipStream_t s) {
  const SparsePlan& r = a.plan.rows;
  for (int64_t tile0 = 0; tile0 < r.tiles; tile0 += HYB_GRID_Y) {
    const int64_t gy = r.tiles - tile0 < HYB_GRID_Y ? r.tiles - tile0 : HYB_GRID_Y;
    const dim3 grid((unsigned)(r.W / HYB_BLOCK_WAVES), (unsigned)gy);
    if (vec4)
      hipLaunchKernelGGL((hybrid_tile_kernel<NQ, KPL, true>), grid, dim3(256), (size_t)r.lds_dynamic, s, a, tile0);
    else
      hipLaunchKernelGGL((hybrid_tile_kernel<NQ, KPL, false>), grid, dim3(256), (size_t)r.lds_dynamic, s, a, tile0);
  }
}

void launch_hybrid_tiles(const HybridArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
  const bool vec4 = rows_vec4(a.rows, a.dim);
  const int kpl = pick_kpl(a.k);
  const int nq = a.plan.rows.nq_tile;
#define EPS_CASE(NQ_, KPL_) \
  if (nq == NQ_ && kpl == KPL_) return launch_hybrid_tiles_t<NQ_, KPL_>(a, vec4, s);
  EPS_CASE(1, 1) EPS_CASE(2, 1) EPS_CASE(4, 1)
  EPS_CASE(1, 2) EPS_CASE(2, 2) EPS_CASE(4, 2)
  EPS_CASE(1, 4) EPS_CASE(1, 8) EPS_CASE(1, 16)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------
// One workgroup per query: its dense query and its sparse pairs in LDS, the four wavefronts stride over the query's k result slots, 64 / G of them
// at a time.  An unused slot gets +inf / +inf.
template <bool VEC4>
__global__ __launch_bounds__(256) void hybrid_parts_kernel(HybridArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float hyb_lds[];   // [qstride] dense query, [qcap] indices, [qcap] values
  const int dim = a.dim;
  const int qstride = a.plan.qstride;
  const int qcap = (int)a.plan.rows.qcap;
  float* const dq = hyb_lds;
  int* const q_idx = reinterpret_cast<int*>(hyb_lds + qstride);
  float* const q_val = hyb_lds + qstride + qcap;
  const int64_t q = blockIdx.x;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sp_metric = a.sp_metric;

  for (int i = threadIdx.x; i < qstride; i += 256) dq[i] = i < dim ? a.queries[q * dim + i] : 0.f;
  const int64_t qb = a.q_offsets[q];
  int64_t len64 = a.q_offsets[q + 1] - qb;
  len64 = len64 < qcap ? len64 : qcap;   // (the host refused a longer query)
  const int qlen = (int)len64;
  for (int i = threadIdx.x; i < qlen; i += 256) {
    q_idx[i] = a.q_indices[qb + i];
    q_val[i] = a.q_values[qb + i];
  }
  __syncthreads();
  float v2_prod = 0.0f;
  if (sp_metric == 1) {
    for (int i = 0; i < qlen; ++i) {
      const float v = q_val[i];
      const float sq = v * v;
      v2_prod = v2_prod + sq;
    }
  }

  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const float inf = __uint_as_float(0x7F800000u);
  for (int e0 = wave * RPW; e0 < a.k; e0 += HYB_BLOCK_WAVES * RPW) {   // (wave-uniform: row_dists' shuffles need every lane)
    const int e = e0 + g;
    const bool have = e < a.k;
    const u64 key = have ? a.run_keys[q * a.k + e] : KEY_EMPTY;
    const bool ok = key != KEY_EMPTY;
    const int64_t row = ok ? (int64_t)key_id(key) : 0;   // an unused slot: row 0's pointer, and no distance
    const float* rp[1] = {a.rows + row * dim};
    float dacc[1][1];
    row_dists<1, 1, VEC4>(rp, dq, qstride, dim, a.metric, G, dacc);
    if (t == 0 && have) {
      float dd = inf, ds = inf;
      if (ok) {
        dd = key_dist(make_key(finish_dist(a.metric, dacc[0][0]), 0u));   // (-0 as +0, a NaN as the quiet NaN: what a search returns)
        // the scan's walk: the row in stored order against the query's cursor, one accumulator from 0.0f
        const int64_t rb = a.sp_offsets[row], re = a.sp_offsets[row + 1];
        float s = 0.0f;
        int c = 0;
        for (int64_t i = rb; i < re && c < qlen; ++i) {
          const int ri = a.sp_indices[i];
          while (c < qlen && q_idx[c] < ri) ++c;
          if (c < qlen && q_idx[c] == ri) {
            const float pr = a.sp_values[i] * q_val[c];
            s = s + pr;
            ++c;
          }
        }
        const float v1_prod = sp_metric == 1 ? a.norms[row] : 0.0f;
        ds = key_dist(make_key(hybrid_sparse_finish(sp_metric, s, v1_prod, v2_prod), 0u));
      }
      if (a.dense_out) a.dense_out[q * a.k + e] = dd;
      if (a.sparse_out) a.sparse_out[q * a.k + e] = ds;
    }
  }
}

// an empty table: every slot is unused
__global__ __launch_bounds__(256) void hybrid_parts_empty_kernel(float* dense_out, float* sparse_out, int64_t slots) {
  const float inf = __uint_as_float(0x7F800000u);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256) {
    if (dense_out) dense_out[i] = inf;
    if (sparse_out) sparse_out[i] = inf;
  }
}

void launch_hybrid_parts(const HybridArgs& a, hipStream_t s) {
  if (a.nq <= 0 || (!a.dense_out && !a.sparse_out)) return;
  if (a.n <= 0) {
    const int64_t slots = a.nq * a.k, blocks = (slots + 255) / 256;
    hipLaunchKernelGGL(hybrid_parts_empty_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, a.dense_out, a.sparse_out, slots);
    return;
  }
  const size_t shm = (size_t)hybrid_parts_lds_bytes(a.dim, a.plan.rows.qcap);
  for (int64_t j0 = 0; j0 < a.nq; j0 += HYB_GRID_Y * 1024) {   // (slices of 2^25 queries: every slice's arrays start at its first query)
    const int64_t m = a.nq - j0 < HYB_GRID_Y * 1024 ? a.nq - j0 : HYB_GRID_Y * 1024;
    HybridArgs b = a;
    b.queries = a.queries + j0 * a.dim;
    b.q_offsets = a.q_offsets + j0;
    b.run_keys = a.run_keys + j0 * a.k;
    if (a.dense_out) b.dense_out = a.dense_out + j0 * a.k;
    if (a.sparse_out) b.sparse_out = a.sparse_out + j0 * a.k;
    if (rows_vec4(a.rows, a.dim))
      hipLaunchKernelGGL((hybrid_parts_kernel<true>), dim3((unsigned)m), dim3(256), shm, s, b);
    else
      hipLaunchKernelGGL((hybrid_parts_kernel<false>), dim3((unsigned)m), dim3(256), shm, s, b);
  }
}

}  // namespace eps
