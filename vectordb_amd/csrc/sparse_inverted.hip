// Inverted lists of a sparse-vector field (eps_sparse_index_build_inverted): the CSR table stored by column, and the term-at-a-time form of
// GetInnerProduct / GetCosineDist (reference: engine/db/vector.cpp:11-47) on it.
//
// The rule.  The reference adds a product only on a matching index, into ONE fp32 accumulator that starts at 0.0f, in ascending index order.  So a
// per-row accumulator that receives `acc = acc + (row_value * query_value)` once per query term present in the row, the terms applied in ascending
// index order, holds the reference's bits: the same operands meet the same additions in the same order.  Term order is the whole contract - and a
// product rounded before it is added: hipcc contracts `s += a * b` into v_fmac_f32 unless `#pragma clang fp contract(off)` covers the statement,
// so the pragma stands at file scope here and again in every block that sums, and no sum is taken in a helper of another header.
//
// The image: col_offsets int64[dim + 1] and nnz postings (row, value) - column c's rows, strictly ascending, at [col_offsets[c], col_offsets[c + 1]).
// The CSR is ascending in row already, so a STABLE sort of its elements by column is the whole build: up to three 8-bit LSD passes over the bits of
// dim - 1 (sparse_inv_sort_plan), each one per-block digit histograms, a scan of the [digit][block] table and a scatter whose ranks inside a
// wavefront come from ballots - every step keeps equal digits in their order, and nothing depends on the order atomics arrive in, so the image is
// the same bits on every build.  The directory is a column histogram (integer atomics) and a scan.  (rocprim's device radix sort was the first
// choice for this one-off step; its kernels spill to scratch memory and the library would import getenv through it, which this one does not.)
//
// sparse_inverted_kernel keeps the scan's outer plan - grid.y over queries, a wavefront owns the rows sparse_wave_rows gives it and ONE k-list over
// all of them - and walks its rows in tiles of SPARSE_INV_TILE_ROWS whose accumulators live in the wavefront's own LDS slice:
//   match   64 terms per round, one per lane: the lane binary-searches ITS column's postings for the rows of the tile (bounds from the directory
//           only, so no probe leaves the arrays; an empty column is an empty range)
//   sum     the lanes with a non-empty range are taken in ascending lane = index order; the range and the query value are broadcast and the lanes
//           stride over the postings.  Rows of one column are distinct, so no two lanes meet, and one wavefront's LDS operations complete in
//           program order, so the next term sees this one's sums without a workgroup barrier
//   finish  every row of the tile - touched or not - reads its accumulator (and leaves 0.0f for the next tile), gets the metric's epilogue and is
//           offered to the list
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace eps {

// ------------------------------------------------------------------------------------------------ build
// one wavefront per row and step: the row's elements as (row, value) pairs in CSR order, and the histogram of their columns into col_offsets[c + 1]
__global__ __launch_bounds__(256) void sparse_inv_expand_kernel(SparseInvBuildArgs a, SparsePosting* pairs) {
  const int lane = lane_id();
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.n; r += waves) {
    const int64_t b = a.offsets[r], e = a.offsets[r + 1];   // (validated: 0 <= b <= e <= nnz)
    for (int64_t i = b + lane; i < e; i += 64) {
      SparsePosting p;
      p.row = (int32_t)r;
      p.value = a.values[i];
      pairs[i] = p;
      atomicAdd(reinterpret_cast<u64*>(a.col_offsets) + a.indices[i] + 1, 1ull);   // (validated: 0 <= index < dim)
    }
  }
}

// ONE workgroup scans v[0 .. len) in place: thread t owns a contiguous run, the 1024 run sums are scanned in LDS.  inclusive = 1: the directory
// (counts at [c + 1], 0 at [0]); 0: the [digit][block] table of a sort pass
__global__ __launch_bounds__(1024) void sparse_inv_scan_kernel(u64* v, int64_t len, int inclusive) {
  __shared__ u64 run_sum[1024];
  const int64_t per = (len + 1023) / 1024;
  const int64_t b = threadIdx.x * per < len ? threadIdx.x * per : len;
  const int64_t e = len - b < per ? len : b + per;
  u64 sum = 0;
  for (int64_t i = b; i < e; ++i) sum += v[i];
  run_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 before = 0;
    for (int t = 0; t < 1024; ++t) {
      const u64 s = run_sum[t];
      run_sum[t] = before;
      before += s;
    }
  }
  __syncthreads();
  u64 running = run_sum[threadIdx.x];
  for (int64_t i = b; i < e; ++i) {
    const u64 x = v[i];
    v[i] = inclusive ? running + x : running;
    running += x;
  }
}

// after the scan: the longest column
__global__ __launch_bounds__(256) void sparse_inv_longest_kernel(const int64_t* col_offsets, int64_t dim, u64* longest) {
  u64 most = 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < dim; c += (int64_t)gridDim.x * 256) {
    const u64 len = (u64)(col_offsets[c + 1] - col_offsets[c]);
    most = len > most ? len : most;
  }
  if (most) atomicMax(longest, most);
}

// a sort pass, step 1: block b counts the digits of ITS chunk of the keys into table[digit][b]
__global__ __launch_bounds__(256) void sparse_inv_digits_kernel(const int32_t* keys, int64_t nnz, SparseInvSortPlan sp, int shift, u64* table) {
  __shared__ unsigned int count[256];
  count[threadIdx.x] = 0;
  __syncthreads();
  int64_t b, e;
  sparse_inv_chunk(sp, nnz, blockIdx.x, &b, &e);
  for (int64_t i = b + threadIdx.x; i < e; i += 256) atomicAdd(&count[((u32)keys[i] >> shift) & 255u], 1u);   // (a chunk holds fewer than 2^32 keys)
  __syncthreads();
  table[(int64_t)threadIdx.x * sp.blocks + blockIdx.x] = count[threadIdx.x];
}

// a sort pass, step 3: block b walks its chunk 256 keys at a time.  An element goes to next[digit] + the same digit's count in the wavefronts in
// front of its own + its rank among the equal digits of its own wavefront's lower lanes: equal digits keep their order.  next[] starts at the
// scanned table's entry for (digit, b), so every destination lies inside [0, nnz) - the table was counted over the same chunks of the same keys.
__global__ __launch_bounds__(256) void sparse_inv_scatter_kernel(const int32_t* keys, const SparsePosting* pairs, int64_t nnz, SparseInvSortPlan sp, int shift,
                                                                 const u64* table, int32_t* keys_out, SparsePosting* pairs_out) {
  __shared__ u64 next[256];
  __shared__ unsigned int wave_count[4][256];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  next[threadIdx.x] = table[(int64_t)threadIdx.x * sp.blocks + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) wave_count[w][threadIdx.x] = 0;
  __syncthreads();
  int64_t b, e;
  sparse_inv_chunk(sp, nnz, blockIdx.x, &b, &e);
  for (int64_t i0 = b; i0 < e; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    const bool valid = i < e;
    int32_t key = 0;
    SparsePosting p;
    p.row = 0;
    p.value = 0.0f;
    if (valid) {
      key = keys[i];
      p = pairs[i];
    }
    const u32 d = ((u32)key >> shift) & 255u;
    u64 peers = __ballot(valid);   // the valid lanes of this wavefront that hold the same digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const u64 m = __ballot(valid && one);
      peers &= one ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wave_count[wave][d] = (unsigned int)__popcll(peers);
    __syncthreads();
    if (valid) {
      u64 at = next[d] + (u64)rank;
      for (int w = 0; w < wave; ++w) at += wave_count[w][d];
      if (keys_out) keys_out[at] = key;
      pairs_out[at] = p;
    }
    __syncthreads();
    {
      const int t = threadIdx.x;   // digit t: move on past this step's elements, clear the counts
      next[t] += (u64)wave_count[0][t] + wave_count[1][t] + wave_count[2][t] + wave_count[3][t];
#pragma unroll
      for (int w = 0; w < 4; ++w) wave_count[w][t] = 0;
    }
    __syncthreads();
  }
}

// the image of a validated CSR; everything on stream s, nothing read back
hipError_t launch_sparse_inv_build(const SparseInvBuildArgs& a, hipStream_t s) {
  hipError_t e = hipMemsetAsync(a.col_offsets, 0, (size_t)(a.dim + 1) * sizeof(int64_t), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.longest, 0, sizeof(u64), s);
  if (e != hipSuccess) return e;
  const SparseInvSortPlan sp = sparse_inv_sort_plan(a.nnz, a.dim);
  // the pairs end in a.postings after the last pass: an odd number of passes starts from the scratch copy, an even one from the image's own array
  SparsePosting* from = (sp.passes & 1) ? a.pairs : a.postings;
  SparsePosting* to = (sp.passes & 1) ? a.postings : a.pairs;
  if (a.n > 0 && a.nnz > 0) hipLaunchKernelGGL(sparse_inv_expand_kernel, dim3((unsigned)sparse_inv_build_blocks(a.n, 4)), dim3(256), 0, s, a, from);
  hipLaunchKernelGGL(sparse_inv_scan_kernel, dim3(1), dim3(1024), 0, s, reinterpret_cast<u64*>(a.col_offsets), a.dim + 1, 1);
  hipLaunchKernelGGL(sparse_inv_longest_kernel, dim3((unsigned)sparse_inv_build_blocks(a.dim, 256)), dim3(256), 0, s, a.col_offsets, a.dim, a.longest);
  if (a.nnz > 0) {
    const int32_t* keys = a.indices;
    int32_t* keys_to = a.keys_a;
    for (int pass = 0; pass < sp.passes; ++pass) {
      const bool last = pass + 1 == sp.passes;
      hipLaunchKernelGGL(sparse_inv_digits_kernel, dim3((unsigned)sp.blocks), dim3(256), 0, s, keys, a.nnz, sp, pass * 8, a.table);
      hipLaunchKernelGGL(sparse_inv_scan_kernel, dim3(1), dim3(1024), 0, s, a.table, 256 * sp.blocks, 0);
      hipLaunchKernelGGL(sparse_inv_scatter_kernel, dim3((unsigned)sp.blocks), dim3(256), 0, s, keys, (const SparsePosting*)from, a.nnz, sp, pass * 8,
                         (const u64*)a.table, last ? nullptr : keys_to, to);
      keys = keys_to;
      keys_to = keys_to == a.keys_a ? a.keys_b : a.keys_a;
      SparsePosting* t = from;
      from = to;
      to = t;
    }
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ search
// first posting of [lo, hi) whose row is >= `row` (hi if none): every probe lies inside [lo, hi)
__device__ __forceinline__ int64_t sparse_inv_lower_bound(const SparsePosting* p, int64_t lo, int64_t hi, int64_t row) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)p[mid].row < row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int KPL>
__global__ __launch_bounds__(256) void sparse_inverted_kernel(SparseInvArgs a, int64_t q_base) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) int sparse_inv_lds[];   // [qcap] indices, [qcap] values, [SPARSE_BLOCK_WAVES][SPARSE_INV_TILE_ROWS] accumulators
  const int qcap = (int)a.plan.rows.qcap;
  int* const q_idx = sparse_inv_lds;
  float* const q_val = reinterpret_cast<float*>(sparse_inv_lds + qcap);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  float* const acc = reinterpret_cast<float*>(sparse_inv_lds + 2 * qcap) + wave * SPARSE_INV_TILE_ROWS;
  const int64_t q = q_base + blockIdx.y;
  const int metric = a.metric;

  // ---- the query, once per workgroup; every wavefront clears its own accumulators
  const int64_t qb = a.q_offsets[q];
  int64_t len64 = a.q_offsets[q + 1] - qb;
  len64 = len64 < qcap ? len64 : qcap;   // (the host refused a longer query)
  const int qlen = (int)len64;
  for (int i = threadIdx.x; i < qlen; i += 256) {
    q_idx[i] = a.q_indices[qb + i];
    q_val[i] = a.q_values[qb + i];
  }
  for (int i = lane; i < SPARSE_INV_TILE_ROWS; i += 64) acc[i] = 0.0f;
  __syncthreads();
  float v2_prod = 0.0f;   // the query's squares in stored order (every lane takes the same sum: the reads are broadcasts)
  if (metric == 1) {
    for (int i = 0; i < qlen; ++i) {
      const float v = q_val[i];
      const float sq = v * v;
      v2_prod = v2_prod + sq;
    }
  }

  const int W = a.plan.rows.W;
  const int64_t w = (int64_t)blockIdx.x * SPARSE_BLOCK_WAVES + wave;
  int64_t row_begin, row_end;
  sparse_wave_rows(a.plan.rows, a.n, w, &row_begin, &row_end);

  WaveTopK<KPL> list[1];
  u64 thr[1];
  list[0].init();
  thr[0] = KEY_EMPTY;

  for (int64_t t0 = row_begin; t0 < row_end; t0 += SPARSE_INV_TILE_ROWS) {
    const int64_t t1 = row_end - t0 < SPARSE_INV_TILE_ROWS ? row_end : t0 + SPARSE_INV_TILE_ROWS;
    for (int base = 0; base < qlen; base += SPARSE_INV_TERMS) {
      // ---- match: one term per lane
      const int term = base + lane;
      int64_t lo = 0, hi = 0;
      float qv = 0.0f;
      if (term < qlen) {
        const int64_t c = q_idx[term];   // (validated: 0 <= c < dim, and the directory has dim + 1 entries)
        qv = q_val[term];
        const int64_t cb = a.col_offsets[c], ce = a.col_offsets[c + 1];
        lo = sparse_inv_lower_bound(a.postings, cb, ce, t0);
        hi = sparse_inv_lower_bound(a.postings, lo, ce, t1);
      }
      // ---- sum: the terms that have postings in this tile, in ascending index order
      u64 m = __ballot(hi > lo);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t b = (int64_t)shfl64((u64)lo, l), e = (int64_t)shfl64((u64)hi, l);
        const float v = __shfl(qv, l);
        for (int64_t i = b + lane; i < e; i += 64) {
          const SparsePosting p = a.postings[i];
          const int slot = (int)((int64_t)p.row - t0);
          const float pr = p.value * v;
          const float s = acc[slot];
          acc[slot] = s + pr;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the next term's lanes read what this term's lanes wrote)
      }
    }
    // ---- finish: every row of the tile is a row at some distance
    for (int64_t r0 = t0; r0 < t1; r0 += SPARSE_WAVE_ROWS) {
      const int64_t r = r0 + lane;
      const bool fin = r < t1;
      const int64_t rr = fin ? r : t1 - 1;
      float s = 0.0f;
      if (fin) {
        s = acc[rr - t0];
        acc[rr - t0] = 0.0f;
      }
      if (metric == 1) {
        const float v1_prod = fin ? a.norms[rr] : 0.0f;
        const float pp = v1_prod * v2_prod;
        const float root = sqrtf(pp);
        const float quot = s / root;
        s = 1.0f - quot;
      } else {
        s = -s;
      }
      const u64 key = make_key(s, (u32)rr);
      offer<1, KPL>(list, thr, 0, key, fin, a.f, a.k, false);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the next tile's sums start from the zeros written here)
  }
  list[0].store(a.partial + (q * W + w) * a.k, a.k);   // (a wavefront beyond the table: an empty list)
}

template <int KPL>
static void launch_sparse_inverted_t(const SparseInvArgs& a, hipStream_t s) {
  for (int64_t q0 = 0; q0 < a.nq; q0 += SPARSE_GRID_Y) {
    const int64_t gy = a.nq - q0 < SPARSE_GRID_Y ? a.nq - q0 : SPARSE_GRID_Y;
    const dim3 grid((unsigned)(a.plan.rows.W / SPARSE_BLOCK_WAVES), (unsigned)gy);
    hipLaunchKernelGGL((sparse_inverted_kernel<KPL>), grid, dim3(256), (size_t)a.plan.lds_dynamic, s, a, q0);
  }
}

void launch_sparse_inverted(const SparseInvArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
  switch (pick_kpl(a.k)) {
    case 1: return launch_sparse_inverted_t<1>(a, s);
    case 2: return launch_sparse_inverted_t<2>(a, s);
    case 4: return launch_sparse_inverted_t<4>(a, s);
    case 8: return launch_sparse_inverted_t<8>(a, s);
    default: return launch_sparse_inverted_t<16>(a, s);
  }
}

}  // namespace eps
