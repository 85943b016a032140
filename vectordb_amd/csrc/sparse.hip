// Sparse-vector fields (eps_sparse_index_*): the device form of BruteForceSearch calling GetL2DistSqr / GetCosineDist / GetInnerProductDist row by
// row on SPARSE_VECTOR_FLOAT fields (reference: engine/db/vector.cpp:7-96, db/index/index.cpp:22-34, db/execution/vec_search_executor.cpp:742).
//
// The table is CSR.  A distance is, bit for bit, what the reference's function returns for (v1 = row, v2 = query): ONE fp32 accumulator from 0.0f, the
// two-pointer merge in ascending index order, every product rounded before it is added.  hipcc contracts `s += a * b` (and the _rn intrinsics) into
// v_fmac_f32 unless `#pragma clang fp contract(off)` covers the statement, so the pragma stands at file scope here and again in every block that
// sums, and no sum is taken in a helper of another header.
//
// sparse_scan_kernel: a wavefront takes 64 consecutive rows per round, one row per lane.  Every lane walks ITS row straight from the arrays, in
// stored order (the next element requested before this one is merged; the 64 rows are one contiguous range, so the wavefront's lines are
// neighbours in the caches), against each of the NQ queries staged in LDS; accumulators and query cursors are registers, so a row may be of any
// length.  When the wavefront is together again every lane finishes its pairs and offers its keys to the wavefront's k-lists (device_common.hpp's
// offer: only a key that would enter a list is judged against the deleted bitset).  Algorithmic traffic: 8 * nnz + 8 * n bytes per tile of NQ
// queries (+ 4 * n under COSINE).  The first form staged the 64 rows' elements in LDS, SPARSE_PIECE = 512 at a time, with coalesced loads, and
// every lane merged its row's part of the piece: a piece holds 512 / row length rows, so at 128 non-zeros per row 4 of 64 lanes worked - measured
// slower at that length than this form (DESIGN 5.7 has both).
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace eps {

// ------------------------------------------------------------------------------------------------ validation
// One thread per row.  A row's elements are read only after ITS two offsets were found ordered and inside [0, nnz], so no input makes the pass
// read outside the three arrays.  The row's sum of squares (GetCosineDist's v1_prod) is taken in stored order on the way.
__global__ __launch_bounds__(256) void sparse_validate_kernel(SparseValidateArgs a) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n) return;
  const int64_t b = a.offsets[r], e = a.offsets[r + 1];
  int32_t bad = SPARSE_BAD_NONE;
  float sum = 0.0f;
  if (r == 0 && b != 0) {
    bad = SPARSE_BAD_FIRST;
  } else if (b < 0 || e < b || e > a.nnz) {
    bad = SPARSE_BAD_OFFSETS;
  } else {
    int64_t prev = -1;
    for (int64_t i = b; i < e; ++i) {
      const int64_t c = a.indices[i];
      if (c < 0 || c >= a.dim) {
        bad = SPARSE_BAD_RANGE;
        break;
      }
      if (c <= prev) {
        bad = SPARSE_BAD_ORDER;
        break;
      }
      prev = c;
      const float v = a.values[i];
      const float sq = v * v;
      sum = sum + sq;
    }
    if (!bad) atomicMax(&a.verdict->longest, (u64)(e - b));
  }
  if (a.norms) a.norms[r] = sum;
  if (bad) atomicMin(&a.verdict->first_bad, ((u64)r << 3) | (u64)bad);
}

void launch_sparse_validate(const SparseValidateArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(sparse_validate_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------ scan
template <int NQ, int KPL>
__global__ __launch_bounds__(256) void sparse_scan_kernel(SparseScanArgs a, int64_t tile0) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) int sparse_q[];   // [NQ][qcap] indices, then [NQ][qcap] values
  __shared__ int s_qlen[NQ];
  __shared__ float s_qnorm[NQ];
  const int qcap = (int)a.plan.qcap;
  int* const q_idx = sparse_q;
  float* const q_val = reinterpret_cast<float*>(sparse_q + NQ * qcap);
  const int64_t q0 = (tile0 + blockIdx.y) * NQ;
  const int metric = a.metric;

  // ---- the tile's queries, once per workgroup
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const bool have = q0 + q < a.nq;
    const int64_t qb = have ? a.q_offsets[q0 + q] : 0;
    int64_t len = have ? a.q_offsets[q0 + q + 1] - qb : 0;
    len = len < qcap ? len : qcap;   // (the host refused a longer query)
    for (int i = threadIdx.x; i < (int)len; i += 256) {
      q_idx[q * qcap + i] = a.q_indices[qb + i];
      q_val[q * qcap + i] = a.q_values[qb + i];
    }
    if (threadIdx.x == 0) s_qlen[q] = (int)len;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {   // v2_prod: the query's squares in stored order
    const int q = threadIdx.x;
    float sum = 0.0f;
    for (int i = 0; i < s_qlen[q]; ++i) {
      const float v = q_val[q * qcap + i];
      const float sq = v * v;
      sum = sum + sq;
    }
    s_qnorm[q] = sum;
  }
  __syncthreads();

  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int W = a.plan.W;
  const int64_t w = (int64_t)blockIdx.x * SPARSE_BLOCK_WAVES + wave;
  int64_t row_begin, row_end;
  sparse_wave_rows(a.plan, a.n, w, &row_begin, &row_end);

  WaveTopK<KPL> list[NQ];
  u64 thr[NQ];
  int qlen[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    list[q].init();
    thr[q] = KEY_EMPTY;
    qlen[q] = s_qlen[q];
  }

  for (int64_t r0 = row_begin; r0 < row_end; r0 += SPARSE_WAVE_ROWS) {
    const int64_t r = r0 + lane;
    const bool valid = r < row_end;
    const int64_t rr = valid ? r : row_end;                    // (offsets has n + 1 entries and row_end <= n)
    const int64_t beg = a.offsets[rr];
    const int64_t end = valid ? a.offsets[rr + 1] : beg;
    float acc[NQ];
    int cur[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      acc[q] = 0.0f;
      cur[q] = 0;
    }
    {
      // the lane walks its row in stored order; the next element is requested before this one is merged
      int ri_next = 0;
      float rv_next = 0.0f;
      if (beg < end) {
        ri_next = a.indices[beg];
        rv_next = a.values[beg];
      }
      for (int64_t i = beg; i < end; ++i) {
        const int ri = ri_next;
        const float rv = rv_next;
        if (i + 1 < end) {
          ri_next = a.indices[i + 1];
          rv_next = a.values[i + 1];
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int* qi = q_idx + q * qcap;
          const float* qv = q_val + q * qcap;
          int c = cur[q];
          float s = acc[q];
          while (c < qlen[q] && qi[c] < ri) {   // the query's entries in front of this index: L2 adds their squares, a dot product passes them
            if (metric == 0) {
              const float v = qv[c];
              const float sq = v * v;
              s = s + sq;
            }
            ++c;
          }
          if (c < qlen[q] && qi[c] == ri) {
            const float v = qv[c];
            if (metric == 0) {
              const float d = rv - v;
              const float sq = d * d;
              s = s + sq;
            } else {
              const float pr = rv * v;
              s = s + pr;
            }
            ++c;
          } else if (metric == 0) {
            const float sq = rv * rv;
            s = s + sq;
          }
          cur[q] = c;
          acc[q] = s;
        }
      }
      // the wavefront is together again: finish the pairs, offer the keys
      const bool fin = valid;
      const float v1_prod = (fin && metric == 1) ? a.norms[rr] : 0.0f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float s = acc[q];
        if (metric == 0) {
          if (fin) {   // the tail of the query
            const float* qv = q_val + q * qcap;
            for (int c = cur[q]; c < qlen[q]; ++c) {
              const float v = qv[c];
              const float sq = v * v;
              s = s + sq;
            }
          }
        } else if (metric == 1) {
          const float pp = v1_prod * s_qnorm[q];
          const float root = sqrtf(pp);
          const float quot = s / root;
          s = 1.0f - quot;
        } else {
          s = -s;
        }
        const u64 key = make_key(s, (u32)rr);
        offer<NQ, KPL>(list, thr, q, key, fin && q0 + q < a.nq, a.f, a.k, false);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q0 + q < a.nq) list[q].store(a.partial + ((q0 + q) * W + w) * a.k, a.k);   // (a wavefront beyond the table: an empty list)
}

template <int NQ, int KPL>
static void launch_sparse_scan_t(const SparseScanArgs& a, hipStream_t s) {
  for (int64_t tile0 = 0; tile0 < a.plan.tiles; tile0 += SPARSE_GRID_Y) {
    const int64_t gy = a.plan.tiles - tile0 < SPARSE_GRID_Y ? a.plan.tiles - tile0 : SPARSE_GRID_Y;
    const dim3 grid((unsigned)(a.plan.W / SPARSE_BLOCK_WAVES), (unsigned)gy);
    hipLaunchKernelGGL((sparse_scan_kernel<NQ, KPL>), grid, dim3(256), (size_t)a.plan.lds_dynamic, s, a, tile0);
  }
}

void launch_sparse_scan(const SparseScanArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
  const int kpl = pick_kpl(a.k);
  const int nq = a.plan.nq_tile;
#define EPS_CASE(NQ_, KPL_) \
  if (nq == NQ_ && kpl == KPL_) return launch_sparse_scan_t<NQ_, KPL_>(a, s);
  EPS_CASE(1, 1) EPS_CASE(2, 1) EPS_CASE(4, 1)
  EPS_CASE(1, 2) EPS_CASE(2, 2) EPS_CASE(4, 2)
  EPS_CASE(1, 4) EPS_CASE(1, 8) EPS_CASE(1, 16)
#undef EPS_CASE
}

}  // namespace eps
