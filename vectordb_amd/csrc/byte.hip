// Byte-vector fields (eps_byte_index_*): the exact top-k of a table of one-byte-per-dimension vectors, int8 or uint8, on the matrix cores.
// v_mfma_i32_16x16x64_i8 returns the exact integer dot product of 16 rows x 16 queries x 64 bytes, and row_term + query_term - (dot << shift) is the
// exact int32 distance (byte_host.hpp derives the terms): no bound, no re-rank, no tolerance.  A key is ((u32)(distance + 2^31) << 32 | row), so
// negative dot distances order as unsigned and ties go to the smaller row.
//
// byte_prepare_kernel   the stored form, at attach and per batch of queries: rows padded to whole 64-byte K-steps, unsigned bytes as b ^ 0x80, one
//                       int32 term per row.  One wavefront per row.
// byte_scan_kernel<NB, KPL>   256 threads = 4 wavefronts, each with a slice of consecutive rows of its own; blockIdx.y is a query tile of NB 16-column
//   blocks.  The tile's operands are staged once per workgroup in LDS as [column block][K-step][lane] x 16 bytes: lane l = (column c = l % 16, K group
//   g = l / 16) reads bytes [64 j + 16 g, +16) of query c with one conflict-free ds_read_b128, shared by the four wavefronts.  A wavefront walks its
//   slice in rounds of 64 rows = four 16-row blocks.  K is the outer loop of a round: per K-step a lane loads the same bytes of rows base + c of its
//   four blocks (four 16-byte global loads, the next step's requested before this step's MFMAs issue - two sets of 16 registers, never a whole row)
//   and issues 4 x NB MFMAs into acc[4][NB]; afterwards lane l holds rows base + 4 g + {0..3} of column c of every block.
//   Common path: a lane owns ONE query column per column block, so that column's threshold is a lane-private register: T = (k-th distance of this
//   wavefront's list) - query_term.  Per accumulator a shift, a subtract from the row term and a compare; one __any per round.  The compare is strict:
//   rows ascend inside a slice, so a later row AT the k-th distance has the larger key and offer would turn it down too.  A list that is not full
//   has T = INT32_MAX, an absent column INT32_MIN.
//   Hit path (wave-uniform, only when the vote is non-zero): the round's values go through a per-wavefront LDS patch, transposed to [row][column];
//   lane l then owns row base + l and offers its keys column by column to the wavefront's lists (device_common.hpp's offer: the deleted bitset, the
//   rows past the slice, absent columns never offered), and the lane-private thresholds are refreshed from thr[].
// The per-wavefront lists go out as partial[q][slice][k]; flat_kernels.hip's merge_lists_kernel joins them and byte_finalize_kernel writes the
// caller's arrays.  HBM traffic: n * d_pad bytes per query tile; matrix work: 2 * n * 16 NB * d_pad operations per tile, whatever the tile holds.
#include "kernels.hpp"

namespace eps {

// ------------------------------------------------------------------------------------------------ stored form
__global__ __launch_bounds__(256) void byte_prepare_kernel(const uint8_t* src, int64_t m, int64_t m_pad, int64_t dim, int64_t stride, int d_pad, int metric,
                                                           int is_unsigned, int is_query, signed char* dst, int32_t* term) {
  const int lane = lane_id();
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < m_pad; r += waves) {
    int s1 = 0, s2 = 0;
    for (int j0 = 0; j0 < d_pad; j0 += 64) {
      const int idx = j0 + lane;
      const int v = r < m && idx < dim ? byte_stored(src[r * stride + idx], is_unsigned) : 0;
      dst[r * d_pad + idx] = (signed char)v;
      s1 += v;
      s2 += v * v;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) term[r] = r < m ? byte_term(metric, is_unsigned, is_query, s1, s2, dim) : 0;
  }
}
void launch_byte_prepare(const uint8_t* src, int64_t m, int64_t m_pad, int64_t dim, int64_t stride, int metric, int is_unsigned, int is_query,
                         signed char* dst, int32_t* term, hipStream_t s) {
  if (m_pad <= 0) return;
  const int64_t blocks = (m_pad + 3) / 4;
  hipLaunchKernelGGL(byte_prepare_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, src, m, m_pad, dim, stride, (int)byte_pad(dim),
                     metric, is_unsigned, is_query, dst, term);
}

// ------------------------------------------------------------------------------------------------ the scan
constexpr int byte_lists(int nb, int kpl) { return BYTE_LIST_BUDGET / kpl < 16 * nb ? BYTE_LIST_BUDGET / kpl : 16 * nb; }   // BytePlan::cols

// (every form is given the register file of a SIMD's two wavefronts: 128 list registers, 32 accumulators, 2 x 16 row operands - no scratch)
template <int NB, int KPL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void byte_scan_kernel(ByteScanArgs a, int64_t tile0) {
  constexpr int NQ = byte_lists(NB, KPL);
  constexpr int PITCH = 16 * NB + 4;   // byte_patch_pitch(NB)
  extern __shared__ i32x4 byte_lds[];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15, kg = lane >> 4;
  const int KS = a.d_pad / BYTE_KSTEP;
  i32x4* const q_s = byte_lds;                                                                  // [NB][KS][64]
  int* const patch = reinterpret_cast<int*>(byte_lds + NB * KS * 64) + wave * BYTE_WAVE_ROWS * PITCH;   // [64][PITCH], this wavefront's
  const int64_t slice = (int64_t)blockIdx.x * BYTE_BLOCK_WAVES + wave;
  const int64_t q0 = (tile0 + blockIdx.y) * NQ;
  const int nq_here = a.nq - q0 < NQ ? (int)(a.nq - q0) : NQ;   // >= 1: the grid holds no empty tile

  // ---- the tile's operands: zeros for the columns the tile does not have
  for (int i = threadIdx.x; i < NB * KS * 64; i += 256) {
    const int l = i & 63, j = (i >> 6) % KS, b = (i >> 6) / KS;
    const int qc = 16 * b + (l & 15);
    i32x4 v = {0, 0, 0, 0};
    if (qc < nq_here) v = *reinterpret_cast<const i32x4*>(a.queries + (q0 + qc) * a.d_pad + j * BYTE_KSTEP + (l >> 4) * 16);
    q_s[i] = v;
  }
  __syncthreads();   // (the only barrier: from here on the wavefronts go their own ways)

  int64_t row_begin, row_end;
  byte_slice_rows(a.plan.rows_per_slice, a.n, slice, &row_begin, &row_end);
  FilterSpec f = no_filter();   // (built here: the compiler sees that nothing but the bitset is ever asked)
  f.deleted = a.deleted;
  WaveTopK<KPL> list[NQ];
  u64 thr[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    list[q].init();
    thr[q] = KEY_EMPTY;
  }
  int qt[NB], T[NB];   // this lane's columns: their query terms and thresholds
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int qc = col + 16 * b;
    qt[b] = qc < nq_here ? a.query_term[q0 + qc] : 0;
    T[b] = qc < nq_here ? 2147483647 : -2147483647 - 1;
  }
  const int sh = a.shift;
  const int64_t block_bytes = (int64_t)16 * a.d_pad;
  u32 hits = 0;

  for (int64_t r0 = row_begin; r0 < row_end; r0 += BYTE_WAVE_ROWS) {   // (r0 + 63 < byte_pad_rows(n): the table and the terms are padded to whole rounds)
    const signed char* const ap = a.rows + (r0 + col) * a.d_pad + kg * 16;
    i32x4 rt[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) rt[rb] = *reinterpret_cast<const i32x4*>(a.row_term + r0 + rb * 16 + 4 * kg);
    i32x4 acc[4][NB];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[rb][b] = i32x4{0, 0, 0, 0};
    auto load = [&](i32x4 (&x)[4], int j) __attribute__((always_inline)) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) x[rb] = *reinterpret_cast<const i32x4*>(ap + rb * block_bytes + j * BYTE_KSTEP);
    };
    auto mma = [&](const i32x4 (&x)[4], int j) __attribute__((always_inline)) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const i32x4 qv = q_s[(b * KS + j) * 64 + lane];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[rb][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x[rb], qv, acc[rb][b], 0, 0, 0);
      }
    };
    i32x4 xa[4], xb[4];   // two K-steps' row operands, in turns
    load(xa, 0);
    int j = 0;
    for (; j + 2 <= KS; j += 2) {
      load(xb, j + 1);
      mma(xa, j);
      if (j + 2 < KS) load(xa, j + 2);
      mma(xb, j + 1);
    }
    if (j < KS) mma(xa, j);

    // ---- common path: distance - query_term against the lane's thresholds
    bool vote = false;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = rt[rb][i] - (int)((u32)acc[rb][b][i] << sh);
          acc[rb][b][i] = p;
          vote |= p < T[b];
        }
    if (!__any(vote)) continue;

    // ---- hit path
    ++hits;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) patch[(rb * 16 + 4 * kg + i) * PITCH + col + 16 * b] = acc[rb][b][i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (one wavefront writes and reads the patch; its LDS operations complete in order)
    __builtin_amdgcn_wave_barrier();
    const int64_t row = r0 + lane;
    const bool valid = row < row_end;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q < nq_here) {
        const int d = patch[lane * PITCH + q] + a.query_term[q0 + q];
        const u64 key = ((u64)((u32)d ^ 0x80000000u) << 32) | (u64)(u32)row;
        offer<NQ, KPL>(list, thr, q, key, valid, f, a.k, false);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int qc = col + 16 * b;
      u64 t = KEY_EMPTY;
#pragma unroll
      for (int q = 0; q < NQ; ++q) t = qc == q ? thr[q] : t;
      if (qc < nq_here) T[b] = t == KEY_EMPTY ? 2147483647 : (int)((u32)(t >> 32) ^ 0x80000000u) - qt[b];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q < nq_here) list[q].store(a.partial + ((q0 + q) * a.plan.slices + slice) * a.k, a.k);   // (a slice beyond the table: an empty list)
  if (hits && lane == 0) atomicAdd(a.hit_rounds, (u64)hits);
}

template <int NB, int KPL>
static void launch_byte_scan_t(const ByteScanArgs& a, hipStream_t s) {
  for (int64_t tile0 = 0; tile0 < a.plan.tiles; tile0 += BIN_GRID_Y) {
    const int64_t gy = a.plan.tiles - tile0 < BIN_GRID_Y ? a.plan.tiles - tile0 : BIN_GRID_Y;
    const dim3 grid((unsigned)(a.plan.slices / BYTE_BLOCK_WAVES), (unsigned)gy);
    hipLaunchKernelGGL((byte_scan_kernel<NB, KPL>), grid, dim3(256), (size_t)a.plan.lds_bytes, s, a, tile0);
  }
}

#define EPS_BYTE_FORMS(X) X(2, 1) X(1, 1) X(1, 2) X(1, 4) X(1, 8) X(1, 16)

void byte_scan_allow_lds() {
#define EPS_CASE(NB_, KPL_) \
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(byte_scan_kernel<NB_, KPL_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                            (int)byte_lds_bytes(NB_, BYTE_LDS_QUERY_BYTES / (16 * NB_)));
  EPS_BYTE_FORMS(EPS_CASE)
#undef EPS_CASE
}

void launch_byte_scan(const ByteScanArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
#define EPS_CASE(NB_, KPL_) \
  if (a.plan.nb == NB_ && a.plan.kpl == KPL_) return launch_byte_scan_t<NB_, KPL_>(a, s);
  EPS_BYTE_FORMS(EPS_CASE)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------ results
__global__ __launch_bounds__(256) void byte_finalize_kernel(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids,
                                                            int32_t* dist, int32_t* counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const u64 key = run_keys[i];
  const bool valid = key != KEY_EMPTY;
  ids[i] = valid ? (int64_t)key_id(key) * id_stride + id_base : -1;
  dist[i] = valid ? (int32_t)((u32)(key >> 32) ^ 0x80000000u) : 2147483647;
  if (counts && (i % k) == 0) {
    int c = 0;
    for (int e = 0; e < k; ++e) c += run_keys[i + e] != KEY_EMPTY;
    counts[i / k] = c;
  }
}
void launch_byte_finalize(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids, int32_t* dist, int32_t* counts,
                          hipStream_t s) {
  const int64_t n = nq * k;
  if (n <= 0) return;
  hipLaunchKernelGGL(byte_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, run_keys, nq, k, id_base, id_stride, ids, dist, counts);
}

}  // namespace eps
