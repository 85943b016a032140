// Half-vector fields (eps_half_index_*): the top-k of a table of fp16 or bf16 vectors on the matrix cores, with no fp32 original behind it.
// The rule: a vector is 1 <= dim <= 4096 elements of IEEE fp16 or of bf16, as the handle was created.  An fp16 x fp16 product has a 22-bit
// significand and a bf16 x bf16 product a 16-bit one, so v_mfma_f32_16x16x32_f16 / _bf16 take every product exactly and only the sums round:
//   x.q          the matrix cores' fp32 sum of the exact products, K-steps of 32 elements in ascending order into one accumulator
//   |x|^2, |q|^2 one fp32 term per row (written at attach) and per query (written per call) by half_prepare_kernel's one order: lane l of a
//                wavefront chains fmaf(v, v, s) over elements l, l + 64, l + 128, ... and the 64 chains are added by an xor butterfly, offsets
//                1, 2, 4, 8, 16, 32.  0 for the two dot metrics
//   EUCLIDEAN    t = (|x|^2 + |q|^2) - 2 x.q, t < 0 ? 0 : t   (a NaN stays a NaN)        DOT_PRODUCT  -x.q        COSINE  1 - x.q (normalising is
//                the caller's job, as everywhere in this library)
// half_distance() below is that expression and the only place a distance is computed - the threshold test, the offered key and the seed pass all
// go through it - so one row has one value in a call.  Order is (distance, row) ascending on device_common.hpp's float keys: a NaN distance orders
// behind +inf, as in the flat search.  A row with an infinite element has |x|^2 = inf and x.q = +-inf or NaN: its EUCLIDEAN distance is a NaN here
// (the flat search's difference form gives +inf); both order behind every number.  Subnormal fp16 inputs: the matrix cores read them
// as their values, as the norm terms do - measured on an MI355X (tests/test_gpu_half_rounds.py: rows of integers x 2^-24 answer bit for bit).
//
// half_convert_kernel   float -> half, round to nearest even on the bits (half_host.hpp's half_from_float_bits).
// half_prepare_kernel   the stored form, at attach and per batch of queries: rows of halves (or of floats, rounded as above) padded with zeros to
//                       d_pad = ceil(dim / 32) * 32 elements, one fp32 norm term per row.  One wavefront per row.
// half_scan_kernel<NB, KPL, BF16>   256 threads = 4 wavefronts, each with a slice of consecutive rows of its own; blockIdx.y is a query tile of NB
//   16-column blocks.  The tile's operands are staged once per workgroup in LDS as [column block][K-step][lane] x 16 bytes: lane l = (column
//   c = l % 16, K group g = l / 16) reads elements [32 j + 8 g, +8) of query c with one conflict-free ds_read_b128, shared by the four wavefronts.
//   NB = 4 (64 queries) fills 128 KB of the workgroup's 160 KB up to d_pad = 1024, NB = 2 up to 2048, NB = 1 above.  A wavefront walks its slice in
//   rounds of 64 rows = four 16-row blocks.  K is the outer loop of a round: per K-step a lane loads the same elements of rows base + c of its four
//   blocks (four 16-byte global loads, the next step's requested before this step's 4 NB MFMAs issue - two sets of 16 registers, never a whole
//   row); afterwards lane l holds rows base + 4 g + {0..3} of column c of every block in acc[4][NB].
//   Common path (no LDS, no list): a lane owns ONE query column per column block, so that column's threshold is a lane-private float T; per
//   accumulator half_distance and one compare !(d >= T), one __any per round.  T is exclusive: a list's k-th distance (rows ascend inside a slice,
//   so a later row AT that distance has the larger key and would be turned down), or the float above the seed, whichever is smaller; a NaN while
//   neither exists (everything passes); -inf for an absent column.
//   Hit path (wave-uniform, only when the vote is non-zero): per column block the round's distances go through a per-wavefront LDS patch,
//   transposed to [row][column] with a pitch of 20 words (the 64 stores fall into 64 banks); lane l then owns row base + l and offers its key
//   column by column (half_offer: rows past the slice and absent columns never offered, the deleted bitset read only for a key that would
//   enter), and the lane-private thresholds are refreshed from bound[].
//   Seeded thresholds: when half_seed_rows() says so, a first launch of this kernel scans a prefix of the table, merge_lists_kernel joins its
//   lists and half_seed_kernel leaves, per query, one more than the ordinal of the k-th key's distance (open if the prefix has fewer than k
//   visible rows).  The main launch covers the whole table and every slice starts from that bound: a row is a candidate iff its distance is <=
//   the seed AND it would enter its slice's list.  The prefix's k-th distance is at least the table's, and a row's distance is one value in both
//   launches, so no row of the answer is turned down.
// The per-wavefront lists go out as partial[q][slice][k]; merge_lists_kernel joins them and half_finalize_kernel writes the caller's arrays.
// HBM traffic: n * 2 d_pad bytes per query tile; matrix work: 2 * n * 16 NB * d_pad operations per tile, whatever the tile holds.
#include "kernels.hpp"

namespace eps {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// the one expression of a row's distance
__device__ __forceinline__ float half_distance(int metric, float dot, float xn, float qn) {
  if (metric == EPS_METRIC_EUCLIDEAN) {
    const float t = (xn + qn) - 2.f * dot;
    return t < 0.f ? 0.f : t;
  }
  return metric == EPS_METRIC_COSINE ? 1.f - dot : -dot;
}

// ------------------------------------------------------------------------------------------------ rounding and the stored form
__global__ __launch_bounds__(256) void half_convert_kernel(const float* x, int64_t count, int is_bf16, uint16_t* out) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step) out[i] = half_from_float_bits(__float_as_uint(x[i]), is_bf16);
}
void launch_half_convert(const float* x, int64_t count, int is_bf16, uint16_t* out, hipStream_t s) {
  if (count <= 0) return;
  const int64_t blocks = (count + 255) / 256;
  hipLaunchKernelGGL(half_convert_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, x, count, is_bf16, out);
}

__global__ __launch_bounds__(256) void half_prepare_kernel(const void* src, int src_float, int64_t m, int64_t m_pad, int64_t dim, int64_t stride, int d_pad,
                                                           int metric, int is_bf16, uint16_t* dst, float* term) {
  const int lane = lane_id();
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < m_pad; r += waves) {
    float s = 0.f;
    for (int j0 = 0; j0 < d_pad; j0 += 64) {
      const int idx = j0 + lane;
      uint16_t h = 0;
      if (r < m && idx < dim)
        h = src_float ? half_from_float_bits(__float_as_uint(static_cast<const float*>(src)[r * stride + idx]), is_bf16)
                      : static_cast<const uint16_t*>(src)[r * stride + idx];
      if (idx < d_pad) dst[r * d_pad + idx] = h;
      const float v = __uint_as_float(half_to_float_bits(h, is_bf16));
      s = fmaf(v, v, s);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0) term[r] = r < m && metric == EPS_METRIC_EUCLIDEAN ? s : 0.f;
  }
}
void launch_half_prepare(const void* src, int src_float, int64_t m, int64_t m_pad, int64_t dim, int64_t stride, int metric, int is_bf16, uint16_t* dst,
                         float* term, hipStream_t s) {
  if (m_pad <= 0) return;
  const int64_t blocks = (m_pad + 3) / 4;
  hipLaunchKernelGGL(half_prepare_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, src, src_float, m, m_pad, dim, stride,
                     (int)half_pad(dim), metric, is_bf16, dst, term);
}

// ------------------------------------------------------------------------------------------------ the scan
constexpr int half_lists(int nb, int kpl) { return HALF_LIST_BUDGET / kpl < 16 * nb ? HALF_LIST_BUDGET / kpl : 16 * nb; }   // HalfPlan::cols

// an exclusive bound on a key's high word as the float the common path compares with: a distance d can enter iff !(d >= T)
__device__ __forceinline__ float half_bound_float(u32 bound) {
  return bound > 0xFF800000u ? __uint_as_float(0x7FC00000u) : ord2f(bound);   // (above f2ord(+inf): NaN distances may enter too - everything passes)
}

// Every lane with `valid` offers its key to query q's list: the keys under the bound enter one by one (wave-uniform), and only those are judged
// against the deleted bitset.  bound[q] follows the k-th entry's distance.  Rows ascend inside a slice and lanes inside a round, so a key AT the
// bound's distance carries a larger row than every entry and is turned down by the strict compare, as the full key compare would
template <int NQ, int KPL>
__device__ __forceinline__ void half_offer(WaveTopK<KPL> (&list)[NQ], u32 (&bound)[NQ], int q, u64 key, bool valid, const uint8_t* deleted, int k) {
  u64 m = __ballot(valid && (u32)(key >> 32) < bound[q]);
  while (m) {
    const int l = __ffsll((long long)m) - 1;
    m &= m - 1;
    const u64 x = shfl64(key, l);
    const u32 row = key_id(x);
    if ((u32)(x >> 32) < bound[q] && !(deleted && ((deleted[row >> 3] >> (row & 7)) & 1))) {
      list[q].insert(x);
      const u32 kth = (u32)(list[q].entry(k - 1) >> 32);   // (no k-th entry yet: the open bound)
      bound[q] = kth < bound[q] ? kth : bound[q];
    }
  }
}

// (the 64-query form is given a SIMD's whole register file - its 128 KB tile leaves room for one workgroup per CU anyway; the others two wavefronts')
template <int NB, int KPL, bool BF16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, NB == 4 ? 1 : 2))) void half_scan_kernel(HalfScanArgs a, int64_t tile0) {
  constexpr int NQ = half_lists(NB, KPL);
  constexpr int CPB = NQ / NB;   // live columns of a column block: 16, or all NQ < 16 of the one block
  constexpr int PITCH = HALF_PATCH_PITCH;
  extern __shared__ i32x4 half_lds[];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15, kg = lane >> 4;
  const int KS = a.d_pad / HALF_KSTEP;
  i32x4* const q_s = half_lds;                                                                     // [NB][KS][64]
  float* const patch = reinterpret_cast<float*>(half_lds + NB * KS * 64) + wave * HALF_WAVE_ROWS * PITCH;   // [64][PITCH], this wavefront's
  const int64_t slice = (int64_t)blockIdx.x * HALF_BLOCK_WAVES + wave;
  const int64_t q0 = (tile0 + blockIdx.y) * NQ;
  const int nq_here = a.nq - q0 < NQ ? (int)(a.nq - q0) : NQ;   // >= 1: the grid holds no empty tile

  // ---- the tile's operands: zeros for the columns the tile does not have
  for (int i = threadIdx.x; i < NB * KS * 64; i += 256) {
    const int l = i & 63, j = (i >> 6) % KS, b = (i >> 6) / KS;
    const int qc = 16 * b + (l & 15);
    i32x4 v = {0, 0, 0, 0};
    if (qc < nq_here) v = *reinterpret_cast<const i32x4*>(a.queries + (q0 + qc) * a.d_pad + j * HALF_KSTEP + (l >> 4) * 8);
    q_s[i] = v;
  }
  __syncthreads();   // (the only barrier: from here on the wavefronts go their own ways)

  int64_t row_begin, row_end;
  half_slice_rows(a.plan.rows_per_slice, a.n, slice, &row_begin, &row_end);
  WaveTopK<KPL> list[NQ];
  u32 bound[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    list[q].init();
    bound[q] = a.seed && q < nq_here ? a.seed[q0 + q] : HALF_BOUND_OPEN;
  }
  float qn[NB], T[NB];   // this lane's columns: their norm terms and thresholds
  auto refresh = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      u32 t = HALF_BOUND_OPEN;
#pragma unroll
      for (int c = 0; c < CPB; ++c) t = col == c ? bound[16 * b + c] : t;
      if (col + 16 * b < nq_here) T[b] = half_bound_float(t);
    }
  };
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int qc = col + 16 * b;
    qn[b] = qc < nq_here ? a.query_term[q0 + qc] : 0.f;
    T[b] = __uint_as_float(0xFF800000u);   // -inf: an absent column
  }
  refresh();
  const int metric = a.metric;
  const int64_t block_elems = (int64_t)16 * a.d_pad;
  u32 hits = 0;

  for (int64_t r0 = row_begin; r0 < row_end; r0 += HALF_WAVE_ROWS) {   // (r0 + 63 < half_pad_rows(n): the table and the terms are padded to whole rounds)
    const uint16_t* const ap = a.rows + (r0 + col) * a.d_pad + kg * 8;
    f32x4 rt[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) rt[rb] = *reinterpret_cast<const f32x4*>(a.row_term + r0 + rb * 16 + 4 * kg);
    f32x4 acc[4][NB];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[rb][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](i32x4 (&x)[4], int j) __attribute__((always_inline)) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) x[rb] = *reinterpret_cast<const i32x4*>(ap + rb * block_elems + j * HALF_KSTEP);
    };
    auto mma = [&](const i32x4 (&x)[4], int j) __attribute__((always_inline)) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const i32x4 qv = q_s[(b * KS + j) * 64 + lane];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          if constexpr (BF16)
            acc[rb][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x[rb]), __builtin_bit_cast(bf16x8, qv), acc[rb][b], 0, 0, 0);
          else
            acc[rb][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, x[rb]), __builtin_bit_cast(f16x8, qv), acc[rb][b], 0, 0, 0);
        }
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

    // ---- common path: every distance against the lane's thresholds
    bool vote = false;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = half_distance(metric, acc[rb][b][i], rt[rb][i], qn[b]);
          acc[rb][b][i] = d;
          vote |= !(d >= T[b]);
        }
    if (!__any(vote)) continue;

    // ---- hit path, one column block at a time
    ++hits;
    const int64_t row = r0 + lane;
    const bool valid = row < row_end;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) patch[(rb * 16 + 4 * kg + i) * PITCH + col] = acc[rb][b][i];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (one wavefront writes and reads the patch; its LDS operations complete in order)
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < CPB; ++c) {
        if (16 * b + c < nq_here) half_offer<NQ, KPL>(list, bound, 16 * b + c, make_key(patch[lane * PITCH + c], (u32)row), valid, a.deleted, a.k);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    refresh();
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q < nq_here) list[q].store(a.partial + ((q0 + q) * a.plan.slices + slice) * a.k, a.k);   // (a slice beyond the table: an empty list)
  if (hits && lane == 0) atomicAdd(a.hit_rounds, (u64)hits);
}

template <int NB, int KPL, bool BF16>
static void launch_half_scan_t(const HalfScanArgs& a, hipStream_t s) {
  for (int64_t tile0 = 0; tile0 < a.plan.tiles; tile0 += BIN_GRID_Y) {
    const int64_t gy = a.plan.tiles - tile0 < BIN_GRID_Y ? a.plan.tiles - tile0 : BIN_GRID_Y;
    const dim3 grid((unsigned)(a.plan.slices / HALF_BLOCK_WAVES), (unsigned)gy);
    hipLaunchKernelGGL((half_scan_kernel<NB, KPL, BF16>), grid, dim3(256), (size_t)a.plan.lds_bytes, s, a, tile0);
  }
}

#define EPS_HALF_FORMS(X) X(4, 1) X(2, 1) X(1, 1) X(2, 2) X(1, 2) X(1, 4) X(1, 8) X(1, 16)

void half_scan_allow_lds() {
#define EPS_CASE(NB_, KPL_)                                                                                                                        \
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(half_scan_kernel<NB_, KPL_, false>), hipFuncAttributeMaxDynamicSharedMemorySize,        \
                            (int)half_lds_bytes(NB_, HALF_LDS_QUERY_BYTES / (32 * NB_)));                                                          \
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(half_scan_kernel<NB_, KPL_, true>), hipFuncAttributeMaxDynamicSharedMemorySize,         \
                            (int)half_lds_bytes(NB_, HALF_LDS_QUERY_BYTES / (32 * NB_)));
  EPS_HALF_FORMS(EPS_CASE)
#undef EPS_CASE
}

void launch_half_scan(const HalfScanArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
#define EPS_CASE(NB_, KPL_)                                                                                \
  if (a.plan.nb == NB_ && a.plan.kpl == KPL_)                                                              \
    return a.is_bf16 ? launch_half_scan_t<NB_, KPL_, true>(a, s) : launch_half_scan_t<NB_, KPL_, false>(a, s);
  EPS_HALF_FORMS(EPS_CASE)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------ the seed and the results
// run_keys[q][k]: the prefix's top-k.  bound[q]: one more than the ordinal of its k-th distance - ties with the seed pass - or open
__global__ __launch_bounds__(256) void half_seed_kernel(const u64* run_keys, int64_t nq, int k, u32* bound) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const u64 kth = run_keys[q * k + k - 1];
  bound[q] = kth == KEY_EMPTY ? HALF_BOUND_OPEN : (u32)(kth >> 32) + 1u;   // (a distance's ordinal is at most ORD_NAN: no wrap)
}
void launch_half_seed(const u64* run_keys, int64_t nq, int k, u32* bound, hipStream_t s) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(half_seed_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, run_keys, nq, k, bound);
}

__global__ __launch_bounds__(256) void half_finalize_kernel(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids,
                                                            float* dist, int32_t* counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const u64 key = run_keys[i];
  const bool valid = key != KEY_EMPTY;
  ids[i] = valid ? (int64_t)key_id(key) * id_stride + id_base : -1;
  dist[i] = valid ? key_dist(key) : __uint_as_float(0x7F800000u);
  if (counts && (i % k) == 0) {
    int c = 0;
    for (int e = 0; e < k; ++e) c += run_keys[i + e] != KEY_EMPTY;
    counts[i / k] = c;
  }
}
void launch_half_finalize(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids, float* dist, int32_t* counts,
                          hipStream_t s) {
  const int64_t n = nq * k;
  if (n <= 0) return;
  hipLaunchKernelGGL(half_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, run_keys, nq, k, id_base, id_stride, ids, dist, counts);
}

}  // namespace eps
