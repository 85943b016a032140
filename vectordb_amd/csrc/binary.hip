// Binary-vector fields (eps_binary_index_*): the exact Hamming scan of a table of packed bits.  distance(row, query) = popcount((row ^ query) &
// mask_dim): small integers, so every answer is exact and full of ties; a key is (distance << 32 | row), ties go to the smaller row.
//
// binary_scan_kernel<NQ, KPL>: one lane owns one row; a wavefront takes 64 consecutive rows per round and walks its slice of the table round by
// round.  The row's words are stationary in registers, BIN_CW = 8 at a time (two 16-byte loads per lane, straight from the table: the lanes of a
// round read neighbouring rows, so the lines of one chunk are the lines of the next three and stay in the vector cache; the next chunk is
// requested before this one is used).  The tile's NQ queries are the same for every lane: their words are read with wave-uniform addresses from a
// table no launch of this call writes, which the compiler turns into scalar loads - a query word is an SGPR operand of the XOR.  One (row, query)
// word costs two vector instructions: v_xor_b32, then v_bcnt_u32_b32 with the pair's running count as its addend; NQ counts per lane.  Only the
// chunk that holds word W - 1 knows of the tail mask: the row's word is masked once per round, the query's word on the scalar unit.  After the
// last chunk every lane offers its NQ keys to the wavefront's lists (device_common.hpp's offer: only a key that would enter a list is judged
// against the deleted bitset).  A tile that is not full skips its absent queries (a wave-uniform branch).
//
// The per-wavefront lists go out as partial[q][slice][k]; flat_kernels.hip's merge_lists_kernel joins them and binary_finalize_kernel writes the
// caller's arrays.  HBM traffic: n * W * 4 bytes per query tile; arithmetic: 2 * W lane instructions per pair (binary_host.hpp has the plan).
#include "kernels.hpp"

namespace eps {

// population count of v plus acc in ONE instruction.  Written out: left to itself the compiler re-associates a chain of popcount + add into
// v_bcnt_u32_b32 with a zero addend and a v_add3_u32 per two words - 2.5 instructions per word where the chain costs 2.
__device__ __forceinline__ u32 bcnt_add(u32 v, u32 acc) {
  u32 r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(acc));
  return r;
}
// words [w0, w0 + BIN_CW) of the row at `rp`, all of them inside the row.  VEC: two 16-byte loads
template <bool VEC>
__device__ __forceinline__ void binary_load_whole(const u32* rp, int w0, u32 (&x)[BIN_CW]) {
  if (VEC) {
    const uint4 lo = *reinterpret_cast<const uint4*>(rp + w0), hi = *reinterpret_cast<const uint4*>(rp + w0 + 4);
    x[0] = lo.x, x[1] = lo.y, x[2] = lo.z, x[3] = lo.w;
    x[4] = hi.x, x[5] = hi.y, x[6] = hi.z, x[7] = hi.w;
  } else {
#pragma unroll
    for (int j = 0; j < BIN_CW; ++j) x[j] = rp[w0 + j];
  }
}
// the chunk that holds word W - 1: zeros behind that word, the word itself masked.  A 16-byte piece is read only where all four of its words
// belong to the row: the last row of a table ends with its W-th word.  Everything but `rp` is wave-uniform.
template <bool VEC>
__device__ __forceinline__ void binary_load_tail(const u32* rp, int w0, int W, u32 mask, u32 (&x)[BIN_CW]) {
#pragma unroll
  for (int g = 0; g < BIN_CW; g += 4) {
    if (VEC && w0 + g + 4 <= W) {
      const uint4 v = *reinterpret_cast<const uint4*>(rp + w0 + g);
      x[g] = v.x, x[g + 1] = v.y, x[g + 2] = v.z, x[g + 3] = v.w;
    } else {
#pragma unroll
      for (int j = g; j < g + 4; ++j) x[j] = w0 + j < W ? rp[w0 + j] : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < BIN_CW; ++j) x[j] &= w0 + j == W - 1 ? mask : 0xFFFFFFFFu;
}
// acc[q] += popcount(x ^ words [w0, w0 + BIN_CW) of query q), for the queries the tile has.  `qbase` is wave-uniform: the query words are
// scalar loads and SGPR operands.  FULL: all NQ queries are there and nothing branches.
template <int NQ, bool FULL>
__device__ __forceinline__ void binary_chunk(const u32 (&x)[BIN_CW], const u32* __restrict__ qbase, int W, int w0, int nq_here, u32 (&acc)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (FULL || q < nq_here) {
      const u32* __restrict__ const qp = qbase + (int64_t)q * W + w0;
#pragma unroll
      for (int j = 0; j < BIN_CW; ++j) acc[q] = bcnt_add(x[j] ^ qp[j], acc[q]);
    }
  }
}
// the Hamming distances of one row to the tile's queries: whole chunks with the next one requested before this one is used, then the chunk of
// the last word, where the words behind W - 1 count as zero on both sides and the last word is masked on both sides
template <int NQ, bool VEC, bool FULL>
__device__ __forceinline__ void binary_row(const u32* __restrict__ rp, const u32* __restrict__ qbase, int W, u32 mask, int nq_here, u32 (&acc)[NQ]) {
  const int tail0 = (W - 1) / BIN_CW * BIN_CW;   // first word of the chunk that holds word W - 1; the chunks in front of it are whole
  u32 x[BIN_CW], xn[BIN_CW];
  if (tail0 > 0) {
    binary_load_whole<VEC>(rp, 0, x);
    for (int w0 = 0; w0 + BIN_CW < tail0; w0 += BIN_CW) {
      binary_load_whole<VEC>(rp, w0 + BIN_CW, xn);
      binary_chunk<NQ, FULL>(x, qbase, W, w0, nq_here, acc);
#pragma unroll
      for (int j = 0; j < BIN_CW; ++j) x[j] = xn[j];
    }
    binary_load_tail<VEC>(rp, tail0, W, mask, xn);
    binary_chunk<NQ, FULL>(x, qbase, W, tail0 - BIN_CW, nq_here, acc);
#pragma unroll
    for (int j = 0; j < BIN_CW; ++j) x[j] = xn[j];
  } else {
    binary_load_tail<VEC>(rp, 0, W, mask, x);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (FULL || q < nq_here) {
      const u32* __restrict__ const qp = qbase + (int64_t)q * W + tail0;
#pragma unroll
      for (int j = 0; j < BIN_CW; ++j) {
        if (tail0 + j < W) {
          const u32 qw = tail0 + j == W - 1 ? qp[j] & mask : qp[j];
          acc[q] = bcnt_add(x[j] ^ qw, acc[q]);
        }
      }
    }
  }
}

// (the forms with 64 list registers and more are given the whole register file of a SIMD's two wavefronts: no scratch)
template <int NQ, int KPL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, (NQ * KPL >= 32 ? 2 : 8)))) void binary_scan_kernel(BinaryScanArgs a, int64_t tile0) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int W = a.W;
  const int vec = a.vec;
  const int64_t slice = (int64_t)blockIdx.x * BIN_BLOCK_WAVES + wave;
  const int64_t q0 = (tile0 + blockIdx.y) * NQ;
  const int nq_here = a.nq - q0 < NQ ? (int)(a.nq - q0) : NQ;   // >= 1: the grid holds no empty tile
  const u32* __restrict__ const qbase = a.queries + q0 * W;
  int64_t row_begin, row_end;
  binary_slice_rows(a.plan, a.n, slice, &row_begin, &row_end);

  FilterSpec f = no_filter();   // (built here: the compiler sees that nothing but the bitset is ever asked)
  f.deleted = a.deleted;
  WaveTopK<KPL> list[NQ];
  u64 thr[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    list[q].init();
    thr[q] = KEY_EMPTY;
  }
  for (int64_t r0 = row_begin; r0 < row_end; r0 += BIN_WAVE_ROWS) {
    const int64_t r = r0 + lane;
    const bool valid = r < row_end;
    const int64_t rr = valid ? r : r0;
    const u32* __restrict__ const rp = a.rows + rr * a.stride;
    u32 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0u;
    if (nq_here == NQ) {
      if (vec) binary_row<NQ, true, true>(rp, qbase, W, a.tail_mask, NQ, acc);
      else binary_row<NQ, false, true>(rp, qbase, W, a.tail_mask, NQ, acc);
    } else {
      if (vec) binary_row<NQ, true, false>(rp, qbase, W, a.tail_mask, nq_here, acc);
      else binary_row<NQ, false, false>(rp, qbase, W, a.tail_mask, nq_here, acc);
    }
    // the wavefront's lists
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const u64 key = ((u64)acc[q] << 32) | (u64)(u32)rr;
      offer<NQ, KPL>(list, thr, q, key, valid && q < nq_here, f, a.k, false);
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q < nq_here) list[q].store(a.partial + ((q0 + q) * a.plan.slices + slice) * a.k, a.k);   // (a slice beyond the table: an empty list)
}

template <int NQ, int KPL>
static void launch_binary_scan_t(const BinaryScanArgs& a, hipStream_t s) {
  for (int64_t tile0 = 0; tile0 < a.plan.tiles; tile0 += BIN_GRID_Y) {
    const int64_t gy = a.plan.tiles - tile0 < BIN_GRID_Y ? a.plan.tiles - tile0 : BIN_GRID_Y;
    const dim3 grid((unsigned)(a.plan.slices / BIN_BLOCK_WAVES), (unsigned)gy);
    hipLaunchKernelGGL((binary_scan_kernel<NQ, KPL>), grid, dim3(256), 0, s, a, tile0);
  }
}

void launch_binary_scan(const BinaryScanArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n <= 0) return;
  const int kpl = a.plan.kpl, nq = a.plan.nq_tile;
#define EPS_CASE(NQ_, KPL_) \
  if (nq == NQ_ && kpl == KPL_) return launch_binary_scan_t<NQ_, KPL_>(a, s);
  EPS_CASE(4, 1) EPS_CASE(8, 1) EPS_CASE(16, 1) EPS_CASE(32, 1)
  EPS_CASE(4, 2) EPS_CASE(8, 2) EPS_CASE(16, 2)
  EPS_CASE(4, 4) EPS_CASE(8, 4)
  EPS_CASE(4, 8) EPS_CASE(4, 16)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------ results
__global__ __launch_bounds__(256) void binary_finalize_kernel(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids,
                                                              int32_t* dist, int32_t* counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const u64 key = run_keys[i];
  const bool valid = key != KEY_EMPTY;
  ids[i] = valid ? (int64_t)key_id(key) * id_stride + id_base : -1;
  dist[i] = valid ? (int32_t)(key >> 32) : 2147483647;
  if (counts && (i % k) == 0) {
    int c = 0;
    for (int e = 0; e < k; ++e) c += run_keys[i + e] != KEY_EMPTY;
    counts[i / k] = c;
  }
}
void launch_binary_finalize(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids, int32_t* dist, int32_t* counts,
                            hipStream_t s) {
  const int64_t n = nq * k;
  if (n <= 0) return;
  hipLaunchKernelGGL(binary_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, run_keys, nq, k, id_base, id_stride, ids, dist, counts);
}

// ------------------------------------------------------------------------------------------------ signs -> bits
// One wavefront per row (grid-stride).  It reads 64 consecutive floats of the row; __ballot(x > 0.0f) is two words of the row (NaN, -0 and +0
// vote 0, and so do the lanes past dim).  The ballots of up to 32 such reads are 64 words: lane l keeps word l, and they leave as one coalesced
// store.
__global__ __launch_bounds__(256) void binary_pack_kernel(const float* x, int64_t m, int64_t dim, u32* words, int64_t stride) {
  const int lane = lane_id();
  const int64_t W = binary_words(dim);
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < m; r += waves) {
    const float* xr = x + r * dim;
    u32* wr = words + r * stride;
    for (int64_t wbase = 0; wbase < W; wbase += 64) {
      u32 mine = 0u;
#pragma unroll 4
      for (int s = 0; s < 32; ++s) {
        const int64_t c = (wbase + 2 * s) * 32 + lane;   // wave-uniform but for the lane
        if ((wbase + 2 * s) * 32 >= dim) break;
        const float v = c < dim ? xr[c] : 0.0f;
        const u64 b = __ballot(v > 0.0f);
        if (lane == 2 * s) mine = (u32)b;
        if (lane == 2 * s + 1) mine = (u32)(b >> 32);
      }
      if (wbase + lane < W) wr[wbase + lane] = mine;
    }
  }
}
void launch_binary_pack(const float* x, int64_t m, int64_t dim, u32* words, int64_t stride, hipStream_t s) {
  if (m <= 0) return;
  const int64_t blocks = (m + 3) / 4;
  hipLaunchKernelGGL(binary_pack_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, x, m, dim, words, stride);
}

}  // namespace eps
