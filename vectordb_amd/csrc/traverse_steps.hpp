// What the two traversal kernels share (traverse2_kernel.hpp: the search path; traverse_kernel.hpp: the build's Link and connectivity searches):
// the queue key, the bitonic passes, the staging of a query into LDS and the exact 8-bit lower-bound test of a neighbour's mirror row - the
// kernels' arguments for it, the lane geometry and the integer dot products.  What differs stays with each kernel: how survivors are compacted,
// the edge constants, the evaluation log, the visited sets.
#pragma once
#include "graph_host.hpp"
#include "index.hpp"
#include "kernels.hpp"

namespace eps {

// ------------------------------------------------------------------------------------------------ arguments of the 8-bit test
// Exact lower-bound prefilter on the table's 8-bit mirror (mirror_build.hip: one grid per table, integer dot product, the row constant folded
// into acc0): a neighbour whose mirror row PROVES `dist > bound` is dropped without its fp32 row ever being read; every other neighbour goes
// through the unchanged fp32 evaluation.  Results are bit-identical with or without it (the proof is the flat engine's: device_common.hpp
// stage_threshold8).  x8 == null: off.
struct Prefilter8Args {
  const signed char* x8;     // [n_pad][d_pad8]
  const int* acc0;           // [n_pad]
  const float* scal8;        // the mirror's table-wide bounds (residual, |xh|, |x|^2, -, |R|)
  const signed char* q8;     // [queries of the launch][d_pad8] the queries on the same grid
  const float* qstat8;       // [queries of the launch][4] |q|^2, |q|, |q - qh|, C + c
  int d_pad8;
  int cols8;                 // leading bytes of a mirror row that carry values (Quant8View::cols8: dim, or dim rounded up to 256 in the rotated frame)
  float u8, slack8;
};

// everything but the launch's queries (q8, qstat8: set per batch); on == false: the test is off, its constants stay readable
inline Prefilter8Args prefilter8_args(const Quant8View& v, bool on, int64_t dim, bool vec4) {
  Prefilter8Args p;
  p.x8 = on ? v.x8 : nullptr;
  p.acc0 = v.acc0;
  p.scal8 = v.scal8;
  p.q8 = nullptr;
  p.qstat8 = nullptr;
  p.d_pad8 = v.d_pad8;
  p.cols8 = v.cols8;
  p.u8 = v.u;
  p.slack8 = prefilter_slack(dim, group_lanes(dim, vec4));
  return p;
}

// ------------------------------------------------------------------------------------------------ keys and their sort
// queue key: ord(dist) << 32 | id << 1 | checked (0 here), so (key >> 1) order is Candidate::operator< (candidate.hpp:16-22)
__device__ __forceinline__ u64 qkey(float d, u32 id) { return ((u64)f2ord(d + 0.0f) << 32) | ((u64)id << 1); }

// compare-exchange network passes of a bitonic sort over buf[0..n) (n a power of two) for strides
// stride_hi, stride_hi/2, ..., 1; `gbase` is the global index of buf[0], `size` the bitonic block size.
template <int NT>
__device__ __forceinline__ void bitonic_passes(u64* buf, int n, int64_t gbase, int64_t size, int stride_hi) {
  for (int stride = stride_hi; stride > 0; stride >>= 1) {
    for (int i = threadIdx.x; i < (n >> 1); i += NT) {
      const int lo = ((i / stride) * (stride << 1)) + (i % stride);
      const int hi = lo + stride;
      const bool up = (((gbase + lo) & size) == 0);
      const u64 x = buf[lo], y = buf[hi];
      if ((x > y) == up) {
        buf[lo] = y;
        buf[hi] = x;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ the query in LDS
// query q of the launch: its fp32 row padded with zeros to qstride floats and, with the prefilter, its image on the table's grid and its
// statistics (query_prep8_kernel, launched ahead of the kernel)
template <int NT>
__device__ __forceinline__ void stage_query(const float* queries, int64_t q, int dim, int qstride, float* sq, bool pf, const Prefilter8Args& p, int q8len,
                                            signed char* sq8, float* qst) {
  const int tid = threadIdx.x;
  for (int i = tid; i < qstride; i += NT) sq[i] = i < dim ? queries[q * dim + i] : 0.f;
  if (pf) {
    for (int i = tid; i < (q8len >> 2); i += NT) reinterpret_cast<u32*>(sq8)[i] = reinterpret_cast<const u32*>(p.q8 + q * p.d_pad8)[i];
    if (tid < 4) qst[tid] = p.qstat8[q * 4 + tid];
  }
}

// ------------------------------------------------------------------------------------------------ the 8-bit dot products
// lanes per mirror row: every lane holds NL8 pieces of 16 bytes of it
__device__ __forceinline__ int lanes_per_row8(int q8len, int NL8) {
  int G8 = 4;
  while (G8 < 64 && G8 * 16 * NL8 < q8len) G8 <<= 1;
  return G8;
}

// dot[u] = the integer dot product of mirror row rp8[u] with the staged query sq8, over q8len bytes, in every lane of the row's group (t8 = this
// lane's place in it).  G8 lanes per row, every lane NL8 16-byte pieces of it 16*G8 bytes apart (one instruction covers 16*G8 contiguous bytes
// of each of its 64/G8 rows); U8 rows per lane group: U8*NL8 loads in flight per lane, 64/G8*U8 rows per wavefront and pass.
template <int U8, int NL8>
__device__ __forceinline__ void mirror_dots(const signed char* const (&rp8)[U8], const signed char* sq8, int q8len, int G8, int t8, int (&dot)[U8]) {
#pragma unroll
  for (int u = 0; u < U8; ++u) dot[u] = 0;
#pragma unroll 1
  for (int c = t8 * 16; c < q8len; c += G8 * 16 * NL8) {
    i32x4 xv[U8][NL8];
#pragma unroll
    for (int j = 0; j < NL8; ++j) {
      const int cj = c + j * G8 * 16;
      const bool in = cj < q8len;
#pragma unroll
      for (int u = 0; u < U8; ++u) xv[u][j] = in ? *reinterpret_cast<const i32x4*>(rp8[u] + cj) : i32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < NL8; ++j) {
      const int cj = c + j * G8 * 16;
      const i32x4 qv = cj < q8len ? *reinterpret_cast<const i32x4*>(sq8 + cj) : i32x4{0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < U8; ++u) {
        dot[u] = __builtin_amdgcn_sdot4(xv[u][j][0], qv[0], dot[u], false);
        dot[u] = __builtin_amdgcn_sdot4(xv[u][j][1], qv[1], dot[u], false);
        dot[u] = __builtin_amdgcn_sdot4(xv[u][j][2], qv[2], dot[u], false);
        dot[u] = __builtin_amdgcn_sdot4(xv[u][j][3], qv[3], dot[u], false);
      }
    }
  }
  if (G8 == 16) {   // (one DPP row per mirror row - d in (512, 768]: 4 VALU instructions per sum instead of 4 LDS-crossbar round trips; integer sums, any order)
#pragma unroll
    for (int u = 0; u < U8; ++u) dot[u] = row16_sum(dot[u]);
  } else {
    for (int o = G8 >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int u = 0; u < U8; ++u) dot[u] += __shfl_xor(dot[u], o);
    }
  }
}

}  // namespace eps
