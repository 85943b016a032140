// The mirrors of the row store (mirror.hpp): the fp16 mirror with its per-row bounds, the 8-bit mirror with its grid, centre and frame, the query
// preparation on that grid, and the view the traversal and the graph build get.  The bounds all of it serves: top of mfma_filter.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mirror.hpp"

namespace eps {

void half_mirror_free(HalfMirror* m) { delete m; }

// ------------------------------------------------------------------------------------------------ mirror build
__device__ __forceinline__ void atomic_max_pos(float* addr, float v) {  // v >= 0
  atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

// rows [row0, n_pad) are (re)written: row0 = 0 builds the mirror, row0 = rows mirrored so far extends it after an append
// (the per-index maxima in `scal` only ever grow, so they are accumulated across calls)
__global__ __launch_bounds__(256) void half_mirror_kernel(const float* rows, int64_t row0, int64_t n, int64_t n_pad, int dim, int d_pad,
                                                          _Float16* xh, float* xn, float* zeros, float* xn_s, float* zeros_s, float* scal,
                                                          float gamma) {
  // one wavefront per row, grid-stride over rows; the four per-index maxima are reduced in registers and
  // published with ONE atomic per wavefront (an atomic per row serialises 10M rows on four addresses)
  const int lane = lane_id();
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  float m_e1 = 0.f, m_nxh = 0.f, m_xn = 0.f, m_bad = 0.f;
  const bool vec = (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(rows) & 15) == 0);
  typedef _Float16 half4 __attribute__((ext_vector_type(4)));
  for (int64_t r = row0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_pad; r += nwaves) {
    _Float16* dst = xh + r * d_pad;
    if (r >= n) {
      for (int c = lane; c < d_pad; c += 64) dst[c] = (_Float16)0.f;
      if (lane == 0) {
        xn[r] = __builtin_inff();
        zeros[r] = __builtin_inff();
        xn_s[r] = -__builtin_inff();
        zeros_s[r] = -__builtin_inff();
      }
      continue;
    }
    const float* src = rows + r * dim;
    float s2 = 0.f, e2 = 0.f, h2 = 0.f, mx = 0.f;
    if (vec) {  // 16 B/lane loads, 8 B/lane stores (d_pad is a multiple of 64, so c + 3 < d_pad)
      for (int c = lane * 4; c < d_pad; c += 256) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < dim) x = *reinterpret_cast<const float4*>(src + c);
        half4 h;
        h[0] = (_Float16)x.x; h[1] = (_Float16)x.y; h[2] = (_Float16)x.z; h[3] = (_Float16)x.w;
        *reinterpret_cast<half4*>(dst + c) = h;
        const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float hf = (float)h[e];
          s2 = fmaf(xs[e], xs[e], s2);
          const float er = xs[e] - hf;
          e2 = fmaf(er, er, e2);
          h2 = fmaf(hf, hf, h2);
          mx = fmaxf(mx, fabsf(xs[e]));
        }
      }
    } else {
      for (int c = lane; c < d_pad; c += 64) {
        const float x = c < dim ? src[c] : 0.f;
        const _Float16 h = (_Float16)x;
        const float hf = (float)h;
        dst[c] = h;
        s2 = fmaf(x, x, s2);
        const float e = x - hf;
        e2 = fmaf(e, e, e2);
        h2 = fmaf(hf, hf, h2);
        mx = fmaxf(mx, fabsf(x));
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      s2 += __shfl_xor(s2, o);
      e2 += __shfl_xor(e2, o);
      h2 += __shfl_xor(h2, o);
      mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (lane == 0) {
      xn[r] = s2;
      zeros[r] = 0.f;
      xn_s[r] = -0.5f * s2;
      zeros_s[r] = 0.f;
    }
    const float nxh = sqrtf(h2) * 1.000001f;
    m_e1 = fmaxf(m_e1, sqrtf(e2) * 1.000001f + gamma * nxh);
    m_nxh = fmaxf(m_nxh, nxh);
    m_xn = fmaxf(m_xn, s2);
    if (!(mx <= 65504.f) || s2 != s2) m_bad = 1.f;  // beyond the fp16 range, or NaN
  }
  if (lane == 0) {
    atomic_max_pos(&scal[0], m_e1);
    atomic_max_pos(&scal[1], m_nxh);
    atomic_max_pos(&scal[2], m_xn);
    if (m_bad != 0.f) atomic_max_pos(&scal[3], 1.f);
  }
}


// ------------------------------------------------------------------------------------------------ 8-bit mirror
// r4: the grid is CENTRED.  Rows and queries are quantised as x' = x - mu on a symmetric grid, xh' = step * xi, with one mu per
// COLUMN (column means of a strided sample of the table + the mid-range of what is left, so that the grid is symmetric).  Distances
// do not care: |x - q|^2 = |x' - q'|^2, q.x = q'.x' + mu.x' + q.mu - the cross terms are a per-row and a per-query constant, exact in
// fp32, folded into R[x] and C[q] - and the Cauchy-Schwarz margin now scales with |q - mu| and |x - mu| instead of |q| and |x|:
// half the margin on U[0,1) rows (every candidate the filter passes for nothing costs a 3 KB gather in the re-rank, an fp32 row in
// the traversal), a third on tables whose columns have their own means, and tables far from the origin lose nothing.  ANY mu keeps
// the bound valid (tests/test_bound_math.py::test_any_centre_keeps_the_bound_valid): it only has to be the same vector for the rows
// and the queries, so it is fixed when the mirror is first built and kept when rows are appended.
constexpr int CENTRE_SEG = 32;   // segments of the sample, summed in a fixed order: mu is bit-reproducible (the build's approximate
                                 // kNN keys depend on it, and two builds of one table must give the same graph)
// partial column sums of sample rows r = (seg * per_seg + i) * stride, i < per_seg:  part[seg][col]
// (clamp_mean != null: every value is clamped into [clamp_mean[col] + clo, clamp_mean[col] + chi] first - the second, ROBUST estimate of the
// column means: an outlier of 30 000 in a 65 536-row sample would otherwise move its column's centre by half the grid)
__global__ __launch_bounds__(256) void colsum_kernel(const float* rows, int64_t n, int dim, int64_t stride, int64_t per_seg, float* part, const float* clamp_mean,
                                                     float clo, float chi) {
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int sub = threadIdx.x >> 6;
  const int64_t seg = blockIdx.y;
  float s = 0.f;
  if (col < dim) {
    for (int64_t i = sub; i < per_seg; i += 4) {
      const int64_t r = (seg * per_seg + i) * stride;
      if (r < n) {
        float v = rows[r * dim + col];
        if (clamp_mean) v = fminf(fmaxf(v, clamp_mean[col] + clo), clamp_mean[col] + chi);
        s += v;
      }
    }
  }
  red[sub][threadIdx.x & 63] = s;
  __syncthreads();
  if (sub == 0 && col < dim) part[seg * dim + col] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// mean[col] = sum of the segments (fixed order) / sampled rows; columns beyond dim: 0
__global__ void colmean_kernel(const float* part, int dim, int d_pad8, float inv_count, float* mu) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= d_pad8) return;
  float s = 0.f;
  if (col < dim)
    for (int g = 0; g < CENTRE_SEG; ++g) s += part[g * dim + col];
  mu[col] = col < dim ? s * inv_count : 0.f;
}
// value range of x - mean over the whole table (ordered-u32 images, so atomicMin / atomicMax work on them): scal8[6] = min,
// scal8[7] = max; one wavefront per row, grid-stride
template <bool ROT>
__global__ __launch_bounds__(256) void minmax_kernel(const float* rows, int64_t n, int dim, const float* mean, u32* scal8, const int* sp, int d_pad8) {
  float lo = __builtin_inff(), hi = -__builtin_inff();
  bool bad = false;
  const int lane = lane_id();
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const bool vec = (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(rows) & 15) == 0);
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += nwaves) {
    const float* src = rows + r * dim;
    if (ROT) {   // the rotated frame (device_common.hpp, rot256_load): d_pad8 here = the rotation's width
      for (int c = lane * 4; c < d_pad8; c += 256) {
        double xd[4];
        rot256_load(src, dim, sp, c, lane, xd);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = (float)(xd[e] - (double)mean[c + e]);
          lo = fminf(lo, a);
          hi = fmaxf(hi, a);
          bad |= !(fabsf(a) < 3.0e38f);
        }
      }
    } else if (vec) {
      for (int c = lane * 4; c < dim; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c);
        const float4 m = *reinterpret_cast<const float4*>(mean + c);
        const float a = v.x - m.x, b = v.y - m.y, c2 = v.z - m.z, d2 = v.w - m.w;
        lo = fminf(fminf(lo, a), fminf(fminf(b, c2), d2));
        hi = fmaxf(fmaxf(hi, a), fmaxf(fmaxf(b, c2), d2));
        bad |= !(fabsf(v.x) < 3.0e38f) || !(fabsf(v.y) < 3.0e38f) || !(fabsf(v.z) < 3.0e38f) || !(fabsf(v.w) < 3.0e38f);
      }
    } else {
      for (int c = lane; c < dim; c += 64) {
        const float a = src[c] - mean[c];
        lo = fminf(lo, a);
        hi = fmaxf(hi, a);
        bad |= !(fabsf(src[c]) < 3.0e38f);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if (lane == 0) {
    if (lo <= hi) {
      atomicMin(&scal8[6], f2ord(lo + 0.0f));
      atomicMax(&scal8[7], f2ord(hi + 0.0f));
    }
  }
  if (__any(bad) && lane == 0) atomicMax(&scal8[3], __float_as_uint(1.f));   // inf / NaN somewhere: the grid would be meaningless
}
// mu = mean + z0 (z0: mid-range of x - mean, so that the grid is symmetric around 0); scal8[5] = |mu| (enters the fp32 slack of IP / COSINE)
__global__ __launch_bounds__(64) void mu_finish_kernel(float* mu, int dim, float z0, float* scal8) {
  float s2 = 0.f;
  for (int c = lane_id(); c < dim; c += 64) {
    const float v = mu[c] + z0;
    mu[c] = v;
    s2 = fmaf(v, v, s2);
  }
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
  if (lane_id() == 0) scal8[5] = sqrtf(s2) * 1.00001f;
}

// r4: the grid's range is set by the BULK of the values: 4096-bin histogram of x - mean over the sample rows (integer atomics: the
// result does not depend on the order), the host cuts both tails at max(2, 1e-7 x values) sample values.  One outlier value used to
// stretch the grid - and with it every row's margin - by its distance; now its row is clamped and pays with ITS OWN residual.
__global__ __launch_bounds__(256) void centre_hist_kernel(const float* rows, int64_t n, int dim, int64_t stride, int64_t sampled, const float* mean, float lo,
                                                          float inv_binw, u32* hist) {
  __shared__ u32 h[4096];
  for (int i = threadIdx.x; i < 4096; i += 256) h[i] = 0;
  __syncthreads();
  for (int64_t j = blockIdx.x; j < sampled; j += gridDim.x) {
    const int64_t r = j * stride;
    if (r >= n) break;
    const float* src = rows + r * dim;
    for (int c = threadIdx.x; c < dim; c += 256) {
      int b = (int)((src[c] - mean[c] - lo) * inv_binw);
      b = b < 0 ? 0 : (b > 4095 ? 4095 : b);
      atomicAdd(&h[b], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4096; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}
// the rotated frame's column statistics (means, histogram) come from the same kernels, run over the rotated images of the sample rows:
// out[j][0 .. d_pad8) = R rows[j * stride], fp32 (statistics only: any centre and any step keep the bound valid)
__global__ __launch_bounds__(256) void rot_sample_kernel(const float* rows, int64_t n, int dim, int64_t stride, int64_t sampled, int d_pad8, const int* sp, float* out) {
  const int lane = lane_id();
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < sampled; j += (int64_t)gridDim.x * 4) {
    const int64_t r = j * stride;
    if (r >= n) break;
    for (int c = lane * 4; c < d_pad8; c += 256) {
      double xd[4];
      rot256_load(rows + r * dim, dim, sp, c, lane, xd);
      *reinterpret_cast<float4*>(out + j * d_pad8 + c) = make_float4((float)xd[0], (float)xd[1], (float)xd[2], (float)xd[3]);
    }
  }
}
constexpr int ACC_FORCE = 0x38000000;   // start value of a row that must pass whatever the threshold (thresholds <= TQ_MAX8, |dot| < 2^27)
// the batch's margins folded into the rows' start values: acc0b[x] = acc0[x] + ceil(|s| (Qn E[x] + Eq H[x]) / u) + 1, Qn / Eq = the batch's
// largest |q'| / |q' - qh'| (>= every query's own margin for row x); forced rows and rows whose margin leaves the range: ACC_FORCE
__global__ __launch_bounds__(256) void fold8_kernel(const int* acc0, const float* erow, const float* hrow, int64_t n, int64_t n_pad, const u32* qmax, float s_abs,
                                                    float inv_u, int* acc0b) {
  const float qn = __uint_as_float(qmax[0]), eq = __uint_as_float(qmax[1]);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += (int64_t)gridDim.x * 256) {
    int v = acc0[r];
    if (r < n) {
      const float add = ceilf(s_abs * (qn * erow[r] + eq * hrow[r]) * inv_u) + 1.f;
      v = add < 536870912.f ? v + (int)add : ACC_FORCE;   // (erow = +inf, or a NaN: forced)
    }
    acc0b[r] = v;
  }
}
// after (re)quantising: scal8[6] = max |x'| bound (for the thresholds' fp32 slack); scal8f = scal8 with the two margin entries zeroed
__global__ void scal_finish_kernel(float* scal8, float* scal8f) {
  if (threadIdx.x == 0) scal8[6] = scal8[0] + scal8[1];
  __syncthreads();
  if (threadIdx.x < 8) scal8f[threadIdx.x] = threadIdx.x < 2 ? 0.f : scal8[threadIdx.x];
}

// rows [row0, n_pad) are (re)written, as in half_mirror_kernel.  x' = x - mu;  metric 0: R = |x'|^2; otherwise R = -mu.x'.  u = |s| step^2.
// ROT: the table's rotated frame (device_common.hpp, rot256_load) - x' = fl32(R x - mu); the first rot_w = ceil(dim / 256) * 256 columns carry values
template <bool ROT>
__global__ __launch_bounds__(256) void quant_mirror_kernel(const float* rows, int64_t row0, int64_t n, int64_t n_pad, int dim, int d_pad8, const float* mu, float step,
                                                           float inv_step, float inv_u, int metric, signed char* x8, int* acc0, float* scal8, float* erow,
                                                           float* hrow, u32* forced_count, const int* sp, int rot_w) {
  const int lane = lane_id();
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  float m_e1 = 0.f, m_nxh = 0.f, m_xn = 0.f, m_bad = 0.f, m_r = 0.f, m_emin = __builtin_inff();
  const bool vec = (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(rows) & 15) == 0);
  for (int64_t r = row0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_pad; r += nwaves) {
    signed char* dst = x8 + r * d_pad8;
    if (r >= n) {
      for (int c = lane * 4; c < d_pad8; c += 256) *reinterpret_cast<u32*>(dst + c) = 0u;
      if (lane == 0) {
        acc0[r] = -(1 << 30);
        erow[r] = 0.f;
        hrow[r] = 0.f;
      }
      continue;
    }
    const float* src = rows + r * dim;
    float s2 = 0.f, e2 = 0.f, h2 = 0.f, c2 = 0.f, mx = 0.f;
    for (int c = lane * 4; c < d_pad8; c += 256) {   // d_pad8 is a multiple of 256
      float xs[4] = {0.f, 0.f, 0.f, 0.f};
      double xd[4] = {0.0, 0.0, 0.0, 0.0};
      if (ROT) {
        if (c < rot_w) rot256_load(src, dim, sp, c, lane, xd);   // (columns [rot_w, d_pad8): padding, zero codes)
#pragma unroll
        for (int e = 0; e < 4; ++e) xs[e] = (float)xd[e];   // (enters |x|^2 only: a slack scale)
      } else if (vec) {
        if (c < dim) {
          const float4 v = *reinterpret_cast<const float4*>(src + c);
          xs[0] = v.x; xs[1] = v.y; xs[2] = v.z; xs[3] = v.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xs[e] = c + e < dim ? src[c + e] : 0.f;
      }
      const float4 mv = *reinterpret_cast<const float4*>(mu + c);   // (mu has d_pad8 entries, zeros beyond dim)
      const float ms[4] = {mv.x, mv.y, mv.z, mv.w};
      u32 packed = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (ROT ? c < rot_w : c + e < dim) {
          const float dx = ROT ? (float)(xd[e] - (double)ms[e]) : xs[e] - ms[e];   // x' (one rounding in either frame)
          const int xi = quant8(dx, 0.f, inv_step);
          const float res = fmaf(-step, (float)xi, dx);     // x' - xh'
          const float xh = step * (float)xi;
          packed |= (u32)(xi & 255) << (8 * e);
          s2 = fmaf(xs[e], xs[e], s2);
          e2 = fmaf(res, res, e2);
          h2 = fmaf(xh, xh, h2);
          c2 = fmaf(dx, dx, c2);
          mx = fmaf(ms[e], dx, mx);
        }
      }
      *reinterpret_cast<u32*>(dst + c) = packed;
    }
    for (int o = 32; o > 0; o >>= 1) {
      s2 += __shfl_xor(s2, o);
      e2 += __shfl_xor(e2, o);
      h2 += __shfl_xor(h2, o);
      c2 += __shfl_xor(c2, o);
      mx += __shfl_xor(mx, o);
    }
    const float R = metric == 0 ? c2 : -mx;
    const float a0 = ceilf(-R * inv_u) + 1.f;
    const float e1 = sqrtf(e2) * 1.00001f + 1.2e-7f * sqrtf(c2) + (ROT ? 1e-12f * sqrtf(s2) : 0.f);   // (+ the rounding of x - mu itself; ROT: + the fp64 transform's)
    const float nxh = sqrtf(h2) * 1.00001f;
    if (s2 != s2 || !(s2 < 3.0e38f)) m_bad = 1.f;
    // |acc0| must stay below 2^29 (the dot product adds < 2^27).  A row beyond that - an outlier far outside the clipped grid - is FORCED:
    // never selected on approximate keys (acc0 = -2^30, as on padding rows), always passed by the exact filter (erow = +inf -> fold8_kernel
    // gives it ACC_FORCE); it does not enter the table's maxima (they only serve rows that are tested)
    const bool forced = !(fabsf(a0) < 536870912.f);
    if (lane == 0) {
      acc0[r] = forced ? -(1 << 30) : (int)a0;
      erow[r] = forced ? __builtin_inff() : e1;
      hrow[r] = nxh;
      if (forced) atomicAdd(forced_count, 1u);
    }
    if (forced) continue;
    m_emin = fminf(m_emin, e1);
    m_e1 = fmaxf(m_e1, e1);
    m_nxh = fmaxf(m_nxh, nxh);
    m_xn = fmaxf(m_xn, s2);
    m_r = fmaxf(m_r, fabsf(R));
  }
  if (lane == 0) {
    atomic_max_pos(&scal8[0], m_e1);
    atomic_max_pos(&scal8[1], m_nxh);
    atomic_max_pos(&scal8[2], m_xn);
    if (m_bad != 0.f) atomic_max_pos(&scal8[3], 1.f);
    atomic_max_pos(&scal8[4], m_r);
    atomicMin(reinterpret_cast<unsigned int*>(&scal8[7]), __float_as_uint(m_emin));   // (smallest residual norm of a tested row: non-negative floats order like their bits)
  }
}

template <bool ROT>
__global__ __launch_bounds__(256) void query_prep8_kernel(const float* q, int64_t nq, int64_t b_pad, int dim, int d_pad8, const float* mu, float step, float inv_step,
                                                          int metric, signed char* q8, float* qstat, Prep8Extra x, const int* sp, int rot_w) {
  if (blockIdx.x == 0) {   // the seeded call's start state (nothing in this launch reads it)
    for (int64_t i = threadIdx.x; x.T2 && i < x.n2; i += 256) x.T2[i] = x.Tv;
    for (int64_t i = threadIdx.x; x.cnt && i < (x.s8g ? S8_MAX_Q + 8 : nq + 8); i += 256) x.cnt[i] = i < nq ? x.cntv : 0u;
    if (x.gsync) x.gsync[threadIdx.x] = 0;
    if (x.s8g) {   // (the slots of the call's queries - at least of the first four: a later call of 1-2 queries that skips this launch relies on its own
                   // slots being empty, and the re-rank of every call restores exactly the slots it used - and S8_MAX_Q + 8 counter words)
      const int qinit = nq > 4 ? (int)nq : 4;
      for (int i = threadIdx.x; i < qinit * x.s8_slots; i += 256) x.s8g[i * S8_SLOT_STRIDE] = S8_EMPTY;
    }
  }
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= b_pad) return;
  const int lane = lane_id();
  signed char* dst = q8 + r * d_pad8;
  // where byte column c of row r lives in the fragment-major copy
  const int64_t fbase = x.qf ? ((r >> 5) * (int64_t)(d_pad8 >> 5)) * 1024 + (r & 31) * 16 : 0;
  // ... and in the 16x16x64 copy: lane = query % 16 + 16 * (16-byte quarter of the K = 64 piece)
  const int64_t fbase16 = x.qf16 ? ((r >> 4) * (int64_t)(d_pad8 >> 6)) * 1024 + (r & 15) * 16 : 0;
  auto fput = [&](int c, u32 v) {
    if (x.qf) *reinterpret_cast<u32*>(x.qf + fbase + (int64_t)(c >> 5) * 1024 + ((c >> 4) & 1) * 512 + (c & 15)) = v;
    if (x.qf16) *reinterpret_cast<u32*>(x.qf16 + fbase16 + (int64_t)(c >> 6) * 1024 + ((c >> 4) & 3) * 256 + (c & 15)) = v;
  };
  if (r >= nq) {
    for (int c = lane * 4; c < d_pad8; c += 256) {
      *reinterpret_cast<u32*>(dst + c) = 0u;
      fput(c, 0u);
    }
    if (lane == 0) qstat[r * 4 + 0] = qstat[r * 4 + 1] = qstat[r * 4 + 2] = qstat[r * 4 + 3] = 0.f;
    return;
  }
  const float* src = q + r * dim;
  float s2 = 0.f, e2 = 0.f, c2 = 0.f, qm = 0.f;
  for (int c = lane * 4; c < d_pad8; c += 256) {
    u32 packed = 0;
    double xd[4] = {0.0, 0.0, 0.0, 0.0};
    if (ROT && c < rot_w) rot256_load(src, dim, sp, c, lane, xd);   // the query in the table's rotated frame
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (ROT ? c < rot_w : c + e < dim) {
        const float xv = ROT ? (float)xd[e] : src[c + e];
        const float m = mu[c + e];
        const float dx = ROT ? (float)(xd[e] - (double)m) : xv - m;
        const int qi = quant8(dx, 0.f, inv_step);
        const float res = fmaf(-step, (float)qi, dx);
        packed |= (u32)(qi & 255) << (8 * e);
        s2 = fmaf(xv, xv, s2);
        c2 = fmaf(dx, dx, c2);
        e2 = fmaf(res, res, e2);
        qm = fmaf(xv, m, qm);
      }
    }
    *reinterpret_cast<u32*>(dst + c) = packed;
    fput(c, packed);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s2 += __shfl_xor(s2, o);
    e2 += __shfl_xor(e2, o);
    c2 += __shfl_xor(c2, o);
    qm += __shfl_xor(qm, o);
  }
  if (lane == 0) {
    const float nqc = sqrtf(c2) * 1.000001f, eqc = sqrtf(e2) * 1.00001f + 1.2e-7f * sqrtf(c2) + (ROT ? 1e-12f * sqrtf(s2) : 0.f);
    qstat[r * 4 + 0] = s2;
    qstat[r * 4 + 1] = nqc;
    qstat[r * 4 + 2] = eqc;
    qstat[r * 4 + 3] = metric == 0 ? c2 : (metric == 1 ? 1.f - qm : -qm);
    if (x.qmax) {   // (non-negative floats order like their bit patterns; a NaN's pattern is above every number: its batch forces every row)
      atomicMax(&x.qmax[0], __float_as_uint(nqc));
      atomicMax(&x.qmax[1], __float_as_uint(eqc));
    }
  }
}

// (the frame is the mirror's: HalfMirror::rot8 / sp8)
static void launch_query_prep8(dim3 grid, hipStream_t s, const int* sp, int rot_w, const float* q, int64_t nq, int64_t b_pad, int dim, int d_pad8, const float* mu, float step,
                               int metric, signed char* q8, float* qstat, const Prep8Extra& x) {
  if (sp) hipLaunchKernelGGL(query_prep8_kernel<true>, grid, dim3(256), 0, s, q, nq, b_pad, dim, d_pad8, mu, step, 1.f / step, metric, q8, qstat, x, sp, rot_w);
  else hipLaunchKernelGGL(query_prep8_kernel<false>, grid, dim3(256), 0, s, q, nq, b_pad, dim, d_pad8, mu, step, 1.f / step, metric, q8, qstat, x, (const int*)nullptr, 0);
}

hipError_t prep8_queries(HalfMirror& m, bool fold, int dim, int metric, const float* q, int64_t nq, int64_t rows, signed char* q8, float* qstat, Prep8Extra px,
                         hipStream_t s) {
  hipError_t er = hipSuccess;
  if (fold) {
    px.qmax = m.qmax.as<u32>();
    er = hipMemsetAsync(m.qmax.p, 0, 8, s);
  }
  launch_query_prep8(dim3((unsigned)((rows + 3) / 4)), s, m.rot8 ? m.sp8.as<int>() : nullptr, m.rot_w8, q, nq, rows, dim, m.d_pad8, m.mu8.as<float>(), m.step8, metric, q8,
                     qstat, px);
  if (fold)   // (16 bytes per row: 5 us at 1M rows, 40 us at 10M)
    hipLaunchKernelGGL(fold8_kernel, dim3((unsigned)std::min<int64_t>((m.n_pad8 + 255) / 256, 8192)), dim3(256), 0, s, m.acc0.as<int>(), m.erow.as<float>(),
                       m.hrow.as<float>(), m.n8, m.n_pad8, m.qmax.as<u32>(), metric == 0 ? 2.f : 1.f, 1.f / key_unit8(metric, m.step8), m.acc0b.as<int>());
  return er;
}

// ------------------------------------------------------------------------------------------------ host
static bool grow_keep(DevBuf& b, size_t bytes, size_t keep, hipStream_t s) {
  if (bytes <= b.cap) return true;
  DevBuf bigger;
  if (!bigger.reserve(bytes + bytes / 4)) return false;
  if (keep && b.p && hipMemcpyAsync(bigger.p, b.p, keep, hipMemcpyDeviceToDevice, s) != hipSuccess) return false;
  if (hipStreamSynchronize(s) != hipSuccess) return false;
  b.release();
  b.p = bigger.p;
  b.cap = bigger.cap;
  bigger.p = nullptr;
  bigger.cap = 0;
  return true;
}

int32_t ensure_mirror(Index& ix) {
  if (!ix.mirror_) ix.mirror_ = new HalfMirror();
  HalfMirror& m = *ix.mirror_;
  const int64_t n = ix.n_rows_;
  if (m.version == ix.rows_version_ && m.n == n) return EPS_OK;
  // appended rows: only the new rows are converted; the 15 GB mirror of a 10M-row table is not rebuilt
  const bool extend = m.version == ix.rows_version_ && m.n > 0 && m.n < n;
  const int64_t n_pad = (n + ROWPAD - 1) / ROWPAD * ROWPAD;
  const int d_pad = (int)((ix.dim_ + BK - 1) / BK * BK);
  hipStream_t s = ix.stream_;
  const size_t keep_rows = extend ? (size_t)m.n : 0;
  if (!grow_keep(m.xh, (size_t)n_pad * d_pad * 2, keep_rows * d_pad * 2, s) || !grow_keep(m.xn, (size_t)n_pad * 4, keep_rows * 4, s) ||
      !grow_keep(m.zeros, (size_t)n_pad * 4, keep_rows * 4, s) || !grow_keep(m.xn_s, (size_t)n_pad * 4, keep_rows * 4, s) ||
      !grow_keep(m.zeros_s, (size_t)n_pad * 4, keep_rows * 4, s) || !m.scal.reserve(64))
    return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory for the fp16 mirror");
  hipError_t er = hipSuccess;
  if (!extend) er = hipMemsetAsync(m.scal.p, 0, 64, s);
  if (er != hipSuccess) return ix.hip_fail(er, "memset");
  // fp32 accumulation slack of the MFMA dot product: <= 4 * d * 2^-24 * |qh||xh| (generous: covers any
  // internal summation order / truncating adder)
  const float gamma = 4.0f * (float)d_pad * 5.9604645e-8f;
  const int64_t row0 = extend ? m.n : 0;
  hipLaunchKernelGGL(half_mirror_kernel, dim3((unsigned)std::min<int64_t>((n_pad - row0 + 3) / 4, 8192)), dim3(256), 0, s, ix.d_rows_, row0, n, n_pad,
                     (int)ix.dim_, d_pad, m.xh.as<_Float16>(), m.xn.as<float>(), m.zeros.as<float>(), m.xn_s.as<float>(), m.zeros_s.as<float>(),
                     m.scal.as<float>(), gamma);
  er = hipMemcpyAsync(m.h_scal, m.scal.p, 16, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return ix.hip_fail(er, "fp16 mirror build");
  m.fp16_range_ok = (m.h_scal[3] == 0.f);
  m.n = n;
  m.n_pad = n_pad;
  m.d_pad = d_pad;
  m.version = ix.rows_version_;
  m.extended_rows += extend ? n - row0 : 0;
  return EPS_OK;
}

static float host_ord2f(u32 o) {
  const u32 u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}


static const char* const OOM8 = "MFMA engine: out of device memory for the 8-bit mirror";

// R's permutation and signs: a fixed sequence (splitmix64), the same for every table of this width
static std::vector<int32_t> rotation_table(int W, int d_pad8) {
  std::vector<int32_t> sp((size_t)d_pad8, 0);
  for (int i = 0; i < W; ++i) sp[(size_t)i] = i;
  uint64_t st = 0x9E3779B97F4A7C15ull ^ (uint64_t)W;
  auto next = [&st]() {
    uint64_t z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  for (int i = W - 1; i > 0; --i) std::swap(sp[(size_t)i], sp[(size_t)(next() % (uint64_t)(i + 1))]);
  for (int i = 0; i < W; ++i)
    if (next() & 1ull) sp[(size_t)i] |= (int32_t)0x80000000u;
  return sp;
}

// One frame's grid: the clipped value range's centre and half width, whether the table fits one grid at all
struct Grid { bool ok = false; float z0 = 0.f, half = 127.f, step = 0.f; };
// The rows a frame's statistics are taken from: every stride-th row of `rows` (n x dim), `sampled` of them in CENTRE_SEG segments of per_seg
struct SampleRows { const float* rows; int64_t n, stride, sampled, per_seg; int dim; };

// clip both tails of the SAMPLE's x - mean at max(2, clip_frac x values) values (centre_hist_kernel); where the cut removes most of the
// range - an outlier thousands of grid widths away leaves the bulk in ONE bin - the histogram is taken again inside the cut (values
// outside fall into the edge bins), up to three times
static int32_t clip_range(Index& ix, HalfMirror& m, const SampleRows& sr, const float* mean, double clip_frac, float* clo, float* chi) {
  hipStream_t s = ix.stream_;
  for (int round = 0; round < 3; ++round) {
    const float binw = (*chi - *clo) / 4096.f;
    if (!(binw > 0.f) || !std::isfinite(1.f / binw)) break;
    std::vector<u32> hh(4096);
    hipError_t e3 = hipMemsetAsync(m.hist.p, 0, (4096 + 8) * 4, s);
    if (e3 != hipSuccess) return ix.hip_fail(e3, "memset");
    hipLaunchKernelGGL(centre_hist_kernel, dim3((unsigned)std::min<int64_t>(sr.sampled, 4096)), dim3(256), 0, s, sr.rows, sr.n, sr.dim, sr.stride, sr.sampled, mean, *clo,
                       1.f / binw, m.hist.as<u32>());
    e3 = hipMemcpyAsync(hh.data(), m.hist.p, 4096 * 4, hipMemcpyDeviceToHost, s);
    if (e3 == hipSuccess) e3 = hipStreamSynchronize(s);
    if (e3 != hipSuccess) return ix.hip_fail(e3, "8-bit mirror: value histogram");
    const unsigned long long tol = std::max<unsigned long long>(2ull, (unsigned long long)(clip_frac * (double)sr.sampled * (double)sr.dim));
    unsigned long long cum = 0;
    int blo = 0, bhi = 4095;
    for (blo = 0; blo < 4096; ++blo) {
      cum += hh[(size_t)blo];
      if (cum > tol) break;
    }
    cum = 0;
    for (bhi = 4095; bhi >= 0; --bhi) {
      cum += hh[(size_t)bhi];
      if (cum > tol) break;
    }
    const float a = *clo + (float)blo * binw, b = *clo + (float)(bhi + 1) * binw;
    if (!(blo < 4096 && bhi >= 0 && b > a)) break;
    const bool cut_most = (b - a) < 0.25f * (*chi - *clo);
    *clo = a;
    *chi = b;
    if (!cut_most) break;
  }
  return EPS_OK;
}

// One frame's grid from the table's values: centre into `mu_out`, the clipped value range into *g.  `rot`: measured on the rotated images of
// the sample rows (all W = m.rot_w8 columns carry values), the value range over the whole table through the transform.
static int32_t measure_grid(Index& ix, HalfMirror& m, bool rot, const SampleRows& table, int d_pad8, DevBuf& mu_out, Grid* g) {
  hipStream_t s = ix.stream_;
  DevBuf part, rsample;
  SampleRows sr = table;
  const int W = m.rot_w8;
  if (rot) {
    if (!rsample.reserve((size_t)table.sampled * W * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, OOM8);
    hipLaunchKernelGGL(rot_sample_kernel, dim3((unsigned)std::min<int64_t>((table.sampled + 3) / 4, 8192)), dim3(256), 0, s, table.rows, table.n, table.dim, table.stride,
                       table.sampled, W, m.sp8.as<int>(), rsample.as<float>());
    sr.rows = rsample.as<float>();
    sr.n = table.sampled;
    sr.stride = 1;
    sr.dim = W;
  }
  hipError_t e2 = hipMemsetAsync(m.scal8.p, 0, 32, s);
  if (e2 == hipSuccess) e2 = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.scal8.as<u32>() + 6), (int)0xFFFFFFFFu, 1, s);
  if (e2 != hipSuccess) return ix.hip_fail(e2, "memset");
  if (!part.reserve((size_t)CENTRE_SEG * sr.dim * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, OOM8);
  const dim3 sum_grid((unsigned)((sr.dim + 63) / 64), CENTRE_SEG), mean_grid((unsigned)((d_pad8 + 255) / 256));
  hipLaunchKernelGGL(colsum_kernel, sum_grid, dim3(256), 0, s, sr.rows, sr.n, sr.dim, sr.stride, sr.per_seg, part.as<float>(), (const float*)nullptr, 0.f, 0.f);
  hipLaunchKernelGGL(colmean_kernel, mean_grid, dim3(256), 0, s, part.as<float>(), sr.dim, d_pad8, 1.f / (float)sr.sampled, mu_out.as<float>());
  const unsigned mm_grid = (unsigned)std::min<int64_t>((table.n + 3) / 4, 8192);
  if (rot) hipLaunchKernelGGL(minmax_kernel<true>, dim3(mm_grid), dim3(256), 0, s, table.rows, table.n, table.dim, mu_out.as<float>(), m.scal8.as<u32>(), m.sp8.as<int>(), W);
  else hipLaunchKernelGGL(minmax_kernel<false>, dim3(mm_grid), dim3(256), 0, s, table.rows, table.n, table.dim, mu_out.as<float>(), m.scal8.as<u32>(), (const int*)nullptr, d_pad8);
  e2 = hipMemcpyAsync(m.h_scal8, m.scal8.p, 32, hipMemcpyDeviceToHost, s);
  if (e2 == hipSuccess) e2 = hipStreamSynchronize(s);   // (also keeps `part` alive until its readers are done)
  if (e2 != hipSuccess) return ix.hip_fail(e2, "8-bit mirror: value range");
  u32 omin, omax;
  std::memcpy(&omin, &m.h_scal8[6], 4);
  std::memcpy(&omax, &m.h_scal8[7], 4);
  const float lo = host_ord2f(omin), hi = host_ord2f(omax);
  g->ok = m.h_scal8[3] == 0.f && omin <= omax && hi > lo && std::isfinite(lo) && std::isfinite(hi) && std::isfinite(hi - lo);
  float clo = lo, chi = hi;
  // (EPS_MIRROR_CLIP = e: cut 10^-e of the sample's values off each tail instead of 10^-7, and keep the cut in the rotated frame too - lab knob, r6)
  const char* clip_e = tune_env("EPS_MIRROR_CLIP");
  // r6, rotated frame: the cut is kept, at 10^-6 per tail.  Near-Gaussian columns put the whole table's range at ~6.3 sigma (10M x 768 values)
  // while 10^-6 of them lie beyond 4.9 sigma: the step - and with it both terms of the margin - shrinks by a quarter, the 0.15 % of rows with
  // a clamped value carry their own residual (folded per batch: 40 us at 10M rows).  10M x 768 embedding-like rows, batch 1024: 958 instead of
  // 2186 re-ranked rows per query, 8.80 -> 7.64 ms per step (10^-7: 7.87, 10^-5: 8.08 - clamped residuals start to dominate;
  // profiles/r6_embedding_like_grid_cut.txt).  1M x 768, 1 / 3 / 8 / 16 queries per call (the one-pass search, which serves tables with
  // folded margins since r6): 0.232 / 0.281 / 0.299 / 0.356 ms against 0.286 / 0.380 / 0.497 / 0.464 with the whole range
  // (profiles/r6_rotated_frame_one_pass_1M.txt).
  const double clip_frac = clip_e ? std::pow(10.0, -std::max(1.0, std::min(9.0, atof(clip_e)))) : (rot ? 1e-6 : 1e-7);
  int32_t rc = g->ok ? clip_range(ix, m, sr, mu_out.as<float>(), clip_frac, &clo, &chi) : EPS_OK;
  if (rc != EPS_OK) return rc;
  if (g->ok && (clo > lo || chi < hi)) {
    // something was cut: the column means it polluted are estimated again from values clamped into the cut (same fixed summation
    // order), and the range once more around the new means (the first range, widened by the largest move of a mean, bounds it)
    DevBuf mean1;
    std::vector<float> h1((size_t)sr.dim), h2((size_t)sr.dim);
    if (!mean1.reserve((size_t)d_pad8 * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, OOM8);
    hipError_t e3 = hipMemcpyAsync(mean1.p, mu_out.p, (size_t)d_pad8 * 4, hipMemcpyDeviceToDevice, s);
    if (e3 != hipSuccess) return ix.hip_fail(e3, "memcpy");
    hipLaunchKernelGGL(colsum_kernel, sum_grid, dim3(256), 0, s, sr.rows, sr.n, sr.dim, sr.stride, sr.per_seg, part.as<float>(), mean1.as<float>(), clo, chi);
    hipLaunchKernelGGL(colmean_kernel, mean_grid, dim3(256), 0, s, part.as<float>(), sr.dim, d_pad8, 1.f / (float)sr.sampled, mu_out.as<float>());
    e3 = hipMemcpyAsync(h1.data(), mean1.p, (size_t)sr.dim * 4, hipMemcpyDeviceToHost, s);
    if (e3 == hipSuccess) e3 = hipMemcpyAsync(h2.data(), mu_out.p, (size_t)sr.dim * 4, hipMemcpyDeviceToHost, s);
    if (e3 == hipSuccess) e3 = hipStreamSynchronize(s);
    if (e3 != hipSuccess) return ix.hip_fail(e3, "8-bit mirror: column means");
    float delta = 0.f;
    for (int c = 0; c < sr.dim; ++c) delta = std::max(delta, std::fabs(h2[(size_t)c] - h1[(size_t)c]));
    clo = lo - delta;
    chi = hi + delta;
    rc = clip_range(ix, m, sr, mu_out.as<float>(), clip_frac, &clo, &chi);
    if (rc != EPS_OK) return rc;
  }
  g->z0 = g->ok ? 0.5f * clo + 0.5f * chi : 0.f;
  g->half = g->ok ? std::max(chi - g->z0, g->z0 - clo) : 127.f;
  g->step = g->half / 127.f;
  if (g->ok && !(g->step > 0.f && std::isfinite(1.f / (g->step * g->step)))) g->ok = false;
  return EPS_OK;
}

// First build: the frame (r6), the centre and the step of the table's grid, and the start state of the quantising pass
static int32_t choose_grid(Index& ix, HalfMirror& m, int64_t n, int d_pad8) {
  hipStream_t s = ix.stream_;
  const int dim = (int)ix.dim_;
  hipError_t er = hipSuccess;
  // centre: column means of up to 65 536 rows spread evenly over the table (any centre is valid, see above), summed in a fixed order
  const int64_t sample = std::min<int64_t>(n, 65536);
  SampleRows table = {ix.d_rows_, n, std::max<int64_t>(1, n / sample), 0, (sample + CENTRE_SEG - 1) / CENTRE_SEG, dim};
  table.sampled = std::min<int64_t>((n + table.stride - 1) / table.stride, table.per_seg * CENTRE_SEG);
  // r6: the frame.  0 = identity, 1 = rotated, otherwise the library's choice (both measured, below)
  const char* rot_e = tune_env("EPS_MIRROR_ROTATE");
  const int rot_mode = rot_e ? atoi(rot_e) : -1;
  const int W = (dim + 255) / 256 * 256;   // the rotation's width (the mirror pads rows to at least 512 bytes: those columns stay zero)
  m.rot_w8 = W;
  if (rot_mode != 0) {
    const std::vector<int32_t> sp = rotation_table(W, d_pad8);
    if (!m.sp8.reserve((size_t)d_pad8 * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, OOM8);
    er = hipMemcpyAsync(m.sp8.p, sp.data(), (size_t)d_pad8 * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) return ix.hip_fail(er, "8-bit mirror: rotation table");
  }
  // The choice: a row's residual norm is ~ step x sqrt(columns that carry values / 12) in either frame - the identity frame quantises
  // `dim` columns, the rotated one W = dim rounded up to 256 - so the frame with the smaller product gives the tighter margin.  The rotated frame must
  // win clearly (0.75): at equal margins the identity frame's query preparation is cheaper, and it is the frame every earlier round measured.
  Grid gi, gr;
  DevBuf mu_rot;
  m.step8_identity = m.step8_rotated = 0.f;
  if (rot_mode != 1) {
    const int32_t rc = measure_grid(ix, m, false, table, d_pad8, m.mu8, &gi);
    if (rc != EPS_OK) return rc;
    m.step8_identity = gi.ok ? gi.step : 0.f;
  }
  if (rot_mode != 0 && (rot_mode == 1 || gi.ok)) {
    if (!mu_rot.reserve((size_t)d_pad8 * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, OOM8);
    const int32_t rc = measure_grid(ix, m, true, table, d_pad8, mu_rot, &gr);
    if (rc != EPS_OK) return rc;
    m.step8_rotated = gr.ok ? gr.step : 0.f;
  }
  m.rot8 = rot_mode == 1 || (rot_mode != 0 && gi.ok && gr.ok &&
                             (double)gr.step * std::sqrt((double)W) < 0.75 * (double)gi.step * std::sqrt((double)dim));
  const Grid& g = m.rot8 ? gr : gi;
  if (m.rot8) {
    er = hipMemcpyAsync(m.mu8.p, mu_rot.p, (size_t)d_pad8 * 4, hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) return ix.hip_fail(er, "memcpy");
  }
  m.i8_ok = g.ok;
  er = hipMemsetAsync(m.scal8.p, 0, 32, s);
  if (er != hipSuccess) return ix.hip_fail(er, "memset");
  if (m.i8_ok) {
    er = hipMemsetAsync(m.hist.p, 0, (4096 + 8) * 4, s);   // ([4096]: the forced-row counter of the quantising pass)
    if (er != hipSuccess) return ix.hip_fail(er, "memset");
  }
  m.step8 = g.step;
  if (m.i8_ok) {
    hipLaunchKernelGGL(mu_finish_kernel, dim3(1), dim3(64), 0, s, m.mu8.as<float>(), m.rot8 ? W : dim, g.z0, m.scal8.as<float>());
    er = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.scal8.as<u32>() + 7), 0x7F800000, 1, s);   // min residual norm: +inf
    if (er != hipSuccess) return ix.hip_fail(er, "memset");
  }
  return EPS_OK;
}

static void release_mirror8_rows(HalfMirror& m) {
  m.x8.release();
  m.acc0.release();
  m.erow.release();
  m.hrow.release();
  m.acc0b.release();
}

// the 8-bit mirror: centre and grid from the table's values on the first build, kept when rows are appended
int32_t ensure_mirror8(Index& ix) {
  if (!ix.mirror_) ix.mirror_ = new HalfMirror();
  HalfMirror& m = *ix.mirror_;
  const int64_t n = ix.n_rows_;
  if (m.version8 == ix.rows_version_ && m.n8 == n) return EPS_OK;
  const bool extend = m.version8 == ix.rows_version_ && m.n8 > 0 && m.n8 < n && m.i8_ok;
  const int64_t n_pad = (n + ROWPAD - 1) / ROWPAD * ROWPAD;
  const int d_pad8 = std::max(512, (int)((ix.dim_ + 255) / 256 * 256));   // K-steps of 128 bytes, in pairs, at least four
  const int dim = (int)ix.dim_;
  hipStream_t s = ix.stream_;
  const size_t keep_rows = extend ? (size_t)m.n8 : 0;
  if (!grow_keep(m.x8, (size_t)n_pad * d_pad8, keep_rows * d_pad8, s) || !grow_keep(m.acc0, (size_t)n_pad * 4, keep_rows * 4, s) || !m.scal8.reserve(64) ||
      !m.mu8.reserve((size_t)d_pad8 * 4) || !grow_keep(m.erow, (size_t)n_pad * 4, keep_rows * 4, s) || !grow_keep(m.hrow, (size_t)n_pad * 4, keep_rows * 4, s) ||
      !m.acc0b.reserve((size_t)n_pad * 4) || !m.scal8f.reserve(64) || !m.qmax.reserve(16) || !m.hist.reserve((4096 + 8) * 4)) {
    (void)hipGetLastError();
    if (!extend) {   // (nothing half-built stays behind: the callers for whom the mirror is optional carry on without it)
      release_mirror8_rows(m);
      m.version8 = -1;
    }
    return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, OOM8);
  }
  if (!extend) {
    const int32_t rc = choose_grid(ix, m, n, d_pad8);
    if (rc != EPS_OK) return rc;
  }
  if (m.i8_ok) {
    const float u = key_unit8(ix.metric_, m.step8);
    const int64_t row0 = extend ? m.n8 : 0;
    const dim3 qgrid((unsigned)std::min<int64_t>((n_pad - row0 + 3) / 4, 8192));
    if (m.rot8)
      hipLaunchKernelGGL(quant_mirror_kernel<true>, qgrid, dim3(256), 0, s, ix.d_rows_, row0, n, n_pad, dim, d_pad8, m.mu8.as<float>(), m.step8, 1.f / m.step8, 1.f / u,
                         ix.metric_, m.x8.as<signed char>(), m.acc0.as<int>(), m.scal8.as<float>(), m.erow.as<float>(), m.hrow.as<float>(), m.hist.as<u32>() + 4096,
                         m.sp8.as<int>(), m.rot_w8);
    else
      hipLaunchKernelGGL(quant_mirror_kernel<false>, qgrid, dim3(256), 0, s, ix.d_rows_, row0, n, n_pad, dim, d_pad8, m.mu8.as<float>(), m.step8, 1.f / m.step8, 1.f / u,
                         ix.metric_, m.x8.as<signed char>(), m.acc0.as<int>(), m.scal8.as<float>(), m.erow.as<float>(), m.hrow.as<float>(), m.hist.as<u32>() + 4096,
                         (const int*)nullptr, 0);
    hipLaunchKernelGGL(scal_finish_kernel, dim3(1), dim3(64), 0, s, m.scal8.as<float>(), m.scal8f.as<float>());
    u32 forced = 0;
    hipError_t er = hipMemcpyAsync(m.h_scal8, m.scal8.p, 32, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipMemcpyAsync(&forced, m.hist.as<u32>() + 4096, 4, hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) return ix.hip_fail(er, "8-bit mirror build");
    m.forced_rows8 = (int64_t)forced;   // (accumulated over extensions: the counter is only zeroed with the histogram)
    // a non-finite value, or a table most of whose row constants leave the accumulator's range (IP / COSINE far from the origin: |mu . x'| / step^2):
    // the fp16 engine serves this table
    if (m.h_scal8[3] != 0.f || (double)forced > 0.01 * (double)n) m.i8_ok = false;
    // Per-row margins are folded per batch only where rows DIFFER: a forced row, or a residual norm beyond 1.5 x the smallest (a clamped
    // value somewhere).  On homogeneous tables (every row a plain rounding residual: within a few per cent of each other) the table-wide
    // margin in the thresholds is as tight, keeps every query's own norms, and costs no pass over the rows (10M rows: 40 us per batch).
    m.fold8 = forced > 0 || m.h_scal8[0] > 1.5f * m.h_scal8[7];
    m.extended_rows8 += extend ? n - row0 : 0;
  }
  if (!m.i8_ok) release_mirror8_rows(m);   // nothing of it is used: give the memory back
  if (!extend) {
    m.i8_overflows = 0;
    m.i8_trusted = false;
    m.epoch8 += 1;
  }
  m.n8 = n;
  m.n_pad8 = n_pad;
  m.d_pad8 = d_pad8;
  m.version8 = ix.rows_version_;
  return EPS_OK;
}

// The 8-bit mirror for kernels outside the flat matrix engine (the traversal's lower-bound prefilter): built or extended on demand;
// v->x8 stays null when the table cannot be put on one grid (non-finite values, constants beyond int32).
int32_t quant8_view(Index& ix, Quant8View* v) {
  *v = Quant8View();
  const int32_t rc = ensure_mirror8(ix);
  if (rc != EPS_OK) return rc;
  const HalfMirror& m = *ix.mirror_;
  if (!m.i8_ok) return EPS_OK;
  v->x8 = m.x8.as<signed char>();
  // (what the traversal kernels read: the start values with the CURRENT batch's per-row margins folded in - quant8_queries below folds
  // them after every query preparation - and the maxima whose two margin entries are zero: their thresholds carry no margin)
  v->acc0 = m.fold8 ? m.acc0b.as<int>() : m.acc0.as<int>();
  v->scal8 = m.fold8 ? m.scal8f.as<float>() : m.scal8.as<float>();
  v->mu = m.mu8.as<float>();
  v->d_pad8 = m.d_pad8;
  v->cols8 = m.rot8 ? m.rot_w8 : (int)ix.dim_;
  v->step = m.step8;
  v->u = key_unit8(ix.metric_, m.step8);
  v->epoch8 = m.epoch8;
  v->per_batch = m.fold8;
  return EPS_OK;
}

// nq queries on the mirror's grid: q8 [nq][d_pad8], qstat [nq][4] (device buffers of the caller).  (The grid is the mirror's own: what `v` copied.)
void quant8_queries(Index& ix, const Quant8View&, const float* dq, int64_t nq, signed char* q8, float* qstat) {
  HalfMirror& m = *ix.mirror_;
  (void)prep8_queries(m, m.fold8, (int)ix.dim_, ix.metric_, dq, nq, nq, q8, qstat, Prep8Extra(), ix.stream_);
}

}  // namespace eps
