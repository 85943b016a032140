// Which int8 MFMA shape does the board clock higher under the filter kernel's tile?  v_mfma_i32_32x32x32_i8 (mfma_filter_kernel_v7 today:
// 16 MFMAs of 32 cycles per K = 32) against v_mfma_i32_16x16x64_i8 (64 MFMAs of 16 cycles per K = 64): the same 1024 MACs per cycle, half
// the accumulator reads and writes per MAC.  Every wavefront owns the kernel's 256 rows x 64 queries (256 accumulator registers), one
// wavefront per SIMD, 256 workgroups x 4 wavefronts, bytes uniform in [-127, 127].  Two forms per shape:
//   reg   row and query fragments stay in registers (two alternating sets)
//   lds   the row fragments are re-read from a 4-slot ring of 256 rows x 128 B with ds_read_b128 in the kernel's granule swizzle and at the
//         kernel's volume (32 reads per wavefront and K-step of 128 B, one behind every second 32x32x32 / every fourth 16x16x64 MFMA);
//         query fragments stay in registers as in the kernel between its loads
// Each loop is launched back to back for >= 2 s and rated over the second half of that window; the in-kernel clock is delta s_memtime
// over delta s_memrealtime (100 MHz) around the loop, median over workgroups, written to a buffer nothing else reads.  The loops alternate, two
// rounds.  A short launch first checks that both lds loops multiply the same matrices (the sum of all accumulators must agree).
//   hipcc --offload-arch=gfx950 -O3 scripts/lab/mfma_shape_i8.hip -o scripts/lab/mfma_shape_i8 && scripts/lab/mfma_shape_i8
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32;

#define CHECK(x)                                                                          \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));   \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

constexpr int SLOT = 256 * 128;   // one ring slot: 256 rows x 128 B
constexpr int RING = 4;

__host__ __device__ inline u32 mix(u32 x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
// byte k of row `row` of ring slot `slot`; byte k of query `q` (0..63 of wavefront `w`) in query set `set`
__device__ inline int row_byte(int slot, int row, int k) { return (int)(mix((u32)((slot * 256 + row) * 128 + k) + 0x9e3779b9u) % 255u) - 127; }
__device__ inline int qry_byte(int w, int set, int q, int k) { return (int)(mix((u32)(((w * 2 + set) * 64 + q) * 128 + k) + 0x51ed270bu) % 255u) - 127; }
__device__ inline int swz(int row, int chunk) { return (row << 3) + (chunk ^ ((row >> 1) & 7)); }   // the kernel's 16-B granule index

template <class F> __device__ inline i32x4 pack16(F f) {   // 16 consecutive bytes f(0..15) -> one fragment register quad
  i32x4 v;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    u32 x = 0;
    for (int e = 0; e < 4; ++e) x |= (u32)(f(4 * w + e) & 255) << (8 * e);
    v[w] = (int)x;
  }
  return v;
}

__device__ inline void fill_ring(unsigned char* lds) {
  for (int g = threadIdx.x; g < RING * 256 * 8; g += 256) {
    const int slot = g >> 11, row = (g >> 3) & 255, chunk = g & 7;
    *reinterpret_cast<i32x4*>(lds + slot * SLOT + swz(row, chunk) * 16) = pack16([&](int b) { return row_byte(slot, row, chunk * 16 + b); });
  }
  __syncthreads();
}

#define SB __builtin_amdgcn_sched_barrier(0)
// The loops are hand-issued like the product kernel's: MFMAs and fragment reads are inline asm (hipcc neither reorders nor pads them, and
// left to itself it shuffles the 16x16 loop's 256 + 128 registers through v_accvgpr copies and scratch), accumulators of the first row
// blocks in arch VGPRs and the rest, with all fragments, in the accumulator file, waits counted by hand.
#define LAB_DS_READ_B128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=a"(dst) : "v"(addr), "n"(off))
#define LAB_WAIT_LGKM(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")
template <bool V> __device__ __forceinline__ void mfma32(i32x16& acc, const i32x4& a, const i32x4& b) {
  if (V) asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(acc) : "a"(a), "a"(b));
  else asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+a"(acc) : "a"(a), "a"(b));
}
template <bool V> __device__ __forceinline__ void mfma16(i32x4& acc, const i32x4& a, const i32x4& b) {
  if (V) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "a"(a), "a"(b));
  else asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc) : "a"(a), "a"(b));
}
#define LAB_PIN_A(x) asm volatile("" : "+a"(x))   // one register tuple in the accumulator file from here on (or hipcc re-forms it at every use)
constexpr int ACC_V = 224;   // accumulator registers kept in arch VGPRs (the product kernel: 7 of its 8 row blocks)

// ---------------------------------------------------------------------------------------------- 32x32x32: 8 row blocks x 2 query blocks
// A (rows): lane l holds row l % 32, bytes 16 (l / 32) .. + 16 of a K = 32 piece; B (queries) the same for query l % 32.
template <bool LDSF>
__global__ __launch_bounds__(256, 1) void loop32(u32* out, int iters, long long* clk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  fill_ring(lds);
  i32x4 fb[2][4][2];   // query fragments of two K-steps
#pragma unroll
  for (int set = 0; set < 2; ++set)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        fb[set][kk][j] = pack16([&](int b) { return qry_byte(wave, set, 32 * j + (lane & 31), 32 * kk + 16 * (lane >> 5) + b); });
        LAB_PIN_A(fb[set][kk][j]);
      }
  u32 faddr[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) faddr[kk] = (u32)swz(lane & 31, kk * 2 + (lane >> 5)) * 16;
  i32x4 fa[2][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    fa[0][i] = *reinterpret_cast<const i32x4*>(lds + faddr[0] + i * 4096);
    fa[1][i] = *reinterpret_cast<const i32x4*>(lds + faddr[1] + i * 4096);   // (reg form: the second set; lds form: overwritten)
    LAB_PIN_A(fa[0][i]);
    LAB_PIN_A(fa[1][i]);
  }
  i32x16 acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
  __syncthreads();
  SB;
  const long long c0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
  SB;
  u32 slot = 0;
  for (int it = 0; it < iters; it += 2) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const u32 slot_n = (slot + SLOT) & (RING * SLOT - 1);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int cur = kk & 1, nxt = cur ^ 1;
        const u32 ad = faddr[(kk + 1) & 3] + (kk < 3 ? slot : slot_n);   // the NEXT sub-step's operands
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (LDSF) LAB_WAIT_LGKM(7);
          SB;
          if (i * 32 < ACC_V) mfma32<true>(acc[i][0], fa[cur][i], fb[rb][kk][0]); else mfma32<false>(acc[i][0], fa[cur][i], fb[rb][kk][0]);
          SB;
          if (LDSF) {
            switch (i) {
              case 0: LAB_DS_READ_B128(fa[nxt][0], ad, 0); break;
              case 1: LAB_DS_READ_B128(fa[nxt][1], ad, 4096); break;
              case 2: LAB_DS_READ_B128(fa[nxt][2], ad, 8192); break;
              case 3: LAB_DS_READ_B128(fa[nxt][3], ad, 12288); break;
              case 4: LAB_DS_READ_B128(fa[nxt][4], ad, 16384); break;
              case 5: LAB_DS_READ_B128(fa[nxt][5], ad, 20480); break;
              case 6: LAB_DS_READ_B128(fa[nxt][6], ad, 24576); break;
              default: LAB_DS_READ_B128(fa[nxt][7], ad, 28672); break;
            }
          }
          SB;
          if (i * 32 < ACC_V) mfma32<true>(acc[i][1], fa[cur][i], fb[rb][kk][1]); else mfma32<false>(acc[i][1], fa[cur][i], fb[rb][kk][1]);
          SB;
        }
      }
      slot = slot_n;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 7" ::: "memory");   // hipcc pads nothing behind an asm MFMA whose D the sums below read
  SB;
  const long long c1 = __builtin_amdgcn_s_memtime(), w1 = __builtin_amdgcn_s_memrealtime();
  SB;
  u32 s = 0;   // (wraps; the comparison between the shapes is modulo 2^32)
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) s += (u32)acc[i][j][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) {
    clk[2 * blockIdx.x] = c1 - c0;
    clk[2 * blockIdx.x + 1] = w1 - w0;
  }
}

// ---------------------------------------------------------------------------------------------- 16x16x64: 16 row blocks x 4 query blocks
// A (rows): lane l holds row l % 16, bytes 16 (l / 16) .. + 16 of a K = 64 piece = granule (row 16 i + l % 16, chunk 4 s + l / 16) of
// sub-step s; B (queries) the same for query l % 16.  Row fragments are single-buffered: block i's registers are reloaded for the next
// sub-step behind the first MFMA of block i + 1 (15 blocks = 960 matrix cycles ahead of their use).
template <bool LDSF>
__global__ __launch_bounds__(256, 1) void loop16(u32* out, int iters, long long* clk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  fill_ring(lds);
  i32x4 fb[2][2][4];   // query fragments of two K-steps
#pragma unroll
  for (int set = 0; set < 2; ++set)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        fb[set][s][j] = pack16([&](int b) { return qry_byte(wave, set, 16 * j + (lane & 15), 64 * s + 16 * (lane >> 4) + b); });
        LAB_PIN_A(fb[set][s][j]);
      }
  u32 faddr[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) faddr[s] = (u32)swz(lane & 15, 4 * s + (lane >> 4)) * 16;   // + 2048 i: (row >> 1) & 7 does not depend on i
  constexpr int NSET = LDSF ? 1 : 2;
  i32x4 fa[NSET][16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    fa[0][i] = *reinterpret_cast<const i32x4*>(lds + faddr[0] + i * 2048);
    if (!LDSF) fa[NSET - 1][i] = *reinterpret_cast<const i32x4*>(lds + faddr[1] + i * 2048);
    LAB_PIN_A(fa[0][i]);
    if (!LDSF) LAB_PIN_A(fa[NSET - 1][i]);
  }
  i32x4 acc[16][4];
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0;
  __syncthreads();
  SB;
  const long long c0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
  SB;
  u32 slot = 0;
  for (int it = 0; it < iters; it += 2) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const u32 slot_n = (slot + SLOT) & (RING * SLOT - 1);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32 ad = faddr[(s + 1) & 1] + (s < 1 ? slot : slot_n);   // the NEXT sub-step's operands
        const u32 ad_here = faddr[s] + slot;                            // this sub-step's (block 15 only)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int set = LDSF ? 0 : s;
          const bool V = i * 16 < ACC_V;
          // block i's fragment was the 15th-last read issued (block 15's own: at block 0 of this sub-step)
          if (LDSF) LAB_WAIT_LGKM(14);
          SB;
          if (V) mfma16<true>(acc[i][0], fa[set][i], fb[rb][s][0]); else mfma16<false>(acc[i][0], fa[set][i], fb[rb][s][0]);
          SB;
          if (LDSF) {   // block i - 1 is done with its registers: its next sub-step's fragment (block 15's own arrives during block 0)
            switch (i) {
              case 0: LAB_DS_READ_B128(fa[0][15], ad_here, 15 * 2048); break;
              case 1: LAB_DS_READ_B128(fa[0][0], ad, 0 * 2048); break;
              case 2: LAB_DS_READ_B128(fa[0][1], ad, 1 * 2048); break;
              case 3: LAB_DS_READ_B128(fa[0][2], ad, 2 * 2048); break;
              case 4: LAB_DS_READ_B128(fa[0][3], ad, 3 * 2048); break;
              case 5: LAB_DS_READ_B128(fa[0][4], ad, 4 * 2048); break;
              case 6: LAB_DS_READ_B128(fa[0][5], ad, 5 * 2048); break;
              case 7: LAB_DS_READ_B128(fa[0][6], ad, 6 * 2048); break;
              case 8: LAB_DS_READ_B128(fa[0][7], ad, 7 * 2048); break;
              case 9: LAB_DS_READ_B128(fa[0][8], ad, 8 * 2048); break;
              case 10: LAB_DS_READ_B128(fa[0][9], ad, 9 * 2048); break;
              case 11: LAB_DS_READ_B128(fa[0][10], ad, 10 * 2048); break;
              case 12: LAB_DS_READ_B128(fa[0][11], ad, 11 * 2048); break;
              case 13: LAB_DS_READ_B128(fa[0][12], ad, 12 * 2048); break;
              case 14: LAB_DS_READ_B128(fa[0][13], ad, 13 * 2048); break;
              default: LAB_DS_READ_B128(fa[0][14], ad, 14 * 2048); break;
            }
          }
          SB;
          if (V) mfma16<true>(acc[i][1], fa[set][i], fb[rb][s][1]); else mfma16<false>(acc[i][1], fa[set][i], fb[rb][s][1]);
          SB;
          if (V) mfma16<true>(acc[i][2], fa[set][i], fb[rb][s][2]); else mfma16<false>(acc[i][2], fa[set][i], fb[rb][s][2]);
          SB;
          if (V) mfma16<true>(acc[i][3], fa[set][i], fb[rb][s][3]); else mfma16<false>(acc[i][3], fa[set][i], fb[rb][s][3]);
          SB;
        }
      }
      slot = slot_n;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 7" ::: "memory");   // hipcc pads nothing behind an asm MFMA whose D the sums below read
  SB;
  const long long c1 = __builtin_amdgcn_s_memtime(), w1 = __builtin_amdgcn_s_memrealtime();
  SB;
  u32 sum = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += (u32)acc[i][j][r];
  out[blockIdx.x * 256 + threadIdx.x] = sum;
  if (threadIdx.x == 0) {
    clk[2 * blockIdx.x] = c1 - c0;
    clk[2 * blockIdx.x + 1] = w1 - w0;
  }
}

// ---------------------------------------------------------------------------------------------- host
typedef void (*kern_t)(u32*, int, long long*);
constexpr int NWG = 256;
constexpr size_t LDS_BYTES = (size_t)RING * SLOT;
static u32* g_out;
static long long* g_clk;

static void launch(kern_t k, int iters) { hipLaunchKernelGGL(k, dim3(NWG), dim3(256), LDS_BYTES, 0, g_out, iters, g_clk); }

static u32 checksum(kern_t k, int iters) {
  launch(k, iters);
  CHECK(hipDeviceSynchronize());
  std::vector<u32> h(NWG * 256);
  CHECK(hipMemcpy(h.data(), g_out, h.size() * 4, hipMemcpyDeviceToHost));
  u32 s = 0;   // (wraps; the comparison between the shapes is modulo 2^32)
  for (u32 v : h) s += v;
  return s;
}

static double window(const char* name, int round, kern_t k, int iters) {
  hipEvent_t e0, e1, e2;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1)); CHECK(hipEventCreate(&e2));
  launch(k, iters);
  CHECK(hipEventRecord(e0, 0));
  launch(k, iters);
  CHECK(hipEventRecord(e1, 0));
  CHECK(hipEventSynchronize(e1));
  float one; CHECK(hipEventElapsedTime(&one, e0, e1));
  int n = (int)(2200.0f / one) + 2;
  n += n & 1;
  CHECK(hipEventRecord(e0, 0));
  for (int r = 0; r < n / 2; ++r) launch(k, iters);
  CHECK(hipEventRecord(e1, 0));
  for (int r = 0; r < n / 2; ++r) launch(k, iters);
  CHECK(hipEventRecord(e2, 0));
  CHECK(hipEventSynchronize(e2));
  float first, second;
  CHECK(hipEventElapsedTime(&first, e0, e1)); CHECK(hipEventElapsedTime(&second, e1, e2));
  std::vector<long long> h(2 * NWG);
  CHECK(hipMemcpy(h.data(), g_clk, h.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> ghz(NWG), cyc(NWG);
  for (int b = 0; b < NWG; ++b) { ghz[b] = (double)h[2 * b] / ((double)h[2 * b + 1] * 10.0); cyc[b] = (double)h[2 * b]; }
  std::sort(ghz.begin(), ghz.end()); std::sort(cyc.begin(), cyc.end());
  const double ms = second / (n / 2);
  const double ops = (double)NWG * 4 * iters * (256.0 * 64 * 128 * 2);   // per wavefront and K-step: 256 rows x 64 queries x 128 B
  const double tops = ops / ms * 1e-9;
  printf("round %d  %-14s %8.3f ms/launch (window %.2f s, first half %.3f ms/launch)  %7.1f TOP/s   clock %.3f GHz   %.1f cycles per K-step\n", round, name, ms,
         (first + second) * 1e-3, first / (n / 2), tops, ghz[NWG / 2], cyc[NWG / 2] / iters);
  fflush(stdout);
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1)); CHECK(hipEventDestroy(e2));
  return tops;
}

int main() {
  CHECK(hipMalloc(&g_out, (size_t)NWG * 256 * 4));
  CHECK(hipMalloc(&g_clk, (size_t)NWG * 2 * 8));
  kern_t ks[4] = {loop32<false>, loop16<false>, loop32<true>, loop16<true>};
  const char* names[4] = {"32x32x32 reg", "16x16x64 reg", "32x32x32 lds", "16x16x64 lds"};
  for (kern_t k : ks) CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
  const u32 s32 = checksum(loop32<true>, 8), s16 = checksum(loop16<true>, 8);
  printf("lds loops, 8 K-steps, sum of all accumulators mod 2^32: 32x32x32 %u, 16x16x64 %u  %s\n", s32, s16, s32 == s16 ? "(equal)" : "MISMATCH");
  if (s32 != s16) return 1;
  const int iters = 4000;   // K-steps per launch: 4000 x 2048 matrix cycles, ~4-5 ms
  double t[2][4];
  for (int round = 0; round < 2; ++round)
    for (int v = 0; v < 4; ++v) t[round][v] = window(names[v], round + 1, ks[v], iters);
  for (int round = 0; round < 2; ++round)
    printf("round %d  16x16x64 / 32x32x32: reg %.4f  lds %.4f\n", round + 1, t[round][1] / t[round][0], t[round][3] / t[round][2]);
  printf("spread between rounds of one loop: 32 reg %.4f  16 reg %.4f  32 lds %.4f  16 lds %.4f\n", t[1][0] / t[0][0], t[1][1] / t[0][1], t[1][2] / t[0][2],
         t[1][3] / t[0][3]);
  return 0;
}
