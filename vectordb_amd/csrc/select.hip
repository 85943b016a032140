// Filter-only gets on the device: which rows are visible, in ascending row order, windowed by [skip, skip + limit) - the full-scan branch of
// VecSearchExecutor::SearchByAttribute (db/execution/vec_search_executor.cpp:1016-1029) as an order-preserving stream compaction.
// Three ordinary launches on the index's stream; no workgroup ever waits on another (no look-back, no flags): a workgroup that faults or
// leaves early cannot hold up the rest of the machine.
//   1. verdict: one thread per row evaluates row_visible (deleted bitset, int-column test, compiled program with @distance = 0 as
//      LogicalEvaluate(root, id) evaluates it there); the wavefront's 64 verdicts become one word of a visibility bitset (bit set = visible),
//      every block of SEL_ROWS rows also leaves its count.  The program evaluator (a function, a stack of 16 doubles) lives in this launch only.
//   2. scan: ONE workgroup turns the block counts into exclusive offsets (int64) and leaves the total and the window's count.
//   3. scatter: every wavefront re-reads its word; rank of a visible row = block offset + set bits of the block's earlier words + set bits
//      below its lane; rows whose rank falls into the window write their id.  A block wholly outside the window leaves after two loads.
// HBM traffic: the attribute bytes the predicate reads, n / 8 bytes of bitset twice, 12 bytes per block, 8 bytes per id written.
#include "kernels.hpp"

namespace eps {

static_assert(SEL_ROWS == 1024 && SEL_THREADS == 256, "a block's 16 words are spread over 4 wavefronts x 4 rounds, and scanned in 16 lanes");

__global__ __launch_bounds__(SEL_THREADS) void select_verdict_kernel(FilterSpec f, int64_t n, u64* bits, u32* counts) {
  __shared__ int wsum[SEL_THREADS / 64];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int64_t first = (int64_t)blockIdx.x * SEL_ROWS;
  int cnt = 0;   // (wave-uniform)
#pragma unroll 1
  for (int it = 0; it < SEL_ROWS / SEL_THREADS; ++it) {
    const int64_t r = first + it * SEL_THREADS + threadIdx.x;
    const bool visible = r < n && row_visible(f, (u32)r, 0.f);
    const u64 word = __ballot(visible);   // bit l: row (first row of the wavefront + l) is visible (rows >= n: hidden)
    if (lane == 0) bits[r >> 6] = word;   // (the bitset holds whole blocks: every word of the last block is written)
    cnt += __popcll(word);
  }
  if (lane == 0) wsum[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) s += wsum[w];
    counts[blockIdx.x] = (u32)s;
  }
}

// inclusive sum over the lanes of a wavefront
__device__ __forceinline__ int64_t wave_inclusive_sum(int64_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t up = (int64_t)shfl_up64((u64)v, o);
    if (lane >= o) v += up;
  }
  return v;
}

// offsets[b] = visible rows in the blocks before b, offsets[nblocks] = all of them; count_out = clamp(total - skip, 0, limit).  One workgroup:
// SEL_SCAN_THREADS counts per round, the rounds chained through `carry`.
__global__ __launch_bounds__(SEL_SCAN_THREADS) void select_scan_kernel(const u32* counts, int64_t nblocks, int64_t* offsets, int64_t skip, int64_t limit,
                                                                       int64_t* count_out, int64_t* total_out) {
  constexpr int WAVES = SEL_SCAN_THREADS / 64;
  __shared__ int64_t wtot[WAVES];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  int64_t carry = 0;   // (uniform over the workgroup)
  for (int64_t base = 0; base < nblocks; base += SEL_SCAN_THREADS) {
    const int64_t i = base + threadIdx.x;
    const int64_t c = i < nblocks ? (int64_t)counts[i] : 0;
    const int64_t inc = wave_inclusive_sum(c, lane);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int64_t t = wtot[w];
      before += w < wave ? t : 0;
      all += t;
    }
    if (i < nblocks) offsets[i] = carry + before + inc - c;
    carry += all;
    __syncthreads();   // (wtot is rewritten by the next round)
  }
  if (threadIdx.x == 0) {
    offsets[nblocks] = carry;
    const int64_t left = carry - skip;
    count_out[0] = left < 0 ? 0 : (left < limit ? left : limit);
    if (total_out) total_out[0] = carry;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void select_scatter_kernel(const u64* bits, const int64_t* offsets, int64_t skip, int64_t limit, int64_t id_base,
                                                                     int64_t id_stride, int64_t* ids_out) {
  const int64_t lo = offsets[blockIdx.x], hi = offsets[blockIdx.x + 1];
  const int64_t end = skip + limit;   // (the host clamps both to the row count: no overflow)
  if (hi <= skip || lo >= end) return;   // (an empty block: hi == lo, one of the two holds - or it writes nothing below)
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  // lane l < 16 holds word l of the block and the set bits of words 0 .. l - 1
  const u64 mine = lane < SEL_ROWS / 64 ? bits[(int64_t)blockIdx.x * (SEL_ROWS / 64) + lane] : 0ull;
  const int pc = __popcll(mine);
  int inc = pc;
#pragma unroll
  for (int o = 1; o < SEL_ROWS / 64; o <<= 1) {
    const int up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  const int excl = inc - pc;
#pragma unroll
  for (int it = 0; it < SEL_ROWS / SEL_THREADS; ++it) {
    const int w = it * (SEL_THREADS / 64) + wave;
    const u64 word = shfl64(mine, w);
    const int before = __shfl(excl, w);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((u32)(word >> 32), __builtin_amdgcn_mbcnt_lo((u32)word, 0u));   // set bits below this lane
    const int64_t rank = lo + before + below;
    if (((word >> lane) & 1ull) && rank >= skip && rank < end) {
      const int64_t row = (int64_t)blockIdx.x * SEL_ROWS + (int64_t)w * 64 + lane;
      ids_out[rank - skip] = row * id_stride + id_base;
    }
  }
}

void launch_select(const SelectArgs& a, hipStream_t s) {
  const int64_t nblocks = select_blocks(a.n);
  hipLaunchKernelGGL(select_verdict_kernel, dim3((unsigned)nblocks), dim3(SEL_THREADS), 0, s, a.f, a.n, a.bits, a.counts);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_SCAN_THREADS), 0, s, a.counts, nblocks, a.offsets, a.skip, a.limit, a.count_out, a.total_out);
  if (a.limit > 0)
    hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)nblocks), dim3(SEL_THREADS), 0, s, a.bits, a.offsets, a.skip, a.limit, a.id_base, a.id_stride,
                       a.ids_out);
}

}  // namespace eps
