// Search under per-query filters (eps_index_search_filters): a batch in which every query names one of up to 64 compiled filter programs.  Today a
// caller installs program after program and searches each one's queries on their own (P x [set_filter_program + search]), and every one of those
// searches evaluates its program over the table again.  Here the table's attribute rows are judged ONCE for all programs, and the scan that follows
// touches only the rows a query's program lets through.  Ordinary launches on the index's stream; no workgroup waits on another.
//   1. filters_verdict_kernel: one thread per row, SEL_ROWS rows per workgroup.  The pass's programs lie in LDS (24-byte instructions, read as a
//      broadcast: every lane runs the same instruction); a lane takes the standing verdict once (deleted bitset, int-column test, the installed
//      program with @distance = 0), then runs program after program through eval_filter_program - the row's bytes come from HBM once, the
//      programs after the first find them in the cache.  The wavefront's 64 verdicts of program j become one word of plane j, stored with the
//      sense of a deleted bitset (bit set = hidden): any engine can read a plane as FilterSpec::deleted.  Per workgroup and plane: the visible rows.
//   2. filters_scan_kernel: one workgroup per plane turns its block counts into exclusive offsets; the totals go to host-mapped words - the call's
//      one host sync reads them: they are visible_out, the sizes of the lists and the engine choice.
//   3. filters_scatter_kernel (list-engine planes only): select.hip's mbcnt rank - block offset + set bits of the block's earlier words + set bits
//      below the lane - writes the visible rows of plane j as u32 row numbers in row order: list j.
//   4. filters_gather_kernel, the hot path: a variant of among_gather_kernel (among.hip) - its blocking with the id decode and the visibility
//      test taken out and an item table in front; filters_merge_kernel is among_merge_kernel with indexed sources.  A workgroup = up to 4 queries of ONE plane staged in
//      LDS x 4 wavefronts, each over its chunk of the plane's list: G lanes per row, U rows in flight per group, row_dists, one WaveTopK per query
//      in registers.  A row is gathered once per 4 queries of its program (count_j x dim x 4 bytes per block) and no visibility test is left in
//      the loop: the list is the verdict.  The fp32 fma chain of row_dists IS the promise (the bits of a flat search): the matrix instructions
//      reorder and widen the sums, so they have no place in this kernel; a plane that wants them goes to the plane engine instead.
//   5. filters_merge_kernel: one workgroup per query joins the partial lists of its block's wavefronts (their number differs from plane to
//      plane, which among_merge_kernel's arguments cannot say) and writes the k best where the caller's query order wants them.
// HBM traffic: the attribute bytes the programs read, planes x n / 8 bytes of verdicts (read again by the scatter), 4 bytes per list entry written
// and read once per block, count_j x dim x 4 bytes of rows per block of 4 queries.
#include "filters_host.hpp"
#include "kernels.hpp"

namespace eps {

static_assert(SEL_ROWS == 1024 && SEL_THREADS == 256, "a block's 16 words are spread over 4 wavefronts x 4 rounds, and scanned in 16 lanes");
static_assert(sizeof(FilterOp) == 24 && FILTERS_LDS_OPS * sizeof(FilterOp) <= 49152, "a verdict pass's programs fit 48 KB of LDS");

__global__ __launch_bounds__(SEL_THREADS) void filters_verdict_kernel(FiltersVerdictArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  __shared__ int wcnt[SEL_THREADS / 64][FILTERS_MAX_PROGS];
  FilterOp* lops = reinterpret_cast<FilterOp*>(fsm);
  const int o0 = a.off[a.p0], o1 = a.off[a.p1];
  for (int i = threadIdx.x; i < o1 - o0; i += SEL_THREADS) lops[i] = a.ops[o0 + i];
  for (int i = threadIdx.x; i < (SEL_THREADS / 64) * FILTERS_MAX_PROGS; i += SEL_THREADS) (&wcnt[0][0])[i] = 0;
  __syncthreads();
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int64_t first = (int64_t)blockIdx.x * SEL_ROWS;
  FilterSpec pf = no_filter();
  pf.prog_rows = a.rows;
  pf.prog_stride = a.stride;
#pragma unroll 1
  for (int it = 0; it < SEL_ROWS / SEL_THREADS; ++it) {
    const int64_t r = first + it * SEL_THREADS + threadIdx.x;
    const bool standing = r < a.n && row_visible(a.f, (u32)r, 0.f);
#pragma unroll 1
    for (int p = a.p0; p < a.p1; ++p) {
      const int len = a.off[p + 1] - a.off[p];
      bool v = standing;
      if (v && len > 0) {   // (the empty program: every row)
        pf.prog = lops + (a.off[p] - o0);
        pf.prog_len = len;
        v = eval_filter_program(pf, (u32)r, 0.f);
      }
      const u64 vis = __ballot(v);   // bit l: row (first row of the wavefront + l) is visible to plane p (rows >= n: hidden)
      if (lane == 0) {
        a.planes[(int64_t)p * a.plane_words + (r >> 6)] = ~vis;   // (whole blocks: every word of the last block is written)
        wcnt[wave][p] += __popcll(vis);
      }
    }
  }
  __syncthreads();
  for (int p = a.p0 + threadIdx.x; p < a.p1; p += SEL_THREADS) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) s += wcnt[w][p];
    a.counts[(int64_t)p * a.nblocks + blockIdx.x] = (u32)s;
  }
}

// offsets[p][b] = visible rows of plane p in the blocks before b, offsets[p][nblocks] = totals[p] = all of them (n < 2^31).  One workgroup per plane
__global__ __launch_bounds__(SEL_SCAN_THREADS) void filters_scan_kernel(const u32* counts, int64_t nblocks, u32* offsets, u32* totals) {
  constexpr int WAVES = SEL_SCAN_THREADS / 64;
  __shared__ u32 wtot[WAVES];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const u32* cnt = counts + (int64_t)blockIdx.x * nblocks;
  u32* off = offsets + (int64_t)blockIdx.x * (nblocks + 1);
  u32 carry = 0;   // (uniform over the workgroup)
  for (int64_t base = 0; base < nblocks; base += SEL_SCAN_THREADS) {
    const int64_t i = base + threadIdx.x;
    const u32 c = i < nblocks ? cnt[i] : 0u;
    u32 inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u32 up = __shfl_up(inc, o);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const u32 t = wtot[w];
      before += w < wave ? t : 0u;
      all += t;
    }
    if (i < nblocks) off[i] = carry + before + inc - c;
    carry += all;
    __syncthreads();   // (wtot is rewritten by the next round)
  }
  if (threadIdx.x == 0) {
    off[nblocks] = carry;
    totals[blockIdx.x] = carry;
    __threadfence_system();
  }
}

// blockIdx.y: which of the list-engine planes; the plane's visible rows of block blockIdx.x to their ranks in its list
__global__ __launch_bounds__(SEL_THREADS) void filters_scatter_kernel(FiltersScatterArgs a) {
  const int p = a.plane[blockIdx.y];
  const u32* off = a.offsets + (int64_t)p * (a.nblocks + 1);
  const u32 lo = off[blockIdx.x];
  if (off[blockIdx.x + 1] == lo) return;   // nothing visible here
  u32* list = a.lists + a.begin[blockIdx.y];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  // lane l < 16 holds word l of the block (visible sense) and the set bits of words 0 .. l - 1
  const u64 mine = lane < SEL_ROWS / 64 ? ~a.planes[(int64_t)p * a.plane_words + (int64_t)blockIdx.x * (SEL_ROWS / 64) + lane] : 0ull;
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
    if ((word >> lane) & 1ull) list[lo + (u32)(before + below)] = (u32)((int64_t)blockIdx.x * SEL_ROWS + w * 64 + lane);   // (rank < the plane's total)
  }
}

void launch_filters_planes(const FiltersVerdictArgs& a0, const int32_t* pass_begin, int passes, u32* offsets, u32* totals, hipStream_t s) {
  FiltersVerdictArgs a = a0;
  for (int i = 0; i < passes; ++i) {
    a.p0 = pass_begin[i];
    a.p1 = pass_begin[i + 1];
    const size_t shm = (size_t)(a.off[a.p1] - a.off[a.p0]) * sizeof(FilterOp);
    hipLaunchKernelGGL(filters_verdict_kernel, dim3((unsigned)a.nblocks), dim3(SEL_THREADS), shm, s, a);
  }
  hipLaunchKernelGGL(filters_scan_kernel, dim3((unsigned)a.planes_n), dim3(SEL_SCAN_THREADS), 0, s, a.counts, a.nblocks, offsets, totals);
}

void launch_filters_scatter(const FiltersScatterArgs& a, hipStream_t s) {
  if (a.n_lists <= 0 || a.nblocks <= 0) return;
  hipLaunchKernelGGL(filters_scatter_kernel, dim3((unsigned)a.nblocks, (unsigned)a.n_lists), dim3(SEL_THREADS), 0, s, a);
}

// ------------------------------------------------------------------------------------------------
template <int NQ, int KPL, bool VEC4, int U>
__global__ __launch_bounds__(64 * FILTERS_BLOCK_WAVES) void filters_gather_kernel(FiltersGatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const FiltersItem item = a.items[blockIdx.x];
  const FiltersBlock b = a.blocks[item.block];
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  for (int i = threadIdx.x; i < NQ * qstride; i += 64 * FILTERS_BLOCK_WAVES) {
    const int q = i / qstride, c = i - q * qstride;
    const int64_t qq = a.order[b.q0 + (q < b.nq ? q : b.nq - 1)];   // (a block of fewer queries: the last one again, its lists never stored)
    smem[i] = c < dim ? a.queries[qq * dim + c] : 0.f;
  }
  __syncthreads();

  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const int64_t w = (int64_t)item.group * FILTERS_BLOCK_WAVES + wave;   // < b.waves
  const int64_t len = b.list_len;
  const int64_t begin = w * b.chunk < len ? w * b.chunk : len;
  const int64_t end = len - begin < b.chunk ? len : begin + b.chunk;
  const u32* list = a.lists + b.list_begin;

  WaveTopK<KPL> top[NQ];
  u64 thr[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    top[q].init();
    thr[q] = KEY_EMPTY;
  }
  const FilterSpec nof = no_filter();   // the list is the verdict

  for (int64_t r0 = begin; r0 < end; r0 += RPW * U) {
    const float* rp[U];
    u32 row[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ci = r0 + u * RPW + g;
      ok[u] = ci < end;
      row[u] = list[ok[u] ? ci : end - 1];   // (end > begin here: entry end - 1 exists; its row again, and no offer)
      rp[u] = a.rows + (int64_t)row[u] * dim;
    }
    float acc[U][NQ];
    row_dists<U, NQ, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = (t == 0) && ok[u];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const u64 key = make_key(finish_dist(a.metric, acc[u][q]), row[u]);
        offer<NQ, KPL>(top, thr, q, key, valid, nof, a.k, false);   // (a list names a row once)
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q < b.nq) top[q].store(a.partial + (((int64_t)b.wave0 + w) * NQ + q) * a.k, a.k);   // (a wavefront beyond the list's end: an empty list)
}

template <int NQ, int KPL>
static void launch_filters_gather_t(const FiltersGatherArgs& a, bool vec4, hipStream_t s) {
  const size_t shm = (size_t)NQ * ((a.dim + 3) & ~3) * sizeof(float);
  const dim3 grid((unsigned)a.n_items), block(64 * FILTERS_BLOCK_WAVES);
  if (vec4)
    hipLaunchKernelGGL((filters_gather_kernel<NQ, KPL, true, 4>), grid, block, shm, s, a);
  else
    hipLaunchKernelGGL((filters_gather_kernel<NQ, KPL, false, 4>), grid, block, shm, s, a);
}

void launch_filters_gather(const FiltersGatherArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return;
  const bool vec4 = rows_vec4(a.rows, a.dim);
  const int kpl = pick_kpl(a.k);
#define EPS_CASE(NQ_, KPL_) \
  if (a.block_q == NQ_ && kpl == KPL_) return launch_filters_gather_t<NQ_, KPL_>(a, vec4, s);
  EPS_CASE(1, 1) EPS_CASE(2, 1) EPS_CASE(4, 1)
  EPS_CASE(1, 2) EPS_CASE(2, 2) EPS_CASE(4, 2)
  EPS_CASE(1, 4) EPS_CASE(1, 8) EPS_CASE(1, 16)
#undef EPS_CASE
}

// One workgroup per query, by sorted position: the block's `waves` partial lists of this query into run_keys[the caller's query][k].  A query on
// the plane engine (block -1) is not this launch's; a query whose list is empty (no partial list) gets an empty answer.
template <int KPL>
__global__ __launch_bounds__(256) void filters_merge_kernel(FiltersGatherArgs a, u64* run_keys) {
  __shared__ u64 sh[4][KPL * 64];
  const int64_t sq = blockIdx.x;
  const int bi = a.block_of[sq];
  if (bi < 0) return;
  const FiltersBlock b = a.blocks[bi];
  const int qi = (int)(sq - b.q0);
  const int k = a.k;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  WaveTopK<KPL> L[1];
  u64 thr[1];
  L[0].init();
  thr[0] = KEY_EMPTY;
  const FilterSpec nof = no_filter();
  const int slots = b.waves * k;   // (<= FILTERS_MERGE_KEYS)
  const int rounded = (slots + 255) / 256 * 256;
  for (int i = threadIdx.x; i < rounded; i += 256) {
    u64 key = KEY_EMPTY;
    if (i < slots) {
      const int c = i / k, e = i - c * k;
      key = a.partial[(((int64_t)b.wave0 + c) * a.block_q + qi) * k + e];
    }
    offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, k, false);
  }
  L[0].store(&sh[wave][0], k);
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < 4; ++w) {
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      const u64 key = e < k ? sh[w][e] : KEY_EMPTY;
      offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, k, false);
    }
  }
  L[0].store(run_keys + (int64_t)a.order[sq] * k, k);
}

void launch_filters_merge(const FiltersGatherArgs& a, int64_t nq, u64* run_keys, hipStream_t s) {
  if (nq <= 0) return;
  const int kpl = pick_kpl(a.k);
#define EPS_CASE(KPL_)                                                                                          \
  if (kpl == KPL_) {                                                                                            \
    hipLaunchKernelGGL((filters_merge_kernel<KPL_>), dim3((unsigned)nq), dim3(256), 0, s, a, run_keys);        \
    return;                                                                                                     \
  }
  EPS_CASE(1) EPS_CASE(2) EPS_CASE(4) EPS_CASE(8) EPS_CASE(16)
#undef EPS_CASE
}

}  // namespace eps
