// Search among given rows (eps_index_search_among): the device form of the loops in which VecSearchExecutor::SearchByAttribute judges a primary-key
// list or a geo index's id list row by row (reference: engine/db/execution/vec_search_executor.cpp:966-1013), with a distance and a top-k on top.
//
// The caller holds the candidate ids; the table is not scanned.  among_gather_kernel has flat_scan_kernel's blocking - NQ queries staged in LDS, G
// lanes per row, U rows in flight per group, a k-entry sorted list per wavefront in registers - but takes its row pointers from the list: every
// wavefront walks a contiguous chunk of it, turns each id into a row (an id that names no row takes no part), and evaluates row_dists on it, so
// the sums are the flat scan's bit for bit.  A row may be named several times: lists hold unique keys (insert_unique), and among_merge_kernel
// drops a key it already holds when it merges the wavefronts' lists.  HBM traffic: m * dim * 4 bytes per NQ queries for a list of m entries that
// the whole batch shares, sum of m_j * dim * 4 for per-query lists, plus 8 bytes per id.
#include "kernels.hpp"

namespace eps {

template <int NQ, int KPL, bool VEC4, int U>
__global__ __launch_bounds__(256) void among_gather_kernel(AmongArgs a, int64_t tile0) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int dim = a.dim;
  const int qstride = (dim + 3) & ~3;
  const int64_t q0 = (tile0 + blockIdx.y) * NQ;
  for (int i = threadIdx.x; i < NQ * qstride; i += 256) {
    const int q = i / qstride, c = i - q * qstride;
    const int64_t qq = (q0 + q < a.nq) ? q0 + q : a.nq - 1;
    smem[i] = c < dim ? a.queries[qq * dim + c] : 0.f;
  }
  __syncthreads();

  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int G = group_lanes(dim, VEC4);
  const int RPW = 64 / G;
  const int g = lane / G;
  const int t = lane & (G - 1);
  const int W = a.plan.W;
  const int64_t w = (int64_t)blockIdx.x * AMONG_BLOCK_WAVES + wave;
  int64_t first = 0, len = a.n_cand;
  if (a.offsets) {   // (per-query lists: NQ = 1)
    first = a.offsets[q0];
    len = a.offsets[q0 + 1] - first;
  }
  const int64_t* ids = a.ids + first;
  int64_t begin, end;
  among_chunk(len, a.plan.chunk, w, &begin, &end);
  const u64 base = (u64)a.id_base, stride = (u64)a.id_stride;

  WaveTopK<KPL> list[NQ];
  u64 thr[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    list[q].init();
    thr[q] = KEY_EMPTY;
  }
  u32 given = 0;   // rows of this chunk that got a distance (< 2^31)

  for (int64_t r0 = begin; r0 < end; r0 += RPW * U) {
    const float* rp[U];
    u32 row[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ci = r0 + u * RPW + g;
      const int64_t id = ids[ci < end ? ci : end - 1];
      const u64 off = (u64)id - base;   // (exact wherever id >= id_base)
      u64 r = off;
      bool whole = true;
      if (stride != 1) {   // (wave-uniform)
        r = off / stride;
        whole = r * stride == off;
      }
      ok[u] = ci < end && id >= a.id_base && whole && r < (u64)a.n_rows;
      row[u] = ok[u] ? (u32)r : 0u;   // an id that names no row: row 0's pointer (row_dists' shuffles need every lane), and no offer
      rp[u] = a.rows + (int64_t)row[u] * dim;
    }
    float acc[U][NQ];
    row_dists<U, NQ, VEC4>(rp, smem, qstride, dim, a.metric, G, acc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = (t == 0) && ok[u];
      given += (u32)__popcll(__ballot(valid));
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const u64 key = make_key(finish_dist(a.metric, acc[u][q]), row[u]);
        offer<NQ, KPL>(list, thr, q, key, valid, a.f, a.k, true);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q0 + q < a.nq) list[q].store(a.partial + ((q0 + q) * W + w) * a.k, a.k);   // (a wavefront beyond the list's end: an empty list)
  if (lane == 0 && given) {
    const int64_t served = a.nq - q0 < NQ ? a.nq - q0 : NQ;
    atomicAdd(a.evals, (unsigned long long)given * (unsigned long long)served);
  }
}

template <int NQ, int KPL>
static void launch_among_gather_t(const AmongArgs& a, bool vec4, hipStream_t s) {
  const size_t shm = (size_t)NQ * ((a.dim + 3) & ~3) * sizeof(float);
  for (int64_t tile0 = 0; tile0 < a.plan.tiles; tile0 += AMONG_GRID_Y) {
    const int64_t gy = a.plan.tiles - tile0 < AMONG_GRID_Y ? a.plan.tiles - tile0 : AMONG_GRID_Y;
    const dim3 grid((unsigned)(a.plan.W / AMONG_BLOCK_WAVES), (unsigned)gy);
    if (vec4)
      hipLaunchKernelGGL((among_gather_kernel<NQ, KPL, true, 4>), grid, dim3(256), shm, s, a, tile0);
    else
      hipLaunchKernelGGL((among_gather_kernel<NQ, KPL, false, 4>), grid, dim3(256), shm, s, a, tile0);
  }
}

void launch_among_gather(const AmongArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n_cand <= 0 || a.n_rows <= 0) return;
  const bool vec4 = (a.dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.rows) & 15) == 0);
  const int kpl = pick_kpl(a.k);
  const int nq = a.plan.nq_tile;
#define EPS_CASE(NQ_, KPL_) \
  if (nq == NQ_ && kpl == KPL_) return launch_among_gather_t<NQ_, KPL_>(a, vec4, s);
  EPS_CASE(1, 1) EPS_CASE(2, 1) EPS_CASE(4, 1)
  EPS_CASE(1, 2) EPS_CASE(2, 2) EPS_CASE(4, 2)
  EPS_CASE(1, 4) EPS_CASE(1, 8) EPS_CASE(1, 16)
#undef EPS_CASE
}

// ------------------------------------------------------------------------------------------------
// One workgroup per query: its W partial lists (W * k key slots) into run_keys[q][k].  Equal keys are the same row with the same distance bits: one
// of them stays.  Every partial list holds the unique best k of its chunk, so the unique best k of the union lie among them.
template <int KPL>
__global__ __launch_bounds__(256) void among_merge_kernel(const u64* partial, int slots, int k, u64* run_keys) {
  __shared__ u64 sh[AMONG_BLOCK_WAVES][KPL * 64];
  const int64_t q = blockIdx.x;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const u64* src = partial + q * (int64_t)slots;
  WaveTopK<KPL> L[1];
  u64 thr[1];
  L[0].init();
  thr[0] = KEY_EMPTY;
  const FilterSpec nof = no_filter();   // (the gather judged every key it kept)
  const int rounded = (slots + 255) / 256 * 256;
  for (int i = threadIdx.x; i < rounded; i += 256) {
    const u64 key = i < slots ? src[i] : KEY_EMPTY;
    offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, k, true);
  }
  L[0].store(&sh[wave][0], k);
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < AMONG_BLOCK_WAVES; ++w) {
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      const u64 key = e < k ? sh[w][e] : KEY_EMPTY;
      offer<1, KPL>(L, thr, 0, key, key != KEY_EMPTY, nof, k, true);
    }
  }
  L[0].store(run_keys + q * k, k);
}

void launch_among_merge(const u64* partial, int W, int k, int64_t nq, u64* run_keys, hipStream_t s) {
  if (nq <= 0) return;
  const int kpl = pick_kpl(k);
  const int slots = W * k;   // (<= AMONG_MERGE_KEYS wherever W > AMONG_BLOCK_WAVES; 4 * 1024 otherwise)
#define EPS_CASE(KPL_)                                                                                                      \
  if (kpl == KPL_) {                                                                                                        \
    hipLaunchKernelGGL((among_merge_kernel<KPL_>), dim3((unsigned)nq), dim3(256), 0, s, partial, slots, k, run_keys);      \
    return;                                                                                                                 \
  }
  EPS_CASE(1) EPS_CASE(2) EPS_CASE(4) EPS_CASE(8) EPS_CASE(16)
#undef EPS_CASE
}

}  // namespace eps
