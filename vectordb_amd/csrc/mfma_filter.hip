// Batched flat scan on the matrix cores: the large-batch form of VecSearchExecutor::BruteForceSearch
// (reference: engine/db/execution/vec_search_executor.cpp:717-768), returning the SAME exact answer as the
// fp32 streaming scan.
//
// Idea: at batch b the flat scan is a GEMM, 2*b*N*d flops over N*d row elements.
// gfx950 has no fast fp32/xf32 MFMA (fp32-in MFMA runs at the vector rate), so the GEMM runs on an fp16 mirror
// of the row store with fp32 accumulation and is used only as a LOWER-BOUND FILTER:
//     key(q,x) = |x|^2 - 2 q.x   (L2; -q.x for IP/COSINE)        exact key, dist = key + const(q)
//     approx   = base[x] + s*acc,  acc = sum_k qh_k xh_k         what the MFMA tile produces
//     |key - approx| <= |s| * (|q| * E1[x] + |q - qh| * |xh|)    E1[x] = |x - xh| + gamma*|xh|   (Cauchy-Schwarz +
//                                                                 fp32 accumulation slack), no distributional assumption
// A row can only be in the exact top-k if approx - bound <= T, where T is ANY valid upper bound of the k-th best
// exact key — we use the k-th best exact key found so far.  Rows that pass are re-ranked in exact fp32 by the
// gather kernel (flat_kernels.hip: rerank_kernel).  The scan is staged so T tightens:
//     stage 0: the first S0 rows: their k best approximate keys (same kernel, every row a candidate), re-ranked
//              exactly, give the first T (with a deleted bitset / attribute filter: exact fp32 stream scan instead)
//     stage i: MFMA filter over a geometrically larger chunk          -> candidates -> exact re-rank -> top-k
// Expected candidates per query ~ k * sum_i (chunk_i / rows_before_i): a few hundred at N = 10M, k = 10.
// If a query's candidate buffer overflows (adversarial order/duplicates) the batch falls back to the fp32 scan.
// The bound is a worst-case one (no distributional assumption) for the fp16 rounding and the accumulation order of the
// GEMM; the fp32 rounding of the re-ranked keys it is compared with is covered by a slack that grows with d.
//
// 8-bit first pass (r3).  The matrix pipe multiplies int8 operands at twice the fp16 rate (v_mfma_i32_32x32x32_i8: measured
// 3.42 POP/s against 1.75 PFLOP/s for the fp16 instruction in the same loop, profiles/r3_mfma_peak_i8_vs_fp16.txt), and a
// lower-bound filter may use any operand whose error it can bound.  Rows and queries are quantised on ONE grid per index,
//     xh = z + sx * xi,  xi = clamp(rint((x - z) / sx), -127, 127),   z = (min + max) / 2,  sx = (max - min) / 254
// so that the dot product of the quantised vectors is exact integer arithmetic plus per-row and per-query constants:
//     qh.xh = d z^2 + z sx SX[x] + z sx SQ[q] + sx^2 * sum_k qi_k xi_k          (SX, SQ: sums of the int8 values)
//     approx(q,x) = R[x] + C[q] - u * dot,   u = |s| sx^2,   R, C: the row / query constants (kernels below)
//     |key - approx| <= |s| * (|q| * |x - xh| + |q - qh| * |xh|)                 (Cauchy-Schwarz on the stored residuals; no
//                                                                                 accumulation slack: the int32 sum is exact)
// A row passes iff  dot + acc0[x] >= Tq[q]  with acc0 = ceil(-R/u) folded into the accumulator's start value and
// Tq = floor((C - T)/u): one integer max + compare per 16 outputs, as in the fp16 kernel.  On U[0,1) rows at d = 768 the margin is
// ~2.0 key units (fp16: 0.03) against a spread of 5.5 per sigma of the distance distribution: a few dozen candidates per query
// in the last stage instead of ~10 - noise for the fp32 re-rank.  The kernel is the v7 kernel with the MFMA instruction and the
// accumulator type exchanged (mfma_kernels.hpp, V7Op): a K-step moves the same 128 bytes per row, but covers 128 dimensions
// instead of 64.  Tables the grid does not fit (all values equal, non-finite values, constants beyond int32) and batches whose
// candidate lists overflow fall back to the fp16 engine.
//
// Kernels: mfma_kernels.hpp - v7 (default: persistent, 4 wavefronts x 256 rows x 64 queries per 256 x 256 tile, query
// fragments straight to VGPRs, 4-slot LDS-DMA ring for the row operand) and v3, the fallback for d_pad % 128 != 0 or
// d_pad < 256 (tests/test_gpu_parity.py::test_mfma_engine_is_exact covers d = 33 and d = 100).  Staging, seeds, re-rank and the overflow fallback are the steps of flat_mfma_search_slice below;
// the mirrors are built in mirror_build.hip, a handful of queries take one pass instead (one_pass.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "mirror.hpp"
#include "mfma_kernels.hpp"

namespace eps {

__global__ __launch_bounds__(256) void query_prep_kernel(const float* q, int64_t nq, int64_t b_pad, int dim, int d_pad,
                                                         _Float16* qh, float* qstat) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= b_pad) return;
  const int lane = lane_id();
  _Float16* dst = qh + r * d_pad;
  if (r >= nq) {
    for (int c = lane; c < d_pad; c += 64) dst[c] = (_Float16)0.f;
    if (lane == 0) qstat[r * 4 + 0] = qstat[r * 4 + 1] = qstat[r * 4 + 2] = qstat[r * 4 + 3] = 0.f;
    return;
  }
  const float* src = q + r * dim;
  float s2 = 0.f, e2 = 0.f;
  for (int c = lane; c < d_pad; c += 64) {
    const float x = c < dim ? src[c] : 0.f;
    // A component beyond the fp16 range is stored as +-65504, not +-inf: inf * 0 would make NaN accumulators that fail every
    // `acc >= T` and silently drop rows from an exact answer.  Clamped, the component's residual enters |q - qh| like any
    // other rounding error: the bound stays valid (and becomes so loose that the batch ends on the stream engine).
    const _Float16 h = (_Float16)fminf(fmaxf(x, -65504.f), 65504.f);
    dst[c] = h;
    s2 = fmaf(x, x, s2);
    const float e = x - (float)h;
    e2 = fmaf(e, e, e2);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s2 += __shfl_xor(s2, o);
    e2 += __shfl_xor(e2, o);
  }
  if (lane == 0) {
    qstat[r * 4 + 0] = s2;
    qstat[r * 4 + 1] = sqrtf(s2) * 1.000001f;
    qstat[r * 4 + 2] = sqrtf(e2) * 1.000001f;
    qstat[r * 4 + 3] = 0.f;
  }
}

// T[j]: pass threshold of query j for the next filter launch, from the current k-th best key (formulas: device_common.hpp,
// stage_threshold8 / stage_threshold16).  Also resets what the launch accumulates into (candidate counts, group arrival counters).
// In exact mode a stage's re-rank computes the next stage's thresholds itself (RerankArgs::fuse); these kernels serve the
// approx mode (kNN build), the unseeded staging, and the padding entries.
__global__ void threshold8_kernel(const u64* run_keys, int k, int64_t nq, int64_t b_pad, const float* qstat, const float* scal8, int metric,
                                  float u, int* T, u32* cnt, u32* gsync, float slack, int approx, int pad_only) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b_pad) return;
  if (!pad_only && gsync && j < 256) gsync[j] = 0;   // (all 256 counters, whatever nq: b_pad >= 256)
  if (j >= nq) {
    T[j] = 0x7FFFFFFF;   // padding queries never pass
    return;
  }
  if (pad_only) return;
  cnt[j] = 0;
  const u64 kth = run_keys[j * k + (k - 1)];
  // fewer than k visible rows so far: everything passes (bounded by the candidate cap)
  T[j] = kth == KEY_EMPTY ? -(1 << 30) : stage_threshold8(key_dist(kth), qstat + j * 4, scal8, metric, u, slack, approx);
}

__global__ void threshold_kernel(const u64* run_keys, int k, int64_t nq, int64_t b_pad, const float* qstat,
                                 const float* scal, int metric, float* T, u32* cnt, u32* gsync, float slack, int approx, int pad_only) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b_pad) return;
  if (!pad_only && gsync && j < 256) gsync[j] = 0;
  if (j >= nq) {
    T[j] = -__builtin_inff();
    return;
  }
  if (pad_only) return;
  cnt[j] = 0;
  const u64 kth = run_keys[j * k + (k - 1)];
  T[j] = kth == KEY_EMPTY ? 3.0e38f : stage_threshold16(key_dist(kth), qstat + j * 4, scal, metric, slack, approx);
}


// Start of a seeded call in one launch (three memset nodes cost a single-query call ~50 us): thresholds = +inf, every query's list
// length = the seed count (the dense seed pass writes slot = row), overflow flag and candidate total = 0, group counters = 0.
__global__ void seed_prologue_kernel(u64* T2, int64_t n2, u64 v, u32* cnt, int64_t nq, u32 cntv, u32* gsync) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n2) T2[i] = v;
  if (i < nq) cnt[i] = cntv;
  if (i < 8) cnt[nq + i] = 0;
  if (gsync && i < 256) gsync[i] = 0;
}

// seed sample: the first S/2 rows of the table plus S/2 rows spread evenly over the rest, copied next to each other (a
// positional filter - "only the newest rows" or "only the oldest" - leaves at least half of the seeds' share visible)
__global__ __launch_bounds__(256) void seed_sample_kernel(const _Float16* xh, const u32* base_s, const u32* base, unsigned long long stride,
                                                          u32 head, int d_pad, _Float16* sxh, u32* sbase, u32* sbase_u) {   // (base columns: raw words - fp32 or int32)
  const int64_t i = blockIdx.x;
  const int64_t r = seed_row((u32)i, head, stride);
  const half8* src = reinterpret_cast<const half8*>(xh + r * d_pad);
  half8* dst = reinterpret_cast<half8*>(sxh + i * d_pad);
  for (int c = threadIdx.x; c < d_pad / 8; c += 256) dst[c] = src[c];
  if (threadIdx.x == 0) {
    sbase[i] = base_s[r];
    sbase_u[i] = base[r];
  }
}

// per stage: queries whose candidate list overflowed, and the number of rows that will be re-ranked
__global__ void stage_counts_kernel(const u32* cnt, int64_t nq, int cap, u32* overflow, unsigned long long* total) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nq) return;
  const u32 c = cnt[j];
  if (c > (u32)cap) atomicAdd(overflow, 1u);
  atomicAdd(total, (unsigned long long)(c < (u32)cap ? c : (u32)cap));
}

bool flat_mfma_profitable(Index& ix, int64_t nq, int k, bool count_call) {
  // FLAT_AUTO: both engines return the same bits, so this is purely a cost decision.  The stream scan reads the fp32 rows once
  // per 4 queries; the filter reads its mirror once per <= 2048 queries - the 8-bit mirror is a quarter of the rows' bytes, the
  // fp16 mirror half - and pays ~20 small launches and one host sync per call (bench.py configs c2, 1M x 768, one query: stream
  // 0.72 ms, 8-bit filter 0.48 ms end to end; scripts/bench_midbatch.py, 10M x 768: stream 5.1 / 11.3 / 43.7 ms vs fp16 filter
  // 3.5 / 3.6 / 3.8 ms at 1 / 8 / 32 queries).
  if (ix.n_rows_ < 65536 || k > 128) return false;
  const HalfMirror* m = ix.mirror_;
  const bool have16 = m && m->version == ix.rows_version_;
  const bool known8 = m && m->version8 == ix.rows_version_;
  const bool have8 = known8 && m->i8_ok;
  const bool can16 = !have16 || m->fp16_range_ok;
  if (known8 && !have8 && !can16) return false;                 // neither mirror can serve this table
  // up to 32 queries, k <= 64, rows of <= 1024 bytes: the one-pass search (stream8_kernel.hpp) - one pass over d_pad8 + 4 bytes per row.
  // (an 8-bit mirror not built yet, or behind appended rows, counts as one without folded margins)
  const bool one_pass = one_pass_fits(ix, known8 && m->n8 == ix.n_rows_ ? m : nullptr, nq, k, ix.n_rows_);
  if (nq < 8 && !have8 && !have16) {
    // single-query traffic alone does not get a mirror (n x d bytes of HBM + a pass over the table to build it) at once: r4, after 16 such
    // calls on the same rows it does, where the one-pass search can use it (0.20 ms instead of 0.62 ms per call at 1M x 768).  Only a call
    // with count_call is such a call (a search); any other is judged as the next one would be and leaves the count as it is
    if (count_call && ix.small_calls_version_ != ix.rows_version_) {
      ix.small_calls_version_ = ix.rows_version_;
      ix.small_calls_ = 0;
    }
    if (!one_pass || known8) return false;
    const int calls = (ix.small_calls_version_ == ix.rows_version_ ? ix.small_calls_ : 0) + 1;
    if (count_call) ix.small_calls_ = calls;
    if (calls <= 16) return false;
  }
  const bool use8 = have8 || !known8;                            // (an 8-bit mirror would be built first)
  const double rows = (double)ix.n_rows_, d = (double)ix.dim_;
  const double op_bytes = use8 ? std::max(512.0, std::ceil(d / 256.0) * 256.0) : std::ceil(d / 128.0) * 256.0;   // operand bytes per row
  const double rate = use8 ? 2.0e15 : 1.2e15;                    // matrix rate the filter kernel reaches
  const double dp = use8 ? op_bytes : op_bytes / 2.0;
  const double stream_s = std::ceil((double)nq / 4.0) * rows * d * 4.0 / 6.0e12 + 0.2e-3;
  const double filter_s = (use8 && one_pass)   // (r5: filter programs take the one-pass form too - behind one mask launch; r6: so do tables with folded margins)
                              ? 0.07e-3 + rows * (std::ceil(d / 256.0) * 256.0 + 4.0) / 5.7e12
                              : 0.35e-3 + std::max(rows * op_bytes / 5.0e12, 2.0 * 128.0 * std::ceil((double)nq / 128.0) * rows * dp / rate);
  return filter_s < stream_s;
}

// ------------------------------------------------------------------------------------------------ the staged chain
// rows of the seed pass (unseeded: of the exact head scan)
static int64_t seed_rows(int k) { return std::max<int64_t>(4096, (int64_t)(32 * k + ROWPAD - 1) / ROWPAD * ROWPAD); }

// Staging.  Every MFMA stage needs a valid upper bound T of the final k-th best exact key; it tightens stage by stage.
//  * seeded (exact mode, no deleted bitset / attribute filter): the head [0, S0) goes through the SAME MFMA kernel in
//    its approx-key mode with T = +inf, the k best approximate keys are re-ranked exactly, and their k-th exact key is
//    the first T (any k exact keys bound the k-th best).  The stages then start at row 0; the exact re-rank dedups rows
//    it meets twice.  Stage sizes grow by the cube root of n / S0, which minimises the re-ranked rows ~ k * sum(ratios).
//  * otherwise: the head is scanned exactly (with the filter) by the stream kernel, stages 32 x and 256 x S0.
// Returns the stages' row boundaries: stage st filters rows [bounds[st], bounds[st + 1]).
static std::vector<int64_t> plan_stages(int64_t n, int64_t nq, int k, int64_t b_pad, int cap, bool i8, bool approx, bool seeded) {
  const int64_t S0 = seed_rows(k);
  std::vector<int64_t> bounds;
  if (seeded) {
    bounds.push_back(approx ? S0 : 0);   // approx mode keeps the head's approximate keys themselves: no second visit
    // Stage count.  A stage whose rows outnumber the rows before it by a factor f passes ~ k * c * f candidates per query, c = how
    // many times more rows lie within the bound's margin of the threshold than below it (fp16: ~1; int8: ~4-5 on U[0,1) rows at
    // d = 768); S stages with equal ratios (n / S0)^(1/S) cost S * k * c * (n / S0)^(1/S) candidates and S times the per-stage
    // overhead (launch tails + one re-rank launch, ~0.1 ms at 10M rows).  A candidate costs its wavefront ~900 cycles in the
    // filter's epilogue and 3 KB of gather in the re-rank, so the looser 8-bit bound wants more, smaller steps (measured at
    // 10M x 768, batch 1024: the stage-count sweep in profiles/r3_stage_sweep.txt).
    // Few queries (<= 64): 4 stages.  A call is then a chain of short dependent launches (profiles/r3_single_query_timeline.txt: one
    // query on 1M x 768 = 400 us of back-to-back kernels, 185 us of them the filter stages streaming the mirror once, 110 us seven
    // one-workgroup re-ranks), and two re-ranks less beat the longer lists: scripts/lab/stages_by_batch.py, 1M x 768, p50 ms at
    // 1 / 16 / 64 queries: 0.392 / 0.440 / 0.504 (3 stages), 0.400 / 0.438 / 0.494 (4), 0.431 / 0.466 / 0.515 (6); from 128 queries
    // on 6 stages win (0.648 vs 0.707 with 3), at 10M rows as well.
    // r4, a handful of queries (<= 4): 3 stages - with the centred grid a stage passes half the candidates it used to, and every stage
    // less is one filter launch tail and one one-workgroup re-rank off a chain of dependent launches (scripts/lab/single_query_stages.sh)
    int nstages = i8 ? (nq <= 4 ? 3 : (nq <= 64 ? 4 : 6)) : 3;
    if (i8)   // ... but never so few that a stage's expected k * c * ratio candidates come near the list capacity
      while (nstages < 8 && (double)k * 5.0 * std::pow((double)n / (double)S0, 1.0 / (double)nstages) > 0.5 * (double)cap) ++nstages;
    const double r = std::max(i8 ? 3.0 : 4.0, std::pow((double)n / (double)S0, 1.0 / (double)nstages));
    // stage boundaries on multiples of the rows one "round" of the persistent grid covers (256 workgroups x 256 rows /
    // query tiles), so the small stages do not end on a mostly idle round
    const int64_t qt = std::max<int64_t>(1, b_pad / 256);
    const int64_t unit = 256 * std::max<int64_t>(1, 256 / std::gcd<int64_t>(256, qt));
    double f = 1.0;
    for (int st = 1; st < nstages; ++st) {
      f *= r;
      int64_t bnd = (int64_t)((double)S0 * f) / ROWPAD * ROWPAD;
      if (bnd >= 2 * unit) bnd = bnd / unit * unit;
      if (bnd < n && bnd > bounds.back()) bounds.push_back(bnd);
    }
  } else {
    bounds.push_back(std::min(S0, n));
    for (int64_t bnd : {S0 * 32, S0 * 256}) {
      if (bnd < n && bnd > bounds.back()) bounds.push_back(bnd);
    }
  }
  if (bounds.back() < n) bounds.push_back(n);
  return bounds;
}

// What the steps of one staged call share: filled once by plan_chain, read by every step
struct Chain {
  const float* dq; int64_t nq; int k; u64* run_keys;   // the call
  bool i8;         // operand width of the filter pass: int8 mirror, or fp16 mirror
  bool approx;     // no exact re-rank: the top-k is selected on the approximate keys (kNN-graph construction)
  int64_t n;       // rows the call scans
  bool fold;       // exact mode on a table whose rows differ: per-row margins folded into the start values, thresholds without margin
  bool seeded;     // the first T comes from a seed pass of the filter kernel (with a filter the seeds are the k best VISIBLE head rows)
  bool prologue;   // one launch resets everything a seeded call starts from
  bool gsync;      // the v7 kernel's groups of workgroups meet at arrival counters
  int version;     // filter kernel: v7 wants K-steps in pairs (d_pad % 128 == 0, >= 256); other shapes stay on v3 (the 8-bit mirror is padded for v7)
  int64_t b_pad, S0;
  int cap;         // candidate slots per query and stage
  int d_pad_h;     // row pitch of the operand in 2-byte units (what the kernels count in)
  float u8, slack;
  CallCounters c;
  FilterSpec fs;
  std::vector<int64_t> bounds;
  // 8-bit operands on v7: fragment-major copy + prologue inside query_prep8_kernel - two launches less per call
  bool prep_does_it_all() const { return i8 && version >= 7; }
  // the stages run the 16x16x64 tile (mfma_filter_kernel_v7<2, FM_IDS, true>), which reads its own fragment-major copy; the seed pass keeps qf
  bool tile16() const { return i8 && version >= 7 && nq > 128 && !approx; }
  const float* maxima(const HalfMirror& m) const { return i8 ? (fold ? m.scal8f.as<float>() : m.scal8.as<float>()) : m.scal.as<float>(); }
  u32* group_counters(const HalfMirror& m) const { return gsync ? m.gsync.as<u32>() : nullptr; }
};

static int32_t plan_chain(Index& ix, HalfMirror& m, const float* dq, int64_t nq, int k, u64* run_keys, bool approx, int cap_scale, bool i8, int64_t n, Chain* out) {
  Chain& c = *out = Chain{dq, nq, k, run_keys, i8, approx, n};
  c.b_pad = (nq + BN3 - 1) / BN3 * BN3;
  c.cap = std::max(4096, 64 * k) * cap_scale;
  c.d_pad_h = i8 ? m.d_pad8 / 2 : m.d_pad;
  c.u8 = key_unit8(ix.metric_, m.step8);
  c.slack = rerank_slack(ix.dim_);
  const int64_t b_pad = c.b_pad;
  if (!m.qstat.reserve((size_t)b_pad * 16) || !m.T.reserve((size_t)b_pad * 4) || !m.cand.reserve((size_t)nq * c.cap * 8) ||
      !m.cnt.reserve((size_t)(nq + 4) * 4 + 16) || !m.seedc.reserve((size_t)nq * k * 4) || !(i8 ? m.q8.reserve((size_t)b_pad * m.d_pad8) : m.qh.reserve((size_t)b_pad * m.d_pad * 2)))
    return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory (scratch)");
  c.version = (c.d_pad_h % 128 != 0 || c.d_pad_h < 256) ? 3 : 7;
  if (c.version >= 7 && !m.qf.reserve((size_t)b_pad * c.d_pad_h * 2)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory (scratch)");
  if (c.tile16() && !m.qf16.reserve((size_t)b_pad * c.d_pad_h * 2)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory (scratch)");
  if (!m.gsync.reserve(1024)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory (scratch)");
  c.S0 = seed_rows(k);
  c.seeded = !(tune_int("EPS_MFMA_SEED", 1) == 0) && n > 4 * c.S0;
  c.prologue = c.seeded && c.version >= 7;
  c.gsync = !(tune_int("EPS_MFMA_GROUPSYNC", 1) == 0);
  c.fold = i8 && !approx && m.fold8;
  c.c = call_counters(m.cnt.as<u32>(), nq);
  c.fs = ix.filter_spec();
  c.bounds = plan_stages(n, nq, k, b_pad, c.cap, i8, approx, c.seeded);
  return EPS_OK;
}

// the query operand on the pass's grid (8-bit: also the seeded call's start state and, with folded margins, the batch's start values), row-major
// and - for v7 - fragment-major
static int32_t prepare_queries(Index& ix, HalfMirror& m, const Chain& c) {
  hipStream_t s = ix.stream_;
  if (c.i8) {
    Prep8Extra px;
    if (c.prep_does_it_all()) {
      px.qf = m.qf.as<signed char>();
      if (c.tile16()) px.qf16 = m.qf16.as<signed char>();
      if (c.prologue) {   // thresholds = 0x7F800000 pairs (+inf as fp32; as the 8-bit pass's int32 thresholds: never passes - the padding entries keep it)
        px.T2 = reinterpret_cast<u64*>(m.T.p);
        px.n2 = c.b_pad / 2;
        px.Tv = 0x7F8000007F800000ull;
        px.cnt = c.c.cnt;
        px.cntv = (u32)c.S0;
        px.gsync = c.group_counters(m);
      }
    }
    const hipError_t er = prep8_queries(m, c.fold, (int)ix.dim_, ix.metric_, c.dq, c.nq, c.b_pad, m.q8.as<signed char>(), m.qstat.as<float>(), px, s);
    if (er != hipSuccess) return ix.hip_fail(er, "memset");
    if (c.fold) ix.stats_.i8_folded = 1;
    ix.stats_.i8_rotated = m.rot8 ? 1 : 0;
  } else {
    hipLaunchKernelGGL(query_prep_kernel, dim3((unsigned)((c.b_pad + 3) / 4)), dim3(256), 0, s, c.dq, c.nq, c.b_pad, (int)ix.dim_,
                       m.d_pad, m.qh.as<_Float16>(), m.qstat.as<float>());
  }
  if (c.version >= 7 && !c.prep_does_it_all())
    hipLaunchKernelGGL(pack_qf_kernel, dim3((unsigned)((c.b_pad / 32) * (c.d_pad_h / 16))), dim3(64), 0, s, m.qh.as<_Float16>(), m.qf.as<_Float16>(), c.b_pad, c.d_pad_h);
  return EPS_OK;
}

static FilterArgs filter_args(const Index& ix, const HalfMirror& m, const Chain& c) {
  const bool i8 = c.i8;
  FilterArgs fa;
  fa.xh = i8 ? reinterpret_cast<const _Float16*>(m.x8.p) : m.xh.as<_Float16>();
  fa.qh = i8 ? reinterpret_cast<const _Float16*>(m.q8.p) : m.qh.as<_Float16>();   // the query operand, row-major
  fa.qf = m.qf.as<_Float16>();
  // (8-bit: int32 words, only ever moved; exact mode: the batch's folded start values)
  fa.base = i8 ? (c.fold ? m.acc0b.as<float>() : m.acc0.as<float>()) : (ix.metric_ == 0 ? m.xn.as<float>() : m.zeros.as<float>());
  fa.base_s = i8 ? (c.fold ? m.acc0b.as<float>() : m.acc0.as<float>()) : (ix.metric_ == 0 ? m.xn_s.as<float>() : m.zeros_s.as<float>());
  fa.T = m.T.as<float>();
  fa.d_pad = c.d_pad_h;
  fa.tiles_q = (int)(c.b_pad / BN3);
  fa.nq = c.nq;
  fa.s = i8 ? -c.u8 : (ix.metric_ == 0 ? -2.f : -1.f);
  fa.inv_s = 1.f / fa.s;
  fa.cand = m.cand.as<u32>();
  fa.cand_keys = c.approx ? m.cand.as<u64>() : nullptr;
  fa.qstat = m.qstat.as<float>();
  fa.metric = ix.metric_;
  fa.cnt = c.c.cnt;
  fa.cap = c.cap;
  fa.group_sync = nullptr;
  fa.sync_shift = std::min(8, std::max(0, tune_int("EPS_MFMA_SYNC_SHIFT", 2)));
  fa.dense = 0;
  return fa;
}

constexpr size_t V3_LDS_BYTES = 2 * 65536 + 2 * 256 * sizeof(float);

// once per index (= per device: no process-wide state): the persistent grid's size, the kernels' LDS allowance
static void ensure_filter_kernels(const Index& ix, HalfMirror& m) {
  if (m.num_cus) return;
  hipDeviceProp_t prop;
  m.num_cus = hipGetDeviceProperties(&prop, ix.device_) == hipSuccess ? prop.multiProcessorCount : 256;
  m.num_cus = m.num_cus / 8 * 8;
  if (m.num_cus < 8) m.num_cus = 8;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mfma_filter_kernel_v3), hipFuncAttributeMaxDynamicSharedMemorySize, (int)V3_LDS_BYTES);
  for (const void* fn : {reinterpret_cast<const void*>(mfma_filter_kernel_v7<2, FM_IDS>), reinterpret_cast<const void*>(mfma_filter_kernel_v7<2, FM_KEYS>),
                         reinterpret_cast<const void*>(mfma_filter_kernel_v7<2, FM_DENSE>), reinterpret_cast<const void*>(mfma_filter_kernel_v7<1, FM_IDS>),
                         reinterpret_cast<const void*>(mfma_filter_kernel_v7<1, FM_KEYS>), reinterpret_cast<const void*>(mfma_filter_kernel_v7<1, FM_DENSE>),
                         reinterpret_cast<const void*>(mfma_filter_kernel_v7<2, FM_IDS, true>), reinterpret_cast<const void*>(mfma_filter_kernel_v7<2, FM_KEYS, true>),
                         reinterpret_cast<const void*>(mfma_filter_kernel_v7<2, FM_DENSE, true>), reinterpret_cast<const void*>(mfma_filter_kernel_v7<1, FM_IDS, true>),
                         reinterpret_cast<const void*>(mfma_filter_kernel_v7<1, FM_KEYS, true>), reinterpret_cast<const void*>(mfma_filter_kernel_v7<1, FM_DENSE, true>)})
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)V7_LDS_BYTES);
}

template <int JQ, bool I8>
static void launch_v7(const FilterArgs& f, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  if (f.dense) hipLaunchKernelGGL((mfma_filter_kernel_v7<JQ, FM_DENSE, I8>), grid, block, V7_LDS_BYTES, s, f);
  else if (f.cand_keys) hipLaunchKernelGGL((mfma_filter_kernel_v7<JQ, FM_KEYS, I8>), grid, block, V7_LDS_BYTES, s, f);
  else hipLaunchKernelGGL((mfma_filter_kernel_v7<JQ, FM_IDS, I8>), grid, block, V7_LDS_BYTES, s, f);
}

// one filter pass over the row tiles [f.tile0, f.tile0 + f.ntiles): the seed pass (f.dense) or a stage
static void launch_filter(const HalfMirror& m, const Chain& c, FilterArgs f, hipStream_t s) {
  const dim3 grid((unsigned)m.num_cus);
  if (c.version < 7) {
    hipLaunchKernelGGL(mfma_filter_kernel_v3, grid, dim3(512), V3_LDS_BYTES, s, f);
    return;
  }
  f.group_sync = c.group_counters(m);
  if (c.tile16() && !f.dense && !f.cand_keys) f.qf = m.qf16.as<_Float16>();
  if (f.group_sync && f.dense && !c.prologue) (void)hipMemsetAsync(f.group_sync, 0, 1024, s);   // (stages: reset by threshold_kernel / the re-rank)
  if (c.nq <= 128) {   // one 128-query tile: half the padded MFMA work, the pass streams the mirror
    f.tiles_q = 1;
    if (c.i8) launch_v7<1, true>(f, grid, s); else launch_v7<1, false>(f, grid, s);
  } else {
    if (c.i8) launch_v7<2, true>(f, grid, s); else launch_v7<2, false>(f, grid, s);
  }
}

// The seed pass: the k best approximate keys of S0 rows.  Approx mode keeps them (the head's keys); exact mode takes the rows from a sample
// spread over the whole table and re-ranks them exactly - their k-th exact key gives the first stage's thresholds.
static int32_t run_seed_pass(Index& ix, HalfMirror& m, const Chain& c, const FilterArgs& fa, RerankArgs ra) {
  hipStream_t s = ix.stream_;
  const bool i8 = c.i8;
  const int64_t S0 = c.S0;
  u32* cnt = c.c.cnt;
  const bool dense = c.version >= 7;   // v7 writes the head's keys densely (slot = row); older kernels append with atomics
  if (c.prologue && c.prep_does_it_all()) {
    // (query_prep8_kernel laid the start state down)
  } else if (c.prologue) {
    const int64_t cells = std::max<int64_t>(std::max<int64_t>(c.b_pad / 2, c.nq), 256);
    hipLaunchKernelGGL(seed_prologue_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, reinterpret_cast<u64*>(m.T.p), c.b_pad / 2, 0x7F8000007F800000ull,
                       cnt, c.nq, (u32)S0, c.group_counters(m));
  } else {
    launch_fill_u64(reinterpret_cast<u64*>(m.T.p), c.b_pad / 2, 0x7F8000007F800000ull, s);   // T = +inf: every head row is a candidate
    const hipError_t er = dense ? hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cnt), (int)S0, (size_t)c.nq, s) : hipMemsetAsync(cnt, 0, (size_t)c.nq * 4, s);
    if (er != hipSuccess) return ix.hip_fail(er, "memset");
  }
  unsigned long long seed_stride = 0;   // != 0: the seed pass ran over the sample, ids are sample indices
  u32 seed_head = 0;
  FilterArgs f0 = fa;
  f0.dense = dense ? 1 : 0;
  f0.cand_keys = m.cand.as<u64>();
  if (!c.approx) {   // exact mode: seeds from a sample spread over the whole table (approx mode keeps the head's keys)
    const u32 sample_head = (u32)(S0 / 2);
    const unsigned long long sample_stride = (unsigned long long)(((unsigned __int128)(c.n - sample_head) << 32) / (unsigned __int128)(S0 - sample_head));
    // (one sample per operand width)
    int64_t& smp_version = i8 ? m.sample8_version : m.sample_version;
    int64_t& smp_n = i8 ? m.sample8_n : m.sample_n;
    int64_t& smp_rows = i8 ? m.sample8_rows : m.sample_rows;
    DevBuf& smp_x = i8 ? m.sx8 : m.sxh;
    DevBuf& smp_base = i8 ? m.sacc0 : m.sbase;
    DevBuf& smp_base_u = i8 ? m.sacc0 : m.sbase_u;
    if (smp_version != ix.rows_version_ || smp_n != c.n || smp_rows != S0) {   // (also after an append: n changed)
      if (!smp_x.reserve((size_t)S0 * c.d_pad_h * 2) || !smp_base.reserve((size_t)S0 * 4) || !smp_base_u.reserve((size_t)S0 * 4))
        return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory (seed sample)");
      // (8-bit: the sample keeps the UNFOLDED start values - the dense seed pass ranks approximate keys and tests nothing - so it stays
      // valid from batch to batch)
      hipLaunchKernelGGL(seed_sample_kernel, dim3((unsigned)S0), dim3(256), 0, s, fa.xh, i8 ? m.acc0.as<u32>() : reinterpret_cast<const u32*>(fa.base_s),
                         i8 ? m.acc0.as<u32>() : reinterpret_cast<const u32*>(fa.base),
                         sample_stride, sample_head, c.d_pad_h, smp_x.as<_Float16>(), smp_base.as<u32>(), smp_base_u.as<u32>());
      smp_version = ix.rows_version_;
      smp_n = c.n;
      smp_rows = S0;
    }
    f0.xh = smp_x.as<_Float16>();
    f0.base_s = smp_base.as<float>();
    f0.base = smp_base_u.as<float>();
    seed_stride = sample_stride;
    seed_head = sample_head;
  }
  f0.tile0 = 0;
  f0.ntiles = (S0 + BM3 - 1) / BM3;
  f0.row_hi = S0;
  launch_filter(m, c, f0, s);
  // k best approximate keys of the visible seeds; exact mode: straight to the candidate lists of the re-rank that follows (the
  // dense seed keys live in the upper half of the candidate buffer's u64 view, the lists in its u32 view: disjoint for cap >= 2 k)
  if (c.approx) {
    launch_merge_lists(f0.cand_keys, c.cap, c.k, c.nq, c.run_keys, false, s, cnt, nullptr, seed_stride, seed_head);
    return EPS_OK;
  }
  // (merge_lists reads a query's seed count before it writes the candidate count there; the re-rank zeroes it)
  launch_merge_lists(f0.cand_keys, c.cap, c.k, c.nq, c.run_keys, false, s, cnt, &c.fs, seed_stride, seed_head, m.seedc.as<u32>(), c.k, cnt);
  ra.cand = m.seedc.as<u32>();
  ra.cap = c.k;
  ra.fuse = 2;          // (thresholds of the first stage; the seeds are not a stage's candidates)
  ra.T_next = m.T.p;
  launch_rerank(ra, s);   // -> their exact keys
  return EPS_OK;
}

// EPS_DEBUG: a stage's candidate counts and thresholds
static void dump_stage(const HalfMirror& m, const Chain& c, size_t st, int64_t ntiles, hipStream_t s) {
  const int64_t nq = c.nq;
  const int k = c.k;
  std::vector<u32> hc((size_t)nq);
  std::vector<float> hT((size_t)nq);
  std::vector<u64> hk((size_t)nq * k);
  (void)hipMemcpyAsync(hc.data(), c.c.cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  (void)hipMemcpyAsync(hT.data(), m.T.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  (void)hipMemcpyAsync(hk.data(), c.run_keys, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s);
  (void)hipStreamSynchronize(s);
  u32 mn = ~0u, mx = 0; double sum = 0; float tmin = 3e38f, tmax = -3e38f; int64_t empt = 0, big = 0;
  for (int64_t j = 0; j < nq; ++j) { mn = std::min(mn, hc[j]); mx = std::max(mx, hc[j]); sum += hc[j]; tmin = std::min(tmin, hT[j]); tmax = std::max(tmax, hT[j]); empt += hk[j * k + k - 1] == KEY_EMPTY; big += hc[j] > (u32)c.cap; }
  fprintf(stderr, "[eps] stage %zu rows [%lld,%lld) tiles %lld: cnt min %u mean %.1f max %u (>cap: %lld), T min %g max %g, empty kth %lld, scal %g %g %g\n", st, (long long)c.bounds[st], (long long)c.bounds[st + 1], (long long)ntiles, mn, sum / nq, mx, (long long)big, tmin, tmax, (long long)empt, m.h_scal[0], m.h_scal[1], m.h_scal[2]);
}

// Stage st: thresholds (where the previous re-rank did not leave them), the filter pass over its rows, and the exact re-rank of what passed
// (approx mode: the selection on the approximate keys).  *fin_done: the call's last re-rank wrote the caller-visible result.
static void run_stage(Index& ix, HalfMirror& m, const Chain& c, size_t st, FilterArgs fa, RerankArgs ra, bool* fin_done) {
  hipStream_t s = ix.stream_;
  const int64_t lo = c.bounds[st], hi = c.bounds[st + 1];
  const bool fused = !c.approx;   // exact mode: every re-rank also does its stage's counts and the next stage's thresholds
  // thresholds of this stage: from the previous re-rank (fused), except for the padding entries (once), the approx mode and
  // the unseeded staging (whose stage 0 was a stream scan)
  const bool have_T = fused && (st > 0 || c.seeded);
  const int pad_only = have_T ? 1 : 0;
  // (8-bit, seeded: the prologue left 0x7F800000 in the padding entries - as an int32 threshold "never passes" - and the dense
  // seed pass does not read thresholds, so the pad-only launch is not needed)
  if ((!have_T || st == 0) && !(have_T && c.i8 && c.prologue)) {
    const dim3 grid((unsigned)((c.b_pad + 255) / 256));
    if (c.i8)
      hipLaunchKernelGGL(threshold8_kernel, grid, dim3(256), 0, s, c.run_keys, c.k, c.nq, c.b_pad, m.qstat.as<float>(), c.maxima(m), ix.metric_, c.u8, m.T.as<int>(), c.c.cnt,
                         m.gsync.as<u32>(), c.slack, c.approx ? 1 : 0, pad_only);
    else
      hipLaunchKernelGGL(threshold_kernel, grid, dim3(256), 0, s, c.run_keys, c.k, c.nq, c.b_pad, m.qstat.as<float>(), c.maxima(m), ix.metric_, m.T.as<float>(), c.c.cnt,
                         m.gsync.as<u32>(), c.slack, c.approx ? 1 : 0, pad_only);
  }
  fa.tile0 = lo / BM3;
  fa.ntiles = (hi + BM3 - 1) / BM3 - fa.tile0;
  fa.row_hi = hi;
  const bool biggest = (st + 2 == c.bounds.size());
  if (biggest) {
    (void)hipEventRecord(ix.evk0_, s);
    ix.stats_.main_kernel_rows = hi - lo;
    ix.stats_.main_kernel_queries = c.nq;
    ix.stats_.main_kernel_bits = c.i8 ? 8 : 16;
  }
  // (timed for throughput-sized batches only: an event record between two dependent launches costs a single-query chain ~4 us per
  // launch boundary; the build's kNN stage runs thousands of calls: untimed)
  const int sev = (!c.approx && c.nq >= 256 && ix.stage_n_ < Index::STAGE_EV) ? ix.stage_n_++ : -1;
  if (sev >= 0) (void)hipEventRecord(ix.stage_ev_[sev][0], s);
  launch_filter(m, c, fa, s);
  if (sev >= 0) {
    (void)hipEventRecord(ix.stage_ev_[sev][1], s);
    ix.stats_.filter_rows_all += hi - lo;
  }
  if (biggest) (void)hipEventRecord(ix.evk1_, s);
  if (!fused) hipLaunchKernelGGL(stage_counts_kernel, dim3((unsigned)((c.nq + 255) / 256)), dim3(256), 0, s, c.c.cnt, c.nq, c.cap, c.c.overflow, c.c.total);
  if (tune_env("EPS_DEBUG")) dump_stage(m, c, st, fa.ntiles, s);
  if (c.approx) {
    launch_merge_lists(fa.cand_keys, c.cap, c.k, c.nq, c.run_keys, true, s, c.c.cnt);  // select on the approximate keys
    return;
  }
  ra.fuse = 3;                                                            // this stage's counts + the next stage's thresholds
  ra.T_next = (st + 2 < c.bounds.size()) ? m.T.p : nullptr;
  // the last re-rank writes the caller-visible result itself (rewritten by a fall-back pass if the lists overflowed)
  const bool fin_here = biggest && finalize_in_rerank(ix, c.nq, &ra);
  launch_rerank(ra, s);
  if (fin_here) {
    (void)hipEventRecord(ix.ev1_, s);
    ix.result_finalized_ = true;
    *fin_done = true;
  }
}

static hipError_t read_counters(const CallCounters& c, hipStream_t s, CountersRead* h) {
  hipError_t er = hipMemcpyAsync(&h->overflow, c.overflow, 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(&h->total, c.total, 8, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  return er;
}

// What answers a batch that this attempt did not, in the order of preference
enum class Fallback { none, fp16, wide_lists, stream };

// The library's own choice of the 8-bit pass is PROBED once per mirror, after the first stage: every stage passes ~ k * c * ratio candidates per
// query (c = how many times more rows lie within the bound's margin of the threshold than below it), so the first, smallest stage
// predicts the others.  Where c is large - rows whose neighbours are close against the value range: low intrinsic dimension,
// tight clusters - the lists of the big stages would overflow and the batch would pay the 8-bit attempt AND the fp16 pass
// (r3: 10M x 768 manifold set 73 k -> 39 k q/s); here it pays one small stage and one sync, once.
static Fallback resolve_probe(Index& ix, HalfMirror& m, const Chain& c, const CountersRead& h) {
  if (!(h.overflow || h.total > (unsigned long long)c.nq * (unsigned long long)c.cap / 6)) {
    m.i8_trusted = true;
    return Fallback::none;
  }
  // declined for this mirror (re-attaching rows re-arms it; EPS_FLAT_MFMA_I8 still forces it) - unless a deleted bitset or a filter is
  // active: a selective filter inflates the lists by 1 / (its pass fraction) whatever the bound is worth, so such a batch only
  // decides for itself and the next one probes again
  if (!(c.fs.deleted || c.fs.column || c.fs.prog)) m.i8_overflows = 3;
  ix.stats_.i8_declined += 1;
  return Fallback::fp16;
}

// The whole chain has run: h.overflow queries lost candidates to a full list (selective filters inflate the lists by 1 / pass fraction,
// adversarial row orders by more).  8-bit pass: its looser bound let too much through - the fp16 pass; fp16 pass: once more with 16 x the
// candidate slots - re-ranking tens of thousands of rows per query is still ~50 x cheaper than the stream scan of a large batch - then
// the exact stream engine.  (Approx mode keeps what it has.)
static Fallback resolve_overflow(HalfMirror& m, const Chain& c, int cap_scale, const CountersRead& h) {
  if (!h.overflow || c.approx) {
    if (c.i8) m.i8_overflows = 0;
    return Fallback::none;
  }
  if (c.i8) {
    m.i8_overflows += 1;
    m.i8_trusted = false;
    return Fallback::fp16;
  }
  if (cap_scale == 1 && (size_t)c.nq * c.cap * 16 * 8 <= ((size_t)4 << 30)) return Fallback::wide_lists;
  return Fallback::stream;
}

int32_t flat_mfma_search_slice(Index& ix, const float* dq, int64_t nq, int k, u64* run_keys, bool approx, int cap_scale, int bits, bool auto_bits) {
  // operand width of the filter pass: 8 = int8 mirror (when the table fits its grid), 16 = fp16 mirror
  bool i8 = bits == 8;
  int32_t rc = EPS_OK;
  if (i8) {
    rc = ensure_mirror8(ix);
    if (rc != EPS_OK) return rc;
    // a table whose 8-bit bound is too loose to filter (an outlier stretches the grid, rows far outside it) overflows on every
    // batch: after three in a row the library's own choice stops paying for the 8-bit pass first (an explicit EPS_FLAT_MFMA_I8
    // request still gets it; re-attaching rows re-arms it)
    if (!ix.mirror_->i8_ok || (auto_bits && ix.mirror_->i8_overflows >= 3)) i8 = false;
  }
  if (i8 && !approx && cap_scale == 1 && nq <= S8_MAX_Q) {
    bool done = false;
    rc = flat_stream8_slice(ix, dq, nq, k, run_keys, &done);
    if (rc != EPS_OK || done) return rc;
  }
  if (!i8) {
    rc = ensure_mirror(ix);
    if (rc != EPS_OK) return rc;
  }
  HalfMirror& m = *ix.mirror_;
  const int64_t n = ix.scan_limit_ >= 0 ? std::min(ix.scan_limit_, ix.n_rows_) : ix.n_rows_;
  // values beyond the fp16 range: the filter bound would be vacuous; the exact stream engine takes over
  if (!i8 && !m.fp16_range_ok) return ix.flat_stream(dq, nq, k, 0, n, run_keys, -1, !approx);
  auto fall_back = [&](Fallback to) -> int32_t {
    if (to == Fallback::fp16) return flat_mfma_search_slice(ix, dq, nq, k, run_keys, approx, 1, 16, false);
    if (to == Fallback::wide_lists) return flat_mfma_search_slice(ix, dq, nq, k, run_keys, approx, 16, 16, false);
    return ix.flat_stream(dq, nq, k, 0, n, run_keys);
  };
  hipStream_t s = ix.stream_;
  Chain c;
  rc = plan_chain(ix, m, dq, nq, k, run_keys, approx, cap_scale, i8, n, &c);
  if (rc == EPS_OK) rc = prepare_queries(ix, m, c);
  if (rc == EPS_OK && !c.seeded) rc = ix.flat_stream(dq, nq, k, 0, c.bounds[0], run_keys, -1, !approx);   // stage 0: exact scan of the head
  if (rc != EPS_OK) return rc;
  ix.stats_.main_kernel_launches = 0;
  m.s8_clean_cnt = nullptr;   // (the chain's counters live where the one-pass form keeps its own)
  hipError_t er = c.prologue ? hipSuccess : hipMemsetAsync(c.c.overflow, 0, 32, s);
  if (er != hipSuccess) return ix.hip_fail(er, "memset");
  const FilterArgs fa = filter_args(ix, m, c);
  // stage bookkeeping folded into the re-rank (exact mode): counts of the stage it follows + thresholds of the stage that follows it
  RerankArgs ra = rerank_args(ix, m, dq, nq, k, c.fs, c.cap, run_keys, c.c, c.maxima(m), i8 ? 8 : 16);
  ra.fuse = approx ? 0 : 1;
  ra.gsync = m.gsync.as<u32>();
  ensure_filter_kernels(ix, m);
  if (c.seeded) {
    rc = run_seed_pass(ix, m, c, fa, ra);
    if (rc != EPS_OK) return rc;
  }
  bool fin_done = false;
  const bool probe = i8 && auto_bits && !approx && c.seeded && !m.i8_trusted && c.bounds.size() > 3 && !(tune_int("EPS_MFMA_PROBE", 1) == 0);
  CountersRead h;
  for (size_t st = 0; st + 1 < c.bounds.size(); ++st) {
    run_stage(ix, m, c, st, fa, ra, &fin_done);
    if (probe && st == 0) {
      er = read_counters(c.c, s, &h);
      if (er != hipSuccess) return ix.hip_fail(er, "MFMA filter (probe)");
      const Fallback to = resolve_probe(ix, m, c, h);
      if (to != Fallback::none) return fall_back(to);
    }
  }
  er = hipGetLastError();
  if (er != hipSuccess) return ix.hip_fail(er, "MFMA filter launch");
  if (!fin_done && ix.call_.pre_sync && !approx && nq == ix.call_.nq) ix.call_.pre_sync();   // (speculative: a fall-back pass below converts again)
  er = read_counters(c.c, s, &h);
  if (er != hipSuccess) return ix.hip_fail(er, "MFMA filter");
  ix.stats_.rerank_rows += (int64_t)h.total;
  ix.stats_.dist_evals += nq * (n - c.bounds[0]) + (c.seeded ? nq * c.S0 : 0);   // (exact mode visits the head twice)
  ix.stats_.main_kernel_launches = 1;
  if (h.overflow) {
    ix.result_finalized_ = false;   // (whatever was converted before the sync is stale: a pass below rewrites the result keys)
    ix.stats_.overflow_queries += h.overflow;
  }
  const Fallback to = resolve_overflow(m, c, cap_scale, h);
  return to == Fallback::none ? EPS_OK : fall_back(to);
}

// Batches beyond 2048 queries run as slices of 2048: the kernel keeps one slice's fp16 query tile set (3 MB) resident in
// each XCD's 4 MB L2 while the row operand streams past; at 4096 / 8192 queries per pass the query fragments thrash L2
// and the filter drops to 0.37 / 0.27 of the MFMA peak (0.46 in slices; bench.py --rows 1250000 --batch 8192).
int32_t flat_mfma_search(Index& ix, const float* dq, int64_t nq, int k, u64* run_keys, bool approx, int bits) {
  if (ix.n_rows_ <= 0) return ix.flat_stream(dq, nq, k, 0, 0, run_keys);   // (nothing to mirror)
  const bool auto_bits = bits != 8 && bits != 16;
  if (auto_bits) bits = 8;   // the library's choice: 8-bit first pass - tables it cannot serve fall back by themselves
  const int64_t slice = std::max(256, tune_int("EPS_MFMA_MAX_BATCH", 2048));
  if (nq <= slice) return flat_mfma_search_slice(ix, dq, nq, k, run_keys, approx, 1, bits, auto_bits);
  for (int64_t q0 = 0; q0 < nq; q0 += slice) {   // the counters in ix.stats_ accumulate over the slices
    const int32_t rc = flat_mfma_search_slice(ix, dq + q0 * ix.dim_, std::min(slice, nq - q0), k, run_keys + q0 * k, approx, 1, bits, auto_bits);
    if (rc != EPS_OK) return rc;
  }
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ stages on their own (tests)
// eps_index_mirror_view / eps_index_filter_pass (include/epsilla_gfx950.h): what the build and the preparation kernels store, and what ONE
// filter launch lets through, handed to a test that compares them with an fp64 reference.  Both run the chain's own steps (plan_chain,
// prepare_queries, filter_args, launch_filter) and leave nothing behind that a later search could see.
namespace {
// the call's statistics and the one-pass search's "clean state" as a probe must leave them
struct ProbeGuard {
  Index& ix;
  eps_search_stats keep;
  explicit ProbeGuard(Index& i) : ix(i), keep(i.stats_) {}
  ~ProbeGuard() {
    ix.stats_ = keep;
    if (ix.mirror_) ix.mirror_->s8_clean_cnt = nullptr;   // (a probe writes the counters the one-pass form keeps its own in: its next call starts with the prep launch)
  }
};
u64 host_key(float dist) {   // make_key(dist, 0) on the host
  dist += 0.0f;
  if (dist != dist) return (u64)ORD_NAN << 32;   // (one ordinal for every NaN, as make_key)
  u32 u;
  std::memcpy(&u, &dist, 4);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return (u64)u << 32;
}
int32_t upload_queries(Index& ix, const float* hq, int64_t nq, DevBuf* dq) {
  if (!dq->reserve((size_t)nq * ix.dim_ * 4)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "out of device memory (queries)");
  const hipError_t er = hipMemcpyAsync(dq->p, hq, (size_t)nq * ix.dim_ * 4, hipMemcpyHostToDevice, ix.stream_);
  return er == hipSuccess ? EPS_OK : ix.hip_fail(er, "memcpy (queries)");
}
int32_t ensure_probe_mirror(Index& ix, bool i8) {
  if (ix.n_rows_ <= 0) return ix.fail(EPS_USER_ERROR, "no rows attached");
  return i8 ? ensure_mirror8(ix) : ensure_mirror(ix);
}
}  // namespace

int32_t flat_mirror_view(Index& ix, int bits, const float* hq, int64_t nq, eps_mirror_view* v) {
  if (bits != 8 && bits != 16) return ix.fail(EPS_USER_ERROR, "mirror_view: bits must be 8 or 16");
  if (nq < 0 || nq > 2048 || (nq > 0 && !hq)) return ix.fail(EPS_USER_ERROR, "mirror_view: 0 .. 2048 host queries");
  const bool i8 = bits == 8;
  int32_t rc = ensure_probe_mirror(ix, i8);
  if (rc != EPS_OK) return rc;
  HalfMirror& m = *ix.mirror_;
  hipStream_t s = ix.stream_;
  v->n = i8 ? m.n8 : m.n;
  v->n_pad = i8 ? m.n_pad8 : m.n_pad;
  v->forced_rows = i8 ? m.forced_rows8 : 0;
  v->extended_rows = i8 ? m.extended_rows8 : m.extended_rows;
  v->d_pad = i8 ? m.d_pad8 : m.d_pad;
  v->usable = i8 ? (m.i8_ok ? 1 : 0) : (m.fp16_range_ok ? 1 : 0);
  v->rot = i8 && m.rot8 ? 1 : 0;
  v->rot_w = i8 ? m.rot_w8 : 0;
  v->fold = i8 && m.fold8 ? 1 : 0;
  v->version = 0;
  v->step = i8 ? m.step8 : 0.f;
  v->slack = rerank_slack(ix.dim_);
  if (!v->usable) return EPS_OK;   // (8-bit: the table does not fit one grid, its row buffers were given back; fp16: values beyond its range - no search reads it)
  hipError_t er = hipSuccess;
  auto get = [&](void* dst, const void* src, size_t bytes) {
    if (dst && src && er == hipSuccess) er = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
  };
  const size_t rows = (size_t)v->n_pad, dp = (size_t)v->d_pad;
  if (i8) {
    get(v->x, m.x8.p, rows * dp);
    get(v->acc0, m.acc0.p, rows * 4);
    get(v->erow, m.erow.p, rows * 4);
    get(v->hrow, m.hrow.p, rows * 4);
    get(v->mu, m.mu8.p, dp * 4);
    if (m.rot8) get(v->sp, m.sp8.p, dp * 4);
    get(v->scal, m.scal8.p, 32);
    get(v->scalf, m.scal8f.p, 32);
  } else {
    get(v->x, m.xh.p, rows * dp * 2);
    get(v->xn, m.xn.p, rows * 4);
    get(v->start, ix.metric_ == 0 ? m.xn_s.p : m.zeros_s.p, rows * 4);   // (what filter_args hands the kernel as start values)
    get(v->scal, m.scal.p, 16);
  }
  if (er != hipSuccess) return ix.hip_fail(er, "mirror_view: copy");
  if (nq > 0) {
    ProbeGuard guard(ix);
    DevBuf dq;
    rc = upload_queries(ix, hq, nq, &dq);
    Chain c;
    if (rc == EPS_OK) rc = plan_chain(ix, m, dq.as<float>(), nq, 1, nullptr, false, 1, i8, ix.n_rows_, &c);
    if (rc == EPS_OK) rc = prepare_queries(ix, m, c);
    if (rc != EPS_OK) return rc;
    v->version = c.version;
    get(v->q, i8 ? m.q8.p : m.qh.p, (size_t)nq * dp * (i8 ? 1 : 2));
    get(v->qstat, m.qstat.p, (size_t)nq * 16);
    if (i8 && c.fold) {
      get(v->acc0b, m.acc0b.p, rows * 4);
      get(v->qmax, m.qmax.p, 8);
    }
    if (er == hipSuccess) er = hipStreamSynchronize(s);   // (before the queries' device copy goes)
    if (er != hipSuccess) return ix.hip_fail(er, "mirror_view: queries");
  }
  er = hipStreamSynchronize(s);
  return er == hipSuccess ? EPS_OK : ix.hip_fail(er, "mirror_view");
}

// ---- what a single pass with IMPOSED thresholds is made of (flat_filter_pass below, the radius search behind it)
// every query's threshold from a distance - keys[j] = make_key(distance, 0), k = 1 - by the chain's own kernels (which also zero the candidate
// counts and the group counters), or (pad_only) the padding entries alone
static void launch_pass_thresholds(const Index& ix, const HalfMirror& m, const Chain& c, const u64* keys, int pad_only) {
  hipStream_t s = ix.stream_;
  const dim3 tgrid((unsigned)((c.b_pad + 255) / 256));
  if (c.i8)
    hipLaunchKernelGGL(threshold8_kernel, tgrid, dim3(256), 0, s, keys, 1, c.nq, c.b_pad, m.qstat.as<float>(), c.maxima(m), ix.metric_, c.u8, m.T.as<int>(), c.c.cnt,
                       m.gsync.as<u32>(), c.slack, c.approx ? 1 : 0, pad_only);
  else
    hipLaunchKernelGGL(threshold_kernel, tgrid, dim3(256), 0, s, keys, 1, c.nq, c.b_pad, m.qstat.as<float>(), c.maxima(m), ix.metric_, m.T.as<float>(), c.c.cnt,
                       m.gsync.as<u32>(), c.slack, c.approx ? 1 : 0, pad_only);
}
// the group counters' start state and ONE filter launch over the row tiles of [lo, hi) against the thresholds in m.T
static hipError_t launch_pass(const Index& ix, const HalfMirror& m, const Chain& c, int64_t lo, int64_t hi, bool dense) {
  hipStream_t s = ix.stream_;
  const hipError_t er = hipMemsetAsync(m.gsync.p, 0, 1024, s);
  if (er != hipSuccess) return er;
  FilterArgs fa = filter_args(ix, m, c);
  fa.tile0 = lo / BM3;
  fa.ntiles = (hi + BM3 - 1) / BM3 - fa.tile0;
  fa.row_hi = hi;
  fa.dense = dense ? 1 : 0;
  launch_filter(m, c, fa, s);
  return hipSuccess;
}

int32_t flat_filter_pass(Index& ix, const float* hq, int64_t nq, int bits, int64_t lo, int64_t hi, int64_t cap, int mode, int thr_form, const void* thr,
                         void* T_out, u32* cnt_out, void* cand_out) {
  if (bits != 8 && bits != 16) return ix.fail(EPS_USER_ERROR, "filter_pass: bits must be 8 or 16");
  if (nq < 1 || nq > 2048 || !hq) return ix.fail(EPS_USER_ERROR, "filter_pass: 1 .. 2048 host queries");
  if (mode < EPS_PASS_IDS || mode > EPS_PASS_DENSE || thr_form < EPS_THR_RAW || thr_form > EPS_THR_DISTANCE) return ix.fail(EPS_USER_ERROR, "filter_pass: unknown mode");
  if (!cnt_out || !cand_out || (!thr && mode != EPS_PASS_DENSE)) return ix.fail(EPS_USER_ERROR, "filter_pass: null argument");
  const bool i8 = bits == 8;
  int32_t rc = ensure_probe_mirror(ix, i8);
  if (rc != EPS_OK) return rc;
  HalfMirror& m = *ix.mirror_;
  const int64_t n = ix.n_rows_;
  if (i8 ? !m.i8_ok : !m.fp16_range_ok) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, "filter_pass: the table has no usable mirror of this width");
  if (lo < 0 || lo >= hi || hi > n || lo % BM3 != 0) return ix.fail(EPS_USER_ERROR, "filter_pass: rows [lo, hi) must lie in the table, lo on a multiple of 256");
  if (cap < 1 || cap > ((int64_t)1 << 30) || (size_t)nq * (size_t)cap * 8 > ((size_t)8 << 30)) return ix.fail(EPS_USER_ERROR, "filter_pass: candidate cap out of range");
  if (mode == EPS_PASS_DENSE && cap < hi - lo) return ix.fail(EPS_USER_ERROR, "filter_pass: the dense form needs one slot per row of the range");
  hipStream_t s = ix.stream_;
  ProbeGuard guard(ix);
  const bool approx = mode != EPS_PASS_IDS;   // (the chain launches the key and the dense forms in its approx mode, on the unfolded start values)
  DevBuf dq, keys;
  rc = upload_queries(ix, hq, nq, &dq);
  Chain c;
  if (rc == EPS_OK) rc = plan_chain(ix, m, dq.as<float>(), nq, 1, nullptr, approx, 1, i8, n, &c);
  if (rc != EPS_OK) return rc;
  if (mode == EPS_PASS_DENSE && c.version < 7) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, "filter_pass: the dense form exists for the v7 kernel's shapes only");
  c.cap = (int)cap;
  if (!m.cand.reserve((size_t)nq * (size_t)cap * 8) || !keys.reserve((size_t)nq * 8)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "filter_pass: out of device memory");
  rc = prepare_queries(ix, m, c);
  if (rc != EPS_OK) return rc;
  ensure_filter_kernels(ix, m);
  // thresholds: the padding entries and - from distances - every query's T by the chain's own kernels; raw ones are used as they are
  hipError_t er = hipSuccess;
  const int pad_only = thr_form == EPS_THR_DISTANCE && mode != EPS_PASS_DENSE ? 0 : 1;
  if (!pad_only) {
    std::vector<u64> hk((size_t)nq);
    for (int64_t j = 0; j < nq; ++j) hk[(size_t)j] = host_key(static_cast<const float*>(thr)[j]);
    er = hipMemcpyAsync(keys.p, hk.data(), (size_t)nq * 8, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) return ix.hip_fail(er, "filter_pass: thresholds");
  }
  launch_pass_thresholds(ix, m, c, keys.as<u64>(), pad_only);
  if (pad_only) {
    if (mode != EPS_PASS_DENSE) er = hipMemcpyAsync(m.T.p, thr, (size_t)nq * 4, hipMemcpyHostToDevice, s);
    else er = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.T.p), 0x7F800000, (size_t)nq, s);   // (the seed pass's start state; the dense form reads no threshold)
    if (er == hipSuccess) er = hipMemsetAsync(c.c.cnt, 0, (size_t)nq * 4, s);
  }
  if (er == hipSuccess) er = launch_pass(ix, m, c, lo, hi, mode == EPS_PASS_DENSE);
  if (er != hipSuccess) return ix.hip_fail(er, "filter_pass: start state");
  er = hipGetLastError();
  if (er != hipSuccess) return ix.hip_fail(er, "filter_pass: launch");
  if (T_out) er = hipMemcpyAsync(T_out, m.T.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess && mode != EPS_PASS_DENSE) er = hipMemcpyAsync(cnt_out, c.c.cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(cand_out, m.cand.p, (size_t)nq * (size_t)cap * (approx ? 8 : 4), hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return ix.hip_fail(er, "filter_pass");
  if (mode == EPS_PASS_DENSE)
    for (int64_t j = 0; j < nq; ++j) cnt_out[j] = (u32)(hi - lo);
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ radius search, matrix form
// eps_index_search_range (Index::search_range): a radius query knows its threshold before the first row is read, so the chain's seed pass and
// stages collapse into ONE filter launch over all rows - thresholds from the radii in the exact-mode, distance form (as flat_filter_pass builds
// them: every row whose exact distance is <= r passes) - and the exact tail (range.hip) into the survivor lists L.  Slices as flat_mfma_search.
__global__ void range_keys_kernel(const float* radius, int64_t nq, u64* keys) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nq) keys[j] = make_key(radius[j], 0u);
}

// candidate slots per query of the filter launch: 4 x cap, and never fewer than fit the scratch the chain reserves anyway (plan_chain: 4096 slots
// of 8 bytes = 8192 row ids).  A performance knob: a query whose list overflows is answered by the stream form
static int range_cand_cap(int cap) { return std::max(8192, 4 * cap); }

static int32_t range_slice(Index& ix, HalfMirror& m, bool i8, const float* dq, int64_t nq, const RangeLists& L, unsigned long long* cand_total) {
  hipStream_t s = ix.stream_;
  const int64_t n = ix.n_rows_;
  Chain c;
  int32_t rc = plan_chain(ix, m, dq, nq, 1, nullptr, false, 1, i8, n, &c);
  if (rc != EPS_OK) return rc;
  c.cap = range_cand_cap(L.cap);
  if (!m.cand.reserve((size_t)nq * (size_t)c.cap * 4) || !m.seedc.reserve((size_t)nq * 8)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "search_range: out of device memory (candidates)");
  rc = prepare_queries(ix, m, c);
  if (rc != EPS_OK) return rc;
  ensure_filter_kernels(ix, m);
  m.s8_clean_cnt = nullptr;   // (the pass's counters live where the one-pass form keeps its own)
  u64* keys = m.seedc.as<u64>();   // (the seed stage's lists: no seeds here)
  hipLaunchKernelGGL(range_keys_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, L.radius, nq, keys);
  launch_pass_thresholds(ix, m, c, keys, 0);
  (void)hipEventRecord(ix.evk0_, s);
  const hipError_t er = launch_pass(ix, m, c, 0, n, false);
  if (er != hipSuccess) return ix.hip_fail(er, "search_range: start state");
  (void)hipEventRecord(ix.evk1_, s);
  ix.stats_.main_kernel_launches += 1;
  ix.stats_.main_kernel_rows = n;
  ix.stats_.main_kernel_queries = nq;
  ix.stats_.main_kernel_bits = i8 ? 8 : 16;
  ix.stats_.dist_evals += nq * n;
  RangeRerankArgs ra{ix.d_rows_, (int)ix.dim_, ix.metric_, dq, nq, c.fs, m.cand.as<u32>(), c.c.cnt, c.cap, L, cand_total};
  launch_range_rerank(ra, s);
  return EPS_OK;
}

int32_t flat_range_lists(Index& ix, const float* dq, int64_t nq, int bits, const RangeLists& L, unsigned long long* cand_total, bool* served) {
  *served = false;
  if (ix.n_rows_ <= 0) return EPS_OK;
  const bool auto_bits = bits != 8 && bits != 16;
  // the chain's own decisions: an 8-bit table that declines falls to fp16, fp16 out of range to the stream form
  bool i8 = bits != 16;
  int32_t rc = EPS_OK;
  if (i8) {
    rc = ensure_mirror8(ix);
    if (rc != EPS_OK) return rc;
    if (!ix.mirror_->i8_ok || (auto_bits && ix.mirror_->i8_overflows >= 3)) i8 = false;
  }
  if (!i8) {
    rc = ensure_mirror(ix);
    if (rc != EPS_OK) return rc;
    if (!ix.mirror_->fp16_range_ok) return EPS_OK;
  }
  HalfMirror& m = *ix.mirror_;
  const int64_t slice = std::max(256, tune_int("EPS_MFMA_MAX_BATCH", 2048));
  for (int64_t q0 = 0; q0 < nq; q0 += slice) {
    const RangeLists Ls{L.keys + q0 * L.cap, L.cnt + q0, L.radius + q0, L.cap};
    rc = range_slice(ix, m, i8, dq + q0 * ix.dim_, std::min(slice, nq - q0), Ls, cand_total);
    if (rc != EPS_OK) return rc;
  }
  const hipError_t er = hipGetLastError();
  if (er != hipSuccess) return ix.hip_fail(er, "search_range: matrix form");
  *served = true;
  return EPS_OK;
}

}  // namespace eps
