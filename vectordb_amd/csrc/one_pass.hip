// A handful of queries (<= 32, k <= 64) in ONE pass over the 8-bit mirror: the host side of stream8_kernel.hpp.  The rule that admits a call,
// the call's filter mask, the pass and its re-rank, and what the form learns from its overflows.  Results are bit-identical to the staged
// chain's (mfma_filter.hip): both end in the same exact re-rank.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mirror.hpp"
#include "stream8_kernel.hpp"

namespace eps {

// The static part of the rule for the one-pass search (stream8_kernel.hpp): the cost model below prices a call as that form exactly when
// the engine (flat_stream8_slice) would take it up, before the state it learns at run time (declined forms, filters).  m8 = the 8-bit mirror
// of these rows, or null while none is built; n = the rows the call scans.
bool one_pass_fits(const Index& ix, const HalfMirror* m8, int64_t nq, int k, int64_t n) {
  if (tune_int("EPS_FLAT_ONE_PASS", 1) == 0) return false;
  const int max_k = std::min(S8_MAX_K, std::max(1, tune_int("EPS_S8_MAX_K", S8_MAX_K)));   // (A/B switch: 16 = the r4 range, larger k on the staged chain)
  // (rows of d_pad8 = 512..1024 bytes: 2..4 pieces of 256 columns)
  if (nq < 1 || nq > S8_MAX_Q || k < 1 || k > max_k || n < 65536 || ix.dim_ > 1024 || (m8 && n > m8->n8)) return false;
  // r6: tables whose margins are folded per batch (fold8: rows with a clamped value) take the form too - behind the prep launch and the fold
  // launch (the margins depend on the call's queries), with margin-free thresholds and offers of `accumulator - 2 x the row's margin` (stream8_offer_value)
  const bool fold8 = m8 && m8->fold8;
  // (17..32 queries, r6: the two-column-block pass beats the staged chain where a query leaves a few hundred candidates - 1M x 768 U[0,1): 17 / 24 / 32
  // queries 0.235 / 0.254 / 0.281 ms against 0.38 - and loses where it leaves several times that: the same table of embedding-like rows 0.433 /
  // 0.465 / 0.505 against 0.432 / 0.443 / 0.443 (profiles/r6_one_pass_17_to_32_queries.txt).  Tables with folded margins are the looser ones.)
  if (nq > 16 && fold8) return false;
  // (... and on LARGE tables: with two column blocks the pass is no longer purely HBM-bound - 24 MFMAs and 12 LDS operand reads per 16-row block - and its
  // time grows with the queries, while the chain's 128-query tiles stream the mirror at the HBM rate whatever nq: 10M x 768, 17 / 24 / 32 queries: 1.46 /
  // 1.54 / 1.73 ms against the chain's 1.53; 4M: 0.66 / 0.70 / 0.79 against 0.78; 2M: 0.38 / 0.40 / 0.45 against 0.51)
  if (nq > 16 && (double)(nq - 16) * (double)n > 64e6) return false;
  return true;
}

// One-pass calls under a compiled filter PROGRAM (r5): the pass itself cannot call the evaluator (a function call = scratch memory for every
// wavefront of an HBM-bound stream), and it does not have to - whether a row is visible does not depend on the query, so the whole predicate
// (deleted bitset, int-column test, program; @distance = 0 as PreFilterBruteForceSearch evaluates it, vec_search_executor.cpp:795) is
// evaluated ONCE per row into a bitset in the deleted bitset's layout (bit i of byte i >> 3 set = row i is NOT visible) by this launch,
// and pass + re-rank read that.  One thread per ROW, the wavefront's 64 verdicts gathered by a ballot, 8 lanes write the 8 bytes (a thread per
// byte evaluated its 8 rows one after the other - 8 dependent attribute loads - and the launch took 21 us at 1M rows under rocprofv3).
__global__ __launch_bounds__(256) void filter_mask_kernel(FilterSpec f, int64_t n, uint8_t* mask) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool visible = r < n && row_visible(f, (u32)r, 0.f);
  const unsigned long long hidden = ~__ballot(visible);   // bit l: row (first row of the wavefront + l) is NOT visible (rows >= n: hidden)
  const int lane = lane_id();
  const int64_t wbase = r - lane;                          // (a multiple of 64)
  if (lane < 8 && wbase + lane * 8 < n) mask[(wbase >> 3) + lane] = (uint8_t)(hidden >> (lane * 8));
}

constexpr int S8_WG_PER_CU = 2;   // workgroups of the one-pass kernel per CU

// the pass for rows of P pieces of 256 columns, in the form the call's shape selects
template <int P>
static void launch_pass(const Stream8Args& a, dim3 grid, hipStream_t s, bool wide, bool mfma_form, bool clean) {
  const dim3 block(256);
  if (wide) {   // k = 17..64, 1-2 queries: the v_dot4 pass with two slots per lane
    if (a.nq == 1) hipLaunchKernelGGL((stream8_kernel<P, 1, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((stream8_kernel<P, 2, false, true>), grid, block, 0, s, a);
  } else if (mfma_form) {   // 5..16 queries (and 3-4 with k > 16): the same pass on the matrix cores; r6, 17..32: two 16-query column blocks per row block
    if (a.nq > 16) hipLaunchKernelGGL((stream8m_kernel<P, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((stream8m_kernel<P, 1>), grid, block, 0, s, a);
  } else if (a.nq > 2) {
    hipLaunchKernelGGL((stream8_kernel<P, 4, false>), grid, block, 0, s, a);
  } else if (clean) {   // (the pass quantises its queries itself)
    if (a.nq == 1) hipLaunchKernelGGL((stream8_kernel<P, 1, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((stream8_kernel<P, 2, true>), grid, block, 0, s, a);
  } else {
    if (a.nq == 1) hipLaunchKernelGGL((stream8_kernel<P, 1, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((stream8_kernel<P, 2, false>), grid, block, 0, s, a);
  }
}

static Stream8Args pass_args(const Index& ix, const HalfMirror& m, const float* dq, int64_t nq, int k, int64_t n, const FilterSpec& fs, int slots) {
  const bool fold = m.fold8;
  Stream8Args a;
  a.x8 = m.x8.as<signed char>();
  a.acc0 = fold ? m.acc0b.as<int>() : m.acc0.as<int>();
  a.acc0_raw = fold ? m.acc0.as<int>() : nullptr;
  a.n = n;
  a.d_pad8 = m.d_pad8;
  a.q8 = m.q8.as<signed char>();
  a.qstat = m.qstat.as<float>();
  a.scal = fold ? m.scal8f.as<float>() : m.scal8.as<float>();   // (folded: the margin entries are zero - the margins are in the start values)
  a.nq = (int)nq;
  a.k = k;
  a.metric = ix.metric_;
  a.u = key_unit8(ix.metric_, m.step8);
  a.slack = rerank_slack(ix.dim_);
  a.G = m.s8g.as<int>();
  a.slots = slots;
  a.raw_cnt = m.s8g.as<u32>() + S8_TABLE_WORDS;
  a.raw = m.s8raw.as<u64>();
  a.f = fs;
  a.qf32 = dq;
  a.mu = m.mu8.as<float>();
  a.qstat_out = m.qstat.as<float>();
  a.dim = (int)ix.dim_;
  a.step = m.step8;
  a.inv_step = 1.f / m.step8;
  return a;
}

// EPS_DEBUG / EPS_DEBUG_ONE_PASS_OVERFLOW: what every query left in the table and the lists
static void dump_one_pass(const HalfMirror& m, const Stream8Args& a, const CountersRead& h) {
  std::vector<u32> hc((size_t)S8_TABLE_WORDS + (size_t)S8_MAX_Q * S8_MAX_WAVES);
  (void)hipMemcpy(hc.data(), m.s8g.p, hc.size() * 4, hipMemcpyDeviceToHost);
  for (int64_t q = 0; q < a.nq; ++q) {
    unsigned long long raw = 0;
    u32 most = 0;
    int filled = 0;
    for (int w = 0; w < a.waves; ++w) {
      raw += hc[S8_TABLE_WORDS + q * a.waves + w];
      most = std::max(most, hc[S8_TABLE_WORDS + q * a.waves + w]);
    }
    for (int i = 0; i < a.slots; ++i) filled += (int)hc[(q * a.slots + i) * S8_SLOT_STRIDE] != S8_EMPTY;
    fprintf(stderr, "[eps one pass] query %lld: %llu raw candidates (at most %u in one wavefront's list of %d), %d of the slots filled, re-ranked (all queries) %llu, overflow %u\n",
            (long long)q, raw, most, S8_WAVE_CAP, filled, h.total, h.overflow);
  }
}

// the call's two counters after its last launch: from the host-mapped words behind a stream sync, or in ONE small copy (every copy is a trip
// through the DMA queue at the end of a 0.2 ms call)
static hipError_t read_counters(const HalfMirror& m, const CallCounters& c, bool host_words, hipStream_t s, CountersRead* h) {
  if (host_words) {
    const hipError_t er = hipStreamSynchronize(s);
    if (er != hipSuccess) return er;
    const volatile u32* hp = m.s8_pub.p;
    h->overflow = hp[0];
    h->total = (unsigned long long)hp[2] | ((unsigned long long)hp[3] << 32);
    return hipSuccess;
  }
  u32 hraw[6] = {0, 0, 0, 0, 0, 0};
  const size_t span = (size_t)(reinterpret_cast<const char*>(c.total) + 8 - reinterpret_cast<const char*>(c.overflow));
  hipError_t er = hipMemcpyAsync(hraw, c.overflow, span, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  if (er != hipSuccess) return er;
  h->overflow = hraw[0];
  memcpy(&h->total, reinterpret_cast<const char*>(hraw) + (span - 8), 8);
  return hipSuccess;
}

// What the form remembers of a call, per kernel form (kclass).  A form that overflowed twice in a row on these rows stays on the chain;
// under a deleted bitset / an int-column filter / a program an overflow usually means "fewer than k rows visible", which the rows' version
// says nothing about: two such overflows in a row send the next 32 filtered calls straight to the staged chain
static void note_outcome(HalfMirror& m, int kclass, bool filtered, bool overflowed, int64_t rows_version) {
  if (!overflowed) {
    if (filtered) m.s8_filt_overflows[kclass] = 0; else m.s8_overflows[kclass] = 0;
  } else if (filtered) {
    if (++m.s8_filt_overflows[kclass] >= 2) {
      m.s8_filt_overflows[kclass] = 0;
      m.s8_filt_skip[kclass] = 32;
    }
  } else if (++m.s8_overflows[kclass] >= 2) {
    m.s8_declined_version[kclass] = rows_version;
  }
}

// What a call of the one-pass form is made of up to and including its pass: what the pass was launched with and what the re-rank launch behind it
// (flat_stream8_slice) or a probe of its leavings (one_pass_probe) needs to know of it
struct OnePass {
  Stream8Args a;
  FilterSpec fs;        // what the pass and the re-rank test rows with (a filter program: its mask, as a deleted bitset)
  CallCounters c;
  int64_t n = 0;        // rows scanned
  int kclass = 0, slots = 0, cap = 0, pieces = 0;
  bool filtered = false, masked = false, mfma_form = false, wide = false, clean = false, host_words = false, two_launches = false, timed = false;
};

// From the entry rule to the pass: the rule (one_pass_fits, declined forms, programs that read @distance, filtered calls sent to the chain), the
// scratch, the mask launch under a filter program, the prep launch - or none where the last one-pass call left the state clean -, the fold launch
// behind it on a folding table, and the pass itself.  *taken = false: the call does not take the form, nothing was launched.  probe: a look at
// what the next search would do - what that search would consume (the count of filtered calls still to skip) stays as it is
static int32_t one_pass_to_the_pass(Index& ix, const float* dq, int64_t nq, int k, bool probe, OnePass* p, bool* taken) {
  *taken = false;
  HalfMirror& m = *ix.mirror_;
  const int64_t n = ix.scan_limit_ >= 0 ? std::min(ix.scan_limit_, ix.n_rows_) : ix.n_rows_;
  if (!one_pass_fits(ix, &m, nq, k, n)) return EPS_OK;
  const bool fold = m.fold8;
  // (a form that overflowed twice in a row on these rows stays on the chain - per kernel form, r6: five or more queries share one list budget per
  // query and overflow on tables where one query does not: an 8-query batch must not talk the table out of the form for single-query traffic)
  const int kclass = (k <= 16 ? 0 : 1) + (nq <= 4 ? 0 : (nq <= 16 ? 2 : 4));   // (r6: 17..32 queries - two column blocks - are a form of their own)
  if (m.s8_declined_version[kclass] == ix.rows_version_) return EPS_OK;
  FilterSpec fs = ix.filter_spec();
  // a compiled filter program: evaluated once per row into a bitset (filter_mask_kernel) that pass and re-rank read as a deleted bitset.  Only
  // where the predicate does not depend on the candidate's distance (Index::search sends programs that read @distance outside a pre-filter
  // call to the stream engine before they get here; checked again, the staged chain evaluates per candidate)
  const bool masked = fs.prog != nullptr;
  if (masked && ix.prog_uses_dist_ && !ix.prefilter_call_) return EPS_OK;
  if (masked && tune_int("EPS_S8_FILTER_PROGRAMS", 1) == 0) return EPS_OK;   // (A/B switch: programs on the staged chain, as until r4)
  const bool filtered = fs.deleted || fs.column || masked;
  if (filtered && m.s8_filt_skip[kclass] > 0) {   // (a mask that starves the pass used to cost a wasted pass on EVERY call)
    if (!probe) --m.s8_filt_skip[kclass];
    return EPS_OK;
  }
  hipStream_t s = ix.stream_;
  const int cap = std::max(4096, 64 * k);
  if (!m.qstat.reserve((size_t)S8_MAX_Q * 16) || !m.q8.reserve((size_t)S8_MAX_Q * m.d_pad8) || !m.cand.reserve((size_t)nq * cap * 8) || !m.cnt.reserve((size_t)(S8_MAX_Q + 16) * 4) ||
      !m.s8g.reserve((size_t)S8_TABLE_WORDS * 4 + (size_t)S8_MAX_Q * S8_MAX_WAVES * 4) || !m.s8raw.reserve((size_t)nq * S8_MAX_WAVES * S8_WAVE_CAP * 8) ||
      (masked && !m.s8mask.reserve((size_t)(n + 7) / 8 + 16)))
    return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "MFMA engine: out of device memory (scratch)");
  if (masked) {   // (every call: the caller's bitset and attribute rows are used in place and may have changed since the last one)
    fs.prog_use_dist = 0;
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fs, n, m.s8mask.as<uint8_t>());
    fs = no_filter();
    fs.deleted = m.s8mask.as<uint8_t>();
  }
  // (cnt: nq + 8 <= 12 words in use here; DevBuf::reserve never hands out less than 256 bytes)
  const CallCounters c = call_counters(m.cnt.as<u32>(), nq);
  const bool host_words = !(tune_int("EPS_S8_HOST_WORDS", 1) == 0) && m.s8_pub.get();   // (A/B switch)
  const bool two_launches = host_words && !(tune_int("EPS_S8_TWO_LAUNCHES", 1) == 0) && !tune_env("EPS_DEBUG");  // (A/B switch; the debug log reads the table after the call)
  // (3-4 queries keep the prep launch: next to four queries' slices and two chunks in flight the in-kernel form does not fit 256 registers)
  // (k = 17..64: 128 slots per query in the same table - a layout of its own, so such a call always starts with the prep launch, which empties
  // the slots it uses, and never leaves the "clean" state behind)
  const int slots = k <= 16 ? S8_SLOTS : S8_SLOTS_WIDE;
  const bool mfma_form = nq > 4 || (slots != S8_SLOTS && nq > 2);   // stream8m_kernel (16 query columns: the prep launch lays down 16 rows, zeros beyond nq)
  // (a table in the rotated frame keeps the prep launch: the transform is its work, not the pass's)
  const bool clean = two_launches && nq <= 2 && slots == S8_SLOTS && m.s8_clean_cnt == m.cnt.p && m.s8_clean_g == m.s8g.p && !m.rot8 && !fold;
  m.s8_clean_cnt = m.s8_clean_g = nullptr;   // (set again when this call has come back)
  if (!clean) {
    Prep8Extra px;
    px.cnt = c.cnt;     // candidate counts, overflow and total counters = 0
    px.cntv = 0;
    px.s8g = m.s8g.as<int>();
    px.s8_slots = slots;
    const int prep_rows = mfma_form ? (nq > 16 ? 32 : 16) : 4;   // (the matrix form reads 16 / 32 query rows: zeros beyond nq)
    const hipError_t er = prep8_queries(m, fold, (int)ix.dim_, ix.metric_, dq, nq, prep_rows, m.q8.as<signed char>(), m.qstat.as<float>(), px, s);
    if (er != hipSuccess) return ix.hip_fail(er, "memset");
  }
  ix.stats_.i8_folded = fold ? 1 : 0;
  Stream8Args a = pass_args(ix, m, dq, nq, k, n, fs, slots);
  if (!m.s8_cus) {   // (once per mirror: the query costs more than the search)
    hipDeviceProp_t prop;
    m.s8_cus = hipGetDeviceProperties(&prop, ix.device_) == hipSuccess ? std::max(8, prop.multiProcessorCount) : 256;
  }
  const dim3 grid((unsigned)std::min<int64_t>(std::min<int64_t>((int64_t)m.s8_cus * S8_WG_PER_CU, S8_MAX_WAVES / 4), (n + 63) / 64));
  a.waves = (int)grid.x * 4;
  // (no event pair around the pass by default: a record between two dependent launches costs this chain 5-10 us each; kernel_ms covers
  // the call.  EPS_ONE_PASS_TIMED=1 - bench.py's roofline leg - records the pair: main_kernel_ms = the pass)
  const bool timed = !probe && tune_int("EPS_ONE_PASS_TIMED", 0) != 0;
  if (timed) (void)hipEventRecord(ix.evk0_, s);
  const bool wide = slots != S8_SLOTS && nq <= 2;
  const int pieces = m.d_pad8 / 256;   // (rows of 512..1024 bytes)
  if (pieces == 2) launch_pass<2>(a, grid, s, wide, mfma_form, clean);
  else if (pieces == 3) launch_pass<3>(a, grid, s, wide, mfma_form, clean);
  else launch_pass<4>(a, grid, s, wide, mfma_form, clean);
  if (timed) (void)hipEventRecord(ix.evk1_, s);
  p->a = a;
  p->fs = fs;
  p->c = c;
  p->n = n;
  p->kclass = kclass;
  p->slots = slots;
  p->cap = cap;
  p->pieces = pieces;
  p->filtered = filtered;
  p->masked = masked;
  p->mfma_form = mfma_form;
  p->wide = wide;
  p->clean = clean;
  p->host_words = host_words;
  p->two_launches = two_launches;
  p->timed = timed;
  *taken = true;
  return EPS_OK;
}

// *done = false: not applicable to this call, or a list overflowed - the staged chain answers it
int32_t flat_stream8_slice(Index& ix, const float* dq, int64_t nq, int k, u64* run_keys, bool* done) {
  *done = false;
  HalfMirror& m = *ix.mirror_;
  OnePass p;
  bool taken = false;
  const int32_t rc = one_pass_to_the_pass(ix, dq, nq, k, false, &p, &taken);
  if (rc != EPS_OK || !taken) return rc;
  const Stream8Args& a = p.a;
  const CallCounters& c = p.c;
  const int64_t n = p.n;
  const int slots = p.slots;
  const bool host_words = p.host_words, two_launches = p.two_launches;
  hipStream_t s = ix.stream_;
  RerankArgs ra = rerank_args(ix, m, dq, nq, k, p.fs, p.cap, run_keys, c, a.scal, 8);   // (fuse = 1: counts only - overflow / total)
  ra.s8_G = a.G;                 // (the launch selects its candidates from the pass's lists first)
  ra.s8_slots = slots;
  ra.s8_fast = !(tune_int("EPS_S8_RERANK", 1) == 0);   // (A/B switch: 0 = rerank_kernel with the selection prologue, as until r5)
  ra.s8_counts = a.raw_cnt;
  ra.s8_lists = a.raw;
  ra.s8_waves = a.waves;
  ra.s8_cand = m.cand.as<u32>();
  if (host_words) {
    ra.pub = m.s8_pub.p;
    ra.pub_ticket = c.cnt + nq + 6;   // (zeroed by the prep launch with the other counters: cnt[nq .. nq + 8))
    ra.s8_reset = two_launches && slots == S8_SLOTS ? 1 : 0;
  }
  const bool fin_here = finalize_in_rerank(ix, nq, &ra);
  launch_rerank(ra, s);
  if (fin_here) (void)hipEventRecord(ix.ev1_, s);
  hipError_t er = hipGetLastError();
  if (er != hipSuccess) return ix.hip_fail(er, "one-pass flat search launch");
  if (!fin_here && ix.call_.pre_sync && nq == ix.call_.nq) ix.call_.pre_sync();
  CountersRead h;
  er = read_counters(m, c, host_words, s, &h);
  if (er != hipSuccess) return ix.hip_fail(er, "one-pass flat search");
  if (host_words && two_launches && slots == S8_SLOTS) {   // (the launch left slots and counters as the next call needs them)
    m.s8_clean_cnt = m.cnt.p;
    m.s8_clean_g = m.s8g.p;
  }
  if (tune_env("EPS_DEBUG") || (h.overflow && tune_env("EPS_DEBUG_ONE_PASS_OVERFLOW"))) dump_one_pass(m, a, h);
  note_outcome(m, p.kclass, p.filtered, h.overflow != 0, ix.rows_version_);
  if (h.overflow) {   // (too loose a bound for this table, or a filter that leaves fewer than k rows visible: the staged chain answers)
    ix.result_finalized_ = false;
    return EPS_OK;
  }
  if (fin_here) ix.result_finalized_ = true;
  ix.stats_.rerank_rows += (int64_t)h.total;
  ix.stats_.dist_evals += nq * n;
  ix.stats_.main_kernel_launches = p.timed ? 1 : 0;   // (0: not timed on its own)
  ix.stats_.main_kernel_rows = n;
  ix.stats_.main_kernel_queries = nq;
  ix.stats_.main_kernel_bits = 8;
  ix.stats_.one_pass = 1;
  ix.stats_.i8_rotated = m.rot8 ? 1 : 0;
  *done = true;
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ the pass on its own (tests)
// eps_index_one_pass_probe (include/epsilla_gfx950.h; tests/one_pass_ref.py, tests/test_gpu_one_pass_pin.py): what ONE pass leaves behind -
// every wavefront's list, the table, the threshold the re-rank's selection would read from it - before any re-rank has looked at it.

// kth and T of every query's FINAL table, by the function the re-rank's selection prologue calls (flat_kernels.hip), with its arguments
__global__ __launch_bounds__(64) void one_pass_threshold_kernel(const int* G, int slots, int nq, int k, const float* qstat, const float* scal, int metric, float u, float slack,
                                                                int* kth, int* T) {
  const int lane = lane_id();
  for (int q = 0; q < nq; ++q) {
    int gk;
    const int Tq = stream8_threshold_of(G + q * (slots * S8_SLOT_STRIDE), k, qstat + q * 4, scal, metric, u, slack, lane, gk, slots);
    if (lane == 0) {
      kth[q] = gk;
      T[q] = Tq;
    }
  }
}

int32_t one_pass_probe(Index& ix, const float* hq, int64_t nq, int k, eps_one_pass_form* form, u32* raw_cnt, u64* raw, int32_t* table, float* qstat, int32_t* kth,
                       int32_t* T_final) {
  if (!hq || !form || !raw_cnt || !raw || !table || !qstat || !kth || !T_final) return ix.fail(EPS_USER_ERROR, "one_pass_probe: null argument");
  if (nq < 1 || k < 1) return ix.fail(EPS_USER_ERROR, "one_pass_probe: nq and k must be positive");
  if (ix.n_rows_ <= 0) return ix.fail(EPS_USER_ERROR, "no rows attached");
  const char* not_this_form = "one_pass_probe: a search with these arguments would not take the one-pass form";
  if (nq > S8_MAX_Q || k > S8_MAX_K) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, not_this_form);   // (before any mirror is built for it)
  int32_t rc = ix.check_filters_cover_table("one_pass_probe");
  if (rc != EPS_OK) return rc;
  // the state a probe must hand back as it found it: the last search's statistics, and whether that search was a pre-filter call (this one is
  // what a search with default parameters would be: it is not)
  struct Guard {
    Index& ix;
    eps_search_stats stats;
    bool prefilter;
    ~Guard() {
      ix.stats_ = stats;
      ix.prefilter_call_ = prefilter;
      if (ix.mirror_) ix.mirror_->s8_clean_cnt = ix.mirror_->s8_clean_g = nullptr;   // (the table is full and the lists are written: the next search starts with its prep launch)
    }
  } guard{ix, ix.stats_, ix.prefilter_call_};
  ix.prefilter_call_ = false;
  if (ix.prog_len_ > 0 && ix.prog_uses_dist_) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, not_this_form);   // (Index::search: the exact stream engine)
  rc = ensure_mirror8(ix);
  if (rc != EPS_OK) return rc;
  HalfMirror& m = *ix.mirror_;
  if (!m.i8_ok) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, not_this_form);
  hipStream_t s = ix.stream_;
  DevBuf dq, out;
  if (!dq.reserve((size_t)nq * ix.dim_ * 4) || !out.reserve((size_t)nq * 8)) return ix.fail(EPS_INFRA_UNEXPECTED_ERROR, "one_pass_probe: out of device memory");
  hipError_t er = hipMemcpyAsync(dq.p, hq, (size_t)nq * ix.dim_ * 4, hipMemcpyHostToDevice, s);
  if (er != hipSuccess) return ix.hip_fail(er, "one_pass_probe: queries");
  OnePass p;
  bool taken = false;
  rc = one_pass_to_the_pass(ix, dq.as<float>(), nq, k, true, &p, &taken);
  if (rc != EPS_OK) return rc;
  if (!taken) return ix.fail(EPS_DB_UNSUPPORTED_ERROR, not_this_form);
  const Stream8Args& a = p.a;
  int* d_kth = out.as<int>();
  int* d_T = d_kth + nq;
  hipLaunchKernelGGL(one_pass_threshold_kernel, dim3(1), dim3(64), 0, s, a.G, a.slots, a.nq, a.k, a.qstat, a.scal, a.metric, a.u, a.slack, d_kth, d_T);
  er = hipGetLastError();
  if (er != hipSuccess) return ix.hip_fail(er, "one_pass_probe: launch");
  form->pieces = p.pieces;
  form->matrix = p.mfma_form ? 1 : 0;
  form->width = p.mfma_form ? (nq > 16 ? 2 : 1) : (nq > 2 ? 4 : (int32_t)nq);
  form->wide = p.wide ? 1 : 0;
  form->prep_in_kernel = p.clean ? 1 : 0;
  form->slots = a.slots;
  form->waves = a.waves;
  form->fold = a.acc0_raw ? 1 : 0;
  form->rot = m.rot8 ? 1 : 0;
  form->masked = p.masked ? 1 : 0;
  form->wave_cap = S8_WAVE_CAP;
  form->chunk = p.mfma_form ? 16 : (p.pieces <= 3 ? 16 : 8);   // (stream8m_kernel: CH = 16; stream8_kernel: CH = 4 U, U = 4 | 2 at 4 pieces)
  std::vector<int> g((size_t)nq * a.slots * S8_SLOT_STRIDE);
  er = hipMemcpyAsync(g.data(), a.G, g.size() * 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(raw_cnt, a.raw_cnt, (size_t)nq * a.waves * 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(raw, a.raw, (size_t)nq * a.waves * S8_WAVE_CAP * 8, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(qstat, a.qstat, (size_t)nq * 16, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(kth, d_kth, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipMemcpyAsync(T_final, d_T, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  if (er == hipSuccess) er = hipStreamSynchronize(s);   // (before the queries' device copy goes)
  if (er != hipSuccess) return ix.hip_fail(er, "one_pass_probe");
  for (size_t i = 0; i < (size_t)nq * a.slots; ++i) table[i] = g[i * S8_SLOT_STRIDE];
  return EPS_OK;
}

}  // namespace eps
