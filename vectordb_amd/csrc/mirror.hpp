// The mirrors of the row store (fp16, 8-bit) that the staged chain (mfma_filter.hip) and the one-pass search (one_pass.hip) read, and what
// those two need from the unit that builds them (mirror_build.hip) and from each other.  Private to csrc/.
#pragma once
#include <algorithm>

#include "index.hpp"

namespace eps {

struct HalfMirror {
  DevBuf xh;       // _Float16 [n_pad][d_pad]
  DevBuf xn;       // float [n_pad]  |x|^2 (+inf on padding rows)
  DevBuf zeros;    // float [n_pad]  base for IP / COSINE (+inf on padding rows)
  DevBuf xn_s;     // float [n_pad]  -|x|^2/2 (= xn / s for L2; -inf on padding rows): the accumulators' start values
  DevBuf zeros_s;  // float [n_pad]  0 (-inf on padding rows)
  DevBuf qf;       // _Float16 fragment-major copy of qh (what the v7 kernel reads)
  DevBuf qf16;     // 8-bit queries, fragment-major in 16x16x64 order (what v7's 256-query row-id tile reads)
  DevBuf gsync;    // u32 [64]: v7 group arrival counters
  DevBuf sxh, sbase, sbase_u;   // seed sample: S0 rows spread evenly over [0, n) (fp16 rows, their base / s, their base)
  int64_t sample_version = -1, sample_n = 0, sample_rows = 0;
  DevBuf scal;     // float [4]: E1max, nxh_max, xn_max, overflow flag (as float bits)
  DevBuf qh;       // _Float16 [b_pad][d_pad]
  DevBuf qstat;    // float [b_pad][4]: |q|^2, |q|, |q-qh|, unused
  DevBuf T;        // float [b_pad]
  DevBuf cand;     // u32 [b][cap]
  DevBuf cnt;      // u32 [b] candidate counts + the call's counters behind them (call_counters)
  DevBuf seedc;    // u32 [b][k]: rows of the k best seeds of every query (the seed stage's candidate lists)
  // 8-bit mirror (first-pass operand of the filter, see above)
  DevBuf x8;       // int8 [n_pad8][d_pad8]
  DevBuf acc0;     // int32 [n_pad8]: accumulator start of every row = ceil(-R/u) + 1 (-2^30 on padding rows)
  DevBuf sx8, sacc0;            // seed sample of the 8-bit mirror
  int64_t sample8_version = -1, sample8_n = 0, sample8_rows = 0;
  DevBuf scal8;    // float [8]: max |x' - xh'|, max |xh'|, max |x|^2, bad flag, max |R|, |mu|, max |x'| (during the build: min / max of x - mean as ordered u32 in [6], [7])
  // r4, per-row margins: the two norms of every row the Cauchy-Schwarz margin multiplies the query's with (erow = +inf: a row whose
  // constant leaves the accumulator's range - it is not tested, it always passes), the batch's folded start values, the maxima with
  // the two margin entries zeroed (what thresholds of folded launches read), the batch's largest query norms, the range histogram
  DevBuf erow, hrow;   // float [n_pad8]
  DevBuf acc0b;        // int32 [n_pad8]: acc0 + the row's margin for the CURRENT batch (fold8_kernel)
  DevBuf scal8f;       // float [8]
  DevBuf qmax;         // u32 [2]: float bits of the batch's max |q'| and max |q' - qh'| (query_prep8_kernel, atomicMax)
  DevBuf hist;         // u32 [4096 + 8]: histogram of x - mean over the sample; [4096]: forced rows
  DevBuf q8;       // int8 [b_pad][d_pad8]
  float h_scal8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  DevBuf mu8;      // float [d_pad8]: the grid's centre, one value per column (zeros beyond dim)
  float step8 = 0.f;            // the grid: xh' = step8 * xi around mu8
  // r6: the grid's frame (device_common.hpp, rot256_load): rot8 = rows and queries are quantised as R x; sp8 = int32 [d_pad8], R's
  // permutation and signs.  Chosen on the first build from the steps the two frames need on the same sample; kept when rows are appended.
  bool rot8 = false;
  int rot_w8 = 0;               // columns the rotation covers: dim rounded up to 256 (<= d_pad8; the columns beyond stay zero)
  DevBuf sp8;
  float step8_identity = 0.f, step8_rotated = 0.f;   // what the choice saw (stats; 0 = that frame was not measured)
  bool i8_trusted = false;      // the library's own choice has seen a batch through the 8-bit pass on this mirror (no probe needed)
  int64_t version8 = -1, n8 = 0, n_pad8 = 0, forced_rows8 = 0;
  int64_t epoch8 = 0;           // full (re)builds of the 8-bit mirror (an extension keeps the grid and every existing row's constant)
  bool fold8 = false;           // exact-mode users fold per-row margins per batch (rows differ); else table-wide margin in the thresholds
  int d_pad8 = 0;
  bool i8_ok = false;
  int i8_overflows = 0;         // consecutive batches whose 8-bit pass overflowed its candidate lists (the fp16 pass then answered)
  // r4, a handful of queries in one pass (stream8_kernel.hpp): the shared best-accumulator tables + raw candidate counters, the raw lists
  DevBuf s8g, s8raw;            // table slots (S8_TABLE_WORDS) + per-wavefront candidate counts;  u64 [nq][waves][S8_WAVE_CAP]
  DevBuf s8mask;                // r5: u8 [(n + 7) / 8] - a call's compiled filter PROGRAM (and bitset, and column test) evaluated once per row into
                                // one bitset (bit set = row invisible), which the pass and its re-rank then read as a deleted bitset
  // rows version on which the one-pass form overflowed twice in a row (the staged chain serves it); [0]: k <= 16, [1]: k = 17..64 - a larger k
  // passes more rows against the same lists, and must not talk the table out of the form for the small-k traffic
  int64_t s8_declined_version[6] = {-1, -1, -1, -1, -1, -1};
  int s8_overflows[6] = {0, 0, 0, 0, 0, 0};
  // under a deleted bitset / an int-column filter an overflow usually means "fewer than k rows visible": the rows' version says nothing
  // about it, so two such overflows in a row make the next 32 filtered calls go straight to the staged chain, then the one-pass form is tried again
  int s8_filt_overflows[6] = {0, 0, 0, 0, 0, 0}, s8_filt_skip[6] = {0, 0, 0, 0, 0, 0};   // (per class, as above)
  int s8_cus = 0;               // CUs of the device (grid of the one-pass kernel)
  // r5: the call's two result counters land in host-mapped memory (written by the last block of the re-rank launch), read after the stream
  // sync: no device-to-host copy at the end of a 0.2 ms call
  struct HostWords {
    u32* p = nullptr;
    ~HostWords() { if (p) (void)hipHostFree(p); }
    bool get() {
      if (!p && hipHostMalloc(reinterpret_cast<void**>(&p), 64, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
      return p != nullptr;
    }
  } s8_pub;
  // r5: the re-rank launch of a one-pass call leaves the table slots empty and the counters zero (RerankArgs::s8_reset), and the pass quantises its
  // queries itself - the next call is TWO launches, no prep launch.  s8_clean_* = the buffers that state lives in; anything else that writes
  // them (the staged chain's counters, a reallocation, a failed call) clears it and the next call starts with the prep launch again
  const void* s8_clean_cnt = nullptr;
  const void* s8_clean_g = nullptr;
  int64_t extended_rows8 = 0;
  int64_t version = -1;
  int64_t n = 0, n_pad = 0;
  int d_pad = 0;
  bool fp16_range_ok = true;
  int num_cus = 0;             // CUs of this index's device (persistent grid size)
  int64_t extended_rows = 0;   // rows converted by incremental extensions (test hook)
  float h_scal[4] = {0, 0, 0, 0};
};

// queries on the table's grid.  qstat[r] = |q|^2, |q'|, |q' - qh'|, C[q] (the constant that turns u-scaled accumulators into
// approximate distances: dist ~ a.s * acc + qstat[3]);  q' = q - mu;  C = |q'|^2 (L2), 1 - q.mu (COSINE), -q.mu (DOT)
// (r4) what the flat engine used to do in two more launches of its own, for calls that are a chain of short dependent launches (one
// query: every launch is ~5 us of latency): the fragment-major copy of the query operand the v7 kernel reads (pack_qf_kernel) and the
// start state of a seeded call (seed_prologue_kernel).  All-null: plain query_prep8 (the traversal's prefilter).
struct Prep8Extra {
  signed char* qf = nullptr;   // fragment-major copy: [b_pad/32][d_pad8/32][64 lanes][16 bytes]
  signed char* qf16 = nullptr; // the same in 16x16x64 order: [b_pad/16][d_pad8/64][64 lanes][16 bytes] (the 256-query row-id tile, mfma_tile16.hpp)
  u64* T2 = nullptr;           // prologue: thresholds (pairs), n2 entries, value Tv
  int64_t n2 = 0;
  u64 Tv = 0;
  u32* cnt = nullptr;          // prologue: cnt[0 .. nq) = cntv, cnt[nq .. nq + 8) = 0
  u32 cntv = 0;
  u32* gsync = nullptr;        // prologue: 256 group counters = 0
  u32* qmax = nullptr;         // [2] (zeroed by the caller): atomicMax of the float bits of |q'| and |q' - qh'| over the batch (fold8_kernel reads them)
  int* s8g = nullptr;          // one-pass form (stream8_kernel.hpp): table slots = empty, raw candidate counters = 0
  int s8_slots = S8_SLOTS;     // slots per query of that call (64 | 128)
};

// mirror_build.hip: both build or extend on demand (rows appended since the last call are converted, nothing else)
int32_t ensure_mirror(Index& ix);
int32_t ensure_mirror8(Index& ix);
// `rows` query rows (zeros beyond nq) on the 8-bit mirror's grid, in its frame.  fold: the batch's per-row margins go into m.acc0b (qmax zeroed -
// its status is returned - collected by the preparation, read by the fold launch behind it)
hipError_t prep8_queries(HalfMirror& m, bool fold, int dim, int metric, const float* q, int64_t nq, int64_t rows, signed char* q8, float* qstat, Prep8Extra px,
                         hipStream_t s);

// one_pass.hip: the static part of the rule for the one-pass search, and the search itself (*done = false: the staged chain answers)
bool one_pass_fits(const Index& ix, const HalfMirror* m8, int64_t nq, int k, int64_t n);
int32_t flat_stream8_slice(Index& ix, const float* dq, int64_t nq, int k, u64* run_keys, bool* done);

// ---- what both searches compute the same way
// key units per accumulator unit of the 8-bit pass
inline float key_unit8(int metric, float step) { return (metric == 0 ? 2.f : 1.f) * step * step; }
// fp32 rounding of the keys the threshold compares: |x|^2, |q|^2 and the re-ranked distance are each a 64-lane sum of
// d_pad/64 sequential fmas per lane plus a 6-level shuffle tree, i.e. <= (d_pad/64 + 6) * 2^-24 relative to their
// magnitude each; doubled for safety.  (A fixed 8e-6 was only enough up to d ~ 1000.)
inline float rerank_slack(int64_t dim) { return std::max(8e-6f, 2.f * (3.f * ((float)((dim + 63) / 64 * 64) / 64.f + 6.f) + 6.f) * 5.9604645e-8f); }

// A call's counters in m.cnt, behind the nq candidate counts: queries whose list overflowed, rows re-ranked (8-byte aligned), and their host copy
struct CallCounters { u32 *cnt, *overflow; unsigned long long* total; };
inline CallCounters call_counters(u32* cnt, int64_t nq) {
  CallCounters c = {cnt, cnt + nq, reinterpret_cast<unsigned long long*>(cnt + nq + 2)};
  if ((reinterpret_cast<uintptr_t>(c.total) & 7) != 0) c.total = reinterpret_cast<unsigned long long*>(cnt + nq + 3);
  return c;
}
struct CountersRead { u32 overflow = 0, pad = 0; unsigned long long total = 0; };

// the re-rank launch behind a filter pass: what both searches set the same way (theirs: fuse beyond counting, gsync, the s8_* fields)
inline RerankArgs rerank_args(const Index& ix, const HalfMirror& m, const float* dq, int64_t nq, int k, const FilterSpec& f, int cap, u64* run_keys,
                              const CallCounters& c, const float* scal, int bits) {
  // (in the struct's order: rows .. run_keys | fuse = 1: the stage's counts only, overflow, total, T_next | qstat, scal, bits, u, slack, gsync)
  return RerankArgs{ix.d_rows_, (int)ix.dim_, ix.metric_, dq, nq, k, f, m.cand.as<u32>(), c.cnt, cap, run_keys, 1, c.overflow, c.total, nullptr,
                    m.qstat.as<float>(), scal, bits, key_unit8(ix.metric_, m.step8), rerank_slack(ix.dim_), nullptr};
}
// the call's LAST re-rank writes the caller-visible result itself where search() asked for that: true = this launch does
inline bool finalize_in_rerank(const Index& ix, int64_t nq, RerankArgs* ra) {
  if (!(ix.call_.pre_sync && nq == ix.call_.nq && ix.call_.fin_ids != nullptr)) return false;
  ra->fin_ids = ix.call_.fin_ids;
  ra->fin_dist = ix.call_.fin_dist;
  ra->fin_counts = ix.call_.fin_cnt;
  ra->fin_base = ix.id_base_;
  ra->fin_stride = ix.id_stride_;
  return true;
}

}  // namespace eps
