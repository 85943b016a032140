// Host-callable launchers for the HIP kernels of libepsilla_gfx950 (definitions in *.hip).
// All pointers are device pointers unless stated otherwise; all launches are asynchronous on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "among_host.hpp"
#include "device_common.hpp"
#include "diverse_host.hpp"
#include "group_rows_host.hpp"
#include "groups_host.hpp"
#include "merge_host.hpp"
#include "multi_host.hpp"
#include "sparse_host.hpp"
#include "sparse_inv_host.hpp"

namespace eps {

// rows of `dim` floats starting at `rows` can be read in 16-byte pieces (the VEC4 form of the kernels that gather rows)
inline bool rows_vec4(const float* rows, int64_t dim) { return (dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(rows) & 15) == 0); }

// ---------------------------------------------------------------- flat scan (BruteForceSearch, :717-768)
struct FlatScanArgs {
  const float* rows;
  int64_t row_begin, row_end;   // local row range scanned
  int dim;
  int metric;
  const float* queries;         // [nq][dim]
  int64_t nq;
  int k;
  FilterSpec f;
  u64* partial;                 // [nq][W][k] per-wave sorted lists
  int W;                        // wavefronts per query = gridDim.x * 4
  const u64* thr_in;            // optional [nq] initial thresholds (only keys < thr can enter), or null
  const u64* lo_in;             // optional: only keys > lo_in[q * lo_stride] can enter (paging through results beyond 1024 per query), or null
  int64_t lo_stride;
};
// the shape of a scan over k-lists: 64-entry registers per lane of a WaveTopK, queries staged per workgroup (flat_kernels.hip, among.hip)
inline int pick_kpl(int k) { return k <= 64 ? 1 : k <= 128 ? 2 : k <= 256 ? 4 : k <= 512 ? 8 : 16; }
inline int pick_nq(int64_t nq, int k, int dim) {
  if (k > 128) return 1;
  int want = nq >= 3 ? 4 : (nq == 2 ? 2 : 1);
  // the NQ queries are staged in LDS: keep NQ * dim floats within 64 KB
  while (want > 1 && (size_t)want * ((dim + 3) & ~3) * sizeof(float) > 65536) want >>= 1;
  return want;
}
// returns W (partial lists per query). `partial` must hold nq * flat_scan_waves(...) * k keys.
int flat_scan_waves(int64_t nrows, int64_t nq, int dim);
void launch_flat_scan(const FlatScanArgs& a, hipStream_t s);

// merge the `slots` keys of each query (plus, if merge_run, the existing run_keys[q][k]) into run_keys[q][k].
// counts (optional): per-query number of valid keys at the front of its slots (candidate lists).
// seed_cand != null (the MFMA engine's seed stage, r4): instead of the k best keys, their ROWS go to seed_cand[q][0 .. count) (sample
// indices mapped by seed_row), seed_cnt[q] = count and run_keys[q] is left EMPTY - no launch of its own between the seed pass and its re-rank
void launch_merge_lists(const u64* keys, int slots, int k, int64_t nq, u64* run_keys, bool merge_run, hipStream_t s,
                        const u32* counts = nullptr, const FilterSpec* visible = nullptr, u64 id_stride = 0, u32 id_head = 0,
                        u32* seed_cand = nullptr, int seed_cap = 0, u32* seed_cnt = nullptr);

// exact fp32 re-rank of gathered candidate rows into run_keys (sorted, unique)
struct RerankArgs {
  const float* rows;
  int dim;
  int metric;
  const float* queries;     // [nq][dim]
  int64_t nq;
  int k;
  FilterSpec f;
  const u32* cand;          // [nq][cap] local row ids
  u32* cand_count;          // [nq] (may exceed cap: only min(count,cap) are present); zeroed per query when fuse is set
  int cap;
  u64* run_keys;            // [nq][k] in/out
  // Stage bookkeeping of the MFMA engine folded into the re-rank (r3; it was two tiny launches per stage): after query q's re-rank
  // the block (i) adds the stage's candidate count to the overflow / total counters, (ii) computes the NEXT stage's pass threshold
  // from the query's new k-th best exact key, (iii) zeroes the query's candidate count and (block 0) the group arrival counters
  // for the next filter launch.  fuse = 0: none of it.
  int fuse;
  u32* overflow;            // [1]
  unsigned long long* total;   // [1]
  void* T_next;             // float [b_pad] (fp16 operands) / int [b_pad] (int8 operands), or null after the last stage
  const float* qstat;       // [b_pad][4]
  const float* scal;        // the mirror's maxima
  int bits;                 // 8 | 16
  float u, slack;
  u32* gsync;               // [256] or null
  // the call's LAST re-rank also converts the result keys (ids = local * stride + base, distances, counts): finalize_kernel's work
  // without its launch (r4: a single-query call is a chain of short dependent launches); fin_ids == null: not this launch
  int64_t* fin_ids = nullptr;
  float* fin_dist = nullptr;
  int32_t* fin_counts = nullptr;
  int64_t fin_base = 0, fin_stride = 1;
  // one-pass search of a handful of queries (stream8_kernel.hpp): the launch first SELECTS its candidates - the entries of the pass's
  // per-wavefront lists that still pass against the final table of best accumulators - into `cand` (written through s8_cand), starts
  // from an empty running list, and counts a lost list entry as an overflow.  s8_G == null: an ordinary re-rank
  const int* s8_G = nullptr;        // [nq][s8_slots]
  int s8_slots = 64;                // 64 (k <= 16) | 128 (k = 17..64): Stream8Args::slots
  const u32* s8_counts = nullptr;   // [nq][s8_waves]
  const u64* s8_lists = nullptr;    // [nq][s8_waves][S8_WAVE_CAP]
  int s8_waves = 0;
  u32* s8_cand = nullptr;           // = cand
  // one-pass form: the block that finishes last (ticket) copies overflow / total to host-mapped words [0] = overflow, [2..3] = total, so the
  // caller needs no device-to-host copy after the launch (a copy is a trip through the DMA queue at the end of a 0.2 ms call)
  u32* pub = nullptr;               // host-mapped [4], or null
  u32* pub_ticket = nullptr;        // device word, zero at launch
  int s8_fast = 0;                  // 1: s8_rerank_kernel (r5, late: the one-pass call's own re-rank); 0: rerank_kernel's s8 prologue (A/B)
  int s8_reset = 0;                 // 1: the launch leaves the one-pass state as the next call needs it (table slots empty, counters zero): no prep launch then
};
void launch_rerank(const RerankArgs& a, hipStream_t s);

// run_keys -> caller-visible results: ids = local*stride+base (int64), dist fp32, counts int32
void launch_finalize(const u64* run_keys, int64_t nq, int k, int64_t id_base, int64_t id_stride, int64_t* ids,
                     float* dist, int32_t* counts, hipStream_t s);

void launch_normalize(float* rows, int64_t n, int dim, bool only_if_nonzero, hipStream_t s);
void launch_merge_shards(const float* dist, const int64_t* ids, int shards, int64_t nq, int k, float* out_dist,
                         int64_t* out_ids, hipStream_t s, int64_t stride_bytes = 0, int32_t* out_counts = nullptr);
void launch_fill_u64(u64* p, int64_t n, u64 v, hipStream_t s);

// ---------------------------------------------------------------- ordered select (SearchByAttribute's full scan, :1016-1029; select.hip)
constexpr int SEL_ROWS = 1024;          // rows per block of the verdict and scatter launches = rows per block count
constexpr int SEL_THREADS = 256;        // threads of such a block: every wavefront judges SEL_ROWS / SEL_THREADS words of 64 rows
constexpr int SEL_SCAN_THREADS = 512;   // block counts the scan's one workgroup takes per round of its loop
inline int64_t select_blocks(int64_t n) { return (n + SEL_ROWS - 1) / SEL_ROWS; }
struct SelectArgs {
  FilterSpec f;          // prog_use_dist = 0: @distance reads as 0
  int64_t n;             // rows [0, n) are judged, 0 < n < 2^31
  int64_t skip, limit;   // the window over the visible rows' ranks; both <= n
  int64_t id_base, id_stride;
  u64* bits;             // [select_blocks(n) * SEL_ROWS / 64] visibility bitset (bit set = visible)
  u32* counts;           // [select_blocks(n)]
  int64_t* offsets;      // [select_blocks(n) + 1]
  int64_t* ids_out;      // [limit]
  int64_t* count_out;    // [1] clamp(total - skip, 0, limit)
  int64_t* total_out;    // [1] visible rows of the whole table, or null
};
// verdict, scan, scatter (the last only when limit > 0)
void launch_select(const SelectArgs& a, hipStream_t s);

// ---------------------------------------------------------------- radius search (eps_index_search_range; range.hip)
constexpr int RANGE_MAX_CAP = 8192;          // results per query: one workgroup orders a query's keys in LDS, 64 KB of them
constexpr u32 RANGE_CNT_RESCAN = ~0u;        // a query's survivor count while its candidate list was too short to be trusted
enum : u32 { RANGE_DONE = 0, RANGE_RESCAN = 1, RANGE_TOPK = 2 };   // per-query status the order launch leaves for the host
// the survivors of every query: rows with dist <= radius that are visible.  cnt[j] counts ALL of them (the query's total), the first `cap` to
// arrive have their (distance, row) key in keys[j][..], in no order.
struct RangeLists {
  u64* keys;             // [nq][cap]
  u32* cnt;              // [nq]
  const float* radius;   // [nq]
  int cap;
};
struct RangeRerankArgs {   // the tail of the matrix form: exact distances of the filter pass's candidates
  const float* rows;
  int dim, metric;
  const float* queries;    // [nq][dim]
  int64_t nq;
  FilterSpec f;
  const u32* cand;         // [nq][cand_cap] row ids, unordered
  const u32* cand_count;   // [nq] rows that passed the filter (may exceed cand_cap)
  int cand_cap;
  RangeLists L;
  unsigned long long* cand_total;   // [1] += candidates given an exact distance
};
void launch_range_rerank(const RangeRerankArgs& a, hipStream_t s);
struct RangeScanArgs {     // the stream form: every row against blocks of queries
  const float* rows;
  int64_t n;
  int dim, metric;
  const float* queries;    // [..][dim], indexed by query number
  int64_t nq;              // queries of this launch
  const int32_t* qsel;     // [nq] their query numbers, or null: 0 .. nq - 1
  FilterSpec f;
  RangeLists L;            // indexed by query number
};
void launch_range_scan(const RangeScanArgs& a, hipStream_t s);
struct RangeOrderArgs {
  int64_t nq;              // queries of this launch
  const int32_t* qsel;     // [nq] their query numbers, or null
  RangeLists L;
  const u64* topk;         // null: order the query's list (where it holds every survivor); else [nq][cap] sorted keys of launch-local query i: cut at the radius
  u32* status;             // [..] RANGE_*, by query number
  int64_t id_base, id_stride;
  int64_t* ids_out;        // [..][cap]
  float* dist_out;         // [..][cap]
  int32_t* counts_out;     // [..] or null
  int64_t* totals_out;     // [..] or null
};
void launch_range_order(const RangeOrderArgs& a, hipStream_t s);
// the queries named by qsel, copied next to each other (out, may be null); zero_cnt: their survivor counts start again at 0
void launch_range_gather(const float* queries, int dim, const int32_t* qsel, int64_t m, float* out, u32* cnt, bool zero_cnt, hipStream_t s);

// ---------------------------------------------------------------- search among given rows (eps_index_search_among; among.hip, plan: among_host.hpp)
struct AmongArgs {
  const float* rows;
  int64_t n_rows;            // > 0: an id names row (id - id_base) / id_stride if that is a whole number below n_rows, else no row
  int dim, metric;
  const float* queries;      // [nq][dim]
  int64_t nq;
  int k;
  FilterSpec f;
  const int64_t* ids;        // the lists' entries, global ids
  const int64_t* offsets;    // [nq + 1] query j's list = ids[offsets[j] .. offsets[j + 1]); null: ids[0 .. n_cand) for every query
  int64_t n_cand;
  int64_t id_base, id_stride;
  AmongPlan plan;
  u64* partial;              // [nq][plan.W][k] per-wavefront sorted lists of unique keys
  unsigned long long* evals; // [1] += (row, query) pairs given a distance
};
// the gather (in slices of AMONG_GRID_Y query tiles), then the merge of every query's partial lists into run_keys[nq][k]: sorted, unique
void launch_among_gather(const AmongArgs& a, hipStream_t s);
void launch_among_merge(const u64* partial, int W, int k, int64_t nq, u64* run_keys, hipStream_t s);

// ---------------------------------------------------------------- grouped search (eps_index_search_groups; groups.hip, plan: groups_host.hpp)
constexpr u32 GROUPS_UNFINISHED = 1;   // a query's status while it holds fewer than k representatives and its last page was full
struct GroupsFirstArgs {     // one round of the page engine: the first occurrences of a page's labels, appended to the queries' results
  const u64* page;           // [m][P] launch-local query i's page: ascending keys, KEY_EMPTY behind the last
  int P;
  int64_t m;                 // queries of this launch
  const int32_t* qsel;       // [m] their query numbers, or null: 0 .. m - 1
  const int32_t* label;      // [n_rows]
  int k;
  u64* res_keys;             // [..][k] by query number: the representatives so far, ascending, KEY_EMPTY behind them
  u32* res_cnt;              // [..]
  u32* status;               // [..] GROUPS_UNFINISHED or 0
  u64* lo;                   // [..] the page's last key: the next page continues after it
};
void launch_groups_first(const GroupsFirstArgs& a, hipStream_t s);
// the queries whose status is GROUPS_UNFINISHED, in ascending order: qsel[0 .. *m_out), *m_out (a host-mapped word) their number.  One workgroup
void launch_groups_compact(const u32* status, int64_t nq, int32_t* qsel, u32* m_out, hipStream_t s);
// the queries named by qsel and their continuation keys, copied next to each other
void launch_groups_gather(const float* queries, int dim, const u64* lo, const int32_t* qsel, int64_t m, float* q_out, u64* lo_out, hipStream_t s);
struct GroupsScanArgs {      // the scan engine: every visible row offers its key to its group's slot
  const float* rows;
  int64_t n;
  int dim, metric;
  const float* queries;      // [..][dim], indexed by query number
  int64_t m;                 // queries of this launch (one chunk of the plan)
  const int32_t* qsel;       // [m] their query numbers, or null: 0 .. m - 1
  FilterSpec f;
  const int32_t* label;      // [n]
  u64* best;                 // [m][G] launch-local query i's slots, KEY_EMPTY before the launch
  int64_t G;
  int W;                     // wavefronts over the rows = gridDim.x * 4
};
void launch_groups_min_scan(const GroupsScanArgs& a, hipStream_t s);
// partial[i][w][k] = the k smallest keys of slice w of query i's slots (sorted, KEY_EMPTY behind them)
void launch_groups_table_topk(const u64* best, int64_t G, int64_t m, int k, const GroupsScanPlan& plan, u64* partial, hipStream_t s);
// res_keys[qsel[i]][..] = run_keys[i][..] (qsel null: i)
void launch_groups_scatter(const u64* run_keys, int k, const int32_t* qsel, int64_t m, u64* res_keys, hipStream_t s);
// group_keys[q][e] = key_of_label[label[row of res_keys[q][e]]], 0 where the slot is unused
void launch_groups_keys(const u64* res_keys, int64_t nq, int k, const int32_t* label, const int64_t* key_of_label, int64_t* group_keys, hipStream_t s);

// ---------------------------------------------------------------- m rows per group (eps_index_search_group_rows; group_rows.hip, plan: group_rows_host.hpp)
// the rows of every label next to each other: offsets[G + 1], group_rows[n] (any order inside a group); cursor: G words, zero before the launch
void launch_group_rows_build(const int32_t* label, int64_t n, int64_t G, u32* cursor, int64_t* offsets, int32_t* group_rows, hipStream_t s);
struct GroupRowsArgs {         // one pass of the second phase: the m closest visible rows of every (query, slot) pair's group
  const float* rows;
  int dim, metric;
  const float* queries;        // [pairs / k][dim]: the pass's queries
  int64_t pairs;               // queries of the pass * k
  int k, m;
  FilterSpec f;
  const u64* res_keys;         // [pairs] the first phase's representatives, KEY_EMPTY where a query has fewer than k groups
  const int32_t* label;        // [n]
  const int64_t* offsets;      // [G + 1]
  const int32_t* group_rows;   // [n]
  int64_t chunk;               // rows of a group per work item
  u32* prefix;                 // [pairs + 1] work items of the pairs in front; [pairs]: all of them (written by the launch, never read by the host)
  u32* sizes;                  // [pairs] visible rows of the pair's group: zero before the launch
  u64* partial;                // [items][m] a sorted list per work item
  int64_t items;               // the plan's bound on the work items
  int64_t waves;               // wavefronts of the gather's grid
  u64* run_keys;               // [pairs][m] the merged lists
  unsigned long long* evals;   // (row, query) pairs given a distance, added to
};
// the work list, then the gather over it
void launch_group_rows_gather(const GroupRowsArgs& a, hipStream_t s);
void launch_group_rows_merge(const GroupRowsArgs& a, hipStream_t s);
// ids [pairs][m] through the id map, dist [pairs][m], row_counts [pairs], group_sizes [pairs] (may be null), counts [pairs / k] (may be null)
void launch_group_rows_finalize(const GroupRowsArgs& a, int64_t id_base, int64_t id_stride, int64_t* ids, float* dist, int32_t* row_counts,
                                int64_t* group_sizes, int32_t* counts, hipStream_t s);

// ---------------------------------------------------------------- multi-vector search (eps_index_search_multi; multi.hip, plan: multi_host.hpp)
struct MultiArgs {             // one pass: whole bags [j0, j0 + bags) of the call's nq
  const float* rows;
  int dim, metric;
  FilterSpec f;
  const float* vectors;        // [T][dim] the vectors of every bag of the call
  const int64_t* q_off;        // [nq + 1] bag j = vectors[q_off[j] .. q_off[j + 1])
  int64_t j0, bags;
  int k;
  int64_t G;                   // labels
  // the pass's table of minimum keys, KEY_EMPTY before the launches.  Whole-table form: best[vector of the pass][G].  Candidate form:
  // pair_best[(bag, candidate) pair][t of the bag], bag j's pairs from element base_off[j] - base_off[j0]
  u64* table;
  const int64_t* base_off;     // [nq + 1] whole-table form: q_off; candidate form: table elements in front of bag j's pairs
  MultiTopkPlan plan;          // how the table's columns (labels; a bag's candidates) are cut among the read-back's wavefronts
  u64* partial;                // [bags][plan.W][k]
  u64* run_keys;               // [bags][k] make_key(score, label), sorted, unique
  // candidate form only (cand_label == null: the whole-table form)
  const int32_t* cand_label;   // [n_cand] the label a candidate key names, -1: none
  const int64_t* cand_off;     // [nq + 1] bag j's candidates = [cand_off[j], cand_off[j + 1]); null: [0, n_cand) for every bag
  int64_t n_cand;
  int64_t pairs;               // (bag, candidate) pairs of the pass
  const int64_t* offsets;      // [G + 1] the rows by group (group_rows.hip)
  const int32_t* group_rows;   // [n]
  unsigned long long* prefix;  // [pairs + 1] work items of the pairs in front; [pairs]: all of them (written by the launch, never read by the host)
  int64_t waves;               // wavefronts of the gather's grid
  unsigned long long* evals;   // (row, vector) pairs given a distance, added to
};
// cand_label[i] = the label whose key is cand_keys[i], -1 where no group has that key
void launch_multi_labels(const int64_t* cand_keys, int64_t n_cand, const int64_t* key_of_label, int64_t G, int32_t* cand_label, hipStream_t s);
// candidate form: the work list, then the gather over it into a.table
void launch_multi_gather(const MultiArgs& a, hipStream_t s);
// the table's columns into a.partial: per bag and wavefront the k smallest make_key(sum of the column's minima, label)
void launch_multi_sum_topk(const MultiArgs& a, hipStream_t s);
// a.run_keys -> group_keys [nq][k], score [nq][k], counts [nq] (may be null) and, read back from a.table, the matches (both null or neither):
// bag j, slot s, vector u at k * q_off[j] + s * t_j + u
void launch_multi_finalize(const MultiArgs& a, const int64_t* key_of_label, int64_t id_base, int64_t id_stride, int64_t* group_keys, float* score,
                           int32_t* counts, int64_t* match_ids, float* match_dist, hipStream_t s);

// ---------------------------------------------------------------- diverse search (eps_index_search_diverse; diverse.hip, layout: diverse_host.hpp)
struct DiverseArgs {
  const float* rows;
  int dim, metric;
  const u64* pool;             // [nq][fetch_k] every query's pool: ascending keys, KEY_EMPTY behind them
  int64_t nq;
  int fetch_k, k;
  float lam, mu;               // lambda, and 1.0f - lambda as the host rounded it
  u64* sel_keys;               // [nq][k] the pool keys of the selected rows in selection order, KEY_EMPTY behind them
  float* score;                // [nq][k] their scores at selection, +inf behind them; may be null
  unsigned long long* evals;   // (row, selected row) pairs given a distance, added to
};
// one workgroup per query (in slices of DIVERSE_GRID queries): the greedy selection over the pool
void launch_diverse_select(const DiverseArgs& a, hipStream_t s);

// ---------------------------------------------------------------- sparse-vector scan (eps_sparse_index_*; sparse.hip, plan: sparse_host.hpp)
struct SparseVerdict {          // what sparse_validate_kernel leaves: ~0 / 0 before the launch
  u64 first_bad;                // min over offending rows of (row << 3 | SPARSE_BAD_*), or ~0
  u64 longest;                  // the longest row
};
struct SparseValidateArgs {
  const int64_t* offsets;       // [n + 1]
  const int32_t* indices;       // [nnz]
  const float* values;          // [nnz]
  int64_t n, nnz, dim;
  float* norms;                 // [n] every row's sum of squares, added in stored order, or null
  SparseVerdict* verdict;
};
void launch_sparse_validate(const SparseValidateArgs& a, hipStream_t s);
struct SparseScanArgs {
  const int64_t* offsets;       // the table, as sparse_validate_kernel passed it
  const int32_t* indices;
  const float* values;
  const float* norms;           // [n]
  int64_t n;
  int metric;
  const int64_t* q_offsets;     // [nq + 1] the queries, validated
  const int32_t* q_indices;
  const float* q_values;
  int64_t nq;
  int k;
  FilterSpec f;                 // the deleted bitset only
  SparsePlan plan;
  u64* partial;                 // [nq][plan.W][k] per-wavefront sorted lists
};
void launch_sparse_scan(const SparseScanArgs& a, hipStream_t s);

// ---------------------------------------------------------------- inverted lists of a sparse table (eps_sparse_index_build_inverted; sparse_inverted.hip, plan: sparse_inv_host.hpp)
struct SparseInvBuildArgs {
  const int64_t* offsets;       // the validated CSR
  const int32_t* indices;
  const float* values;
  int64_t n, nnz, dim;
  int64_t* col_offsets;         // [dim + 1] out
  SparsePosting* postings;      // [nnz] out: the CSR's elements in (column, row) order
  SparsePosting* pairs;         // [nnz] scratch: the sort's payload ping-pongs between it and `postings`
  int32_t* keys_a;              // [nnz] scratch (sparse_inv_bytes: unused below two passes)
  int32_t* keys_b;              // [nnz] scratch (unused below three passes)
  u64* table;                   // [256][sort blocks] scratch
  u64* longest;                 // [1] out: the longest column (zeroed by the launcher)
};
hipError_t launch_sparse_inv_build(const SparseInvBuildArgs& a, hipStream_t s);
struct SparseInvArgs {
  const int64_t* col_offsets;   // the image
  const SparsePosting* postings;
  const float* norms;           // [n]
  int64_t n;
  int metric;                   // 1 COSINE, 2 DOT_PRODUCT
  const int64_t* q_offsets;     // [nq + 1] the queries, validated
  const int32_t* q_indices;
  const float* q_values;
  int64_t nq;
  int k;
  FilterSpec f;                 // the deleted bitset only
  SparseInvPlan plan;
  u64* partial;                 // [nq][plan.rows.W][k] per-wavefront sorted lists
};
void launch_sparse_inverted(const SparseInvArgs& a, hipStream_t s);

// ---------------------------------------------------------------- windowed merge of sorted lists by rank (eps_merge_range, eps_merge_select; merge_lists.hip)
// a.dist != null: the radius form, else the select form (MergeRankArgs: merge_host.hpp); one launch
void launch_merge_rank(const MergeRankArgs& a, hipStream_t s);

}  // namespace eps
