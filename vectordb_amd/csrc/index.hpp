// Host side of libepsilla_gfx950: the per-field index object behind the C ABI (include/epsilla_gfx950.h).
// It plays the role of one VecSearchExecutor + its ANNGraphSegment (reference:
// engine/db/execution/vec_search_executor.hpp:30-74, engine/db/ann_graph_segment.hpp:22-55) with the
// vector table, graph and scratch mirrored in HBM.
#pragma once
#include <atomic>
#include <thread>
#include <mutex>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/epsilla_gfx950.h"
#include "kernels.hpp"
#include "result_block.hpp"

namespace eps {

struct DevBuf {  // growable device allocation
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf();
  // returns false on allocation failure
  bool reserve(size_t bytes);
  // a new allocation of `want` bytes (sized as reserve sizes it) whose first `keep` bytes are the old one's, complete when this returns;
  // hipErrorOutOfMemory: nothing changed
  hipError_t grow_keeping(size_t want, size_t keep, hipStream_t s);
  void release();
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// Reclaimable scratch (r6): a device allocation that only makes a path faster (the traversal's visited stamps: 4 bytes x nodes x slots,
// tens of GB) is registered here with a flag its owner holds while host code is about to launch kernels on it.  When ANY DevBuf::reserve of the
// process fails, every registered buffer whose owner is not in that window is released (hipFree waits for the kernels already launched) and
// the allocation is tried again; the owner finds its buffer gone at its next search and takes the form that needs no such table.
struct ScratchClaim {
  DevBuf* buf = nullptr;
  ScratchClaim();
  ~ScratchClaim();
  ScratchClaim(const ScratchClaim&) = delete;
  ScratchClaim& operator=(const ScratchClaim&) = delete;
  // The owner's window (from "is the table there?" to its last launch on it) and the reclaimer's release exclude each other.  enter(): the owner -
  // WAITS for a release in progress on another thread; false = this thread is already inside (a nested call: nothing to take, nothing to give back).
  // try_enter(): the reclaimer - never waits, never takes what its own thread is using.
  bool enter() {
    if (holder_.load() == std::this_thread::get_id()) return false;
    mu_.lock();
    holder_.store(std::this_thread::get_id());
    return true;
  }
  bool try_enter() {
    if (holder_.load() == std::this_thread::get_id() || !mu_.try_lock()) return false;
    holder_.store(std::this_thread::get_id());
    return true;
  }
  void leave() {
    holder_.store(std::thread::id());
    mu_.unlock();
  }

 private:
  std::mutex mu_;
  std::atomic<std::thread::id> holder_{};
};
size_t scratch_reclaim();   // bytes released

// Engine-selection switches (eps_set_tuning, include/epsilla_gfx950.h): the value of `name` in the process-wide table, or null.  The
// library never reads the environment.
const char* tune_env(const char* name);
// the integer value of a switch, read ONCE (a second lookup may find the entry gone: eps_set_tuning is a process-wide runtime call), or `dflt`
int tune_int(const char* name, int dflt);
void tune_set(const char* name, const char* value);   // eps_set_tuning: value null removes the entry, name null empties the table

struct BuildStage;   // stage-level entry of the graph build (below)
struct Quant8View {   // the table's 8-bit mirror as other kernels see it (mirror_build.hip)
  const signed char* x8 = nullptr;
  const int* acc0 = nullptr;
  const float* scal8 = nullptr;
  const float* mu = nullptr;   // [d_pad8] the grid's centre (one value per column)
  int d_pad8 = 0;
  int cols8 = 0;          // columns of a mirror row that carry values: dim (identity frame), dim rounded up to 256 (rotated frame, r6) - what a kernel that reads
                          // a row's leading bytes only (the traversal's prefilter) must cover
  float step = 1.f, u = 1.f;
  int64_t epoch8 = 0;     // counts the mirror's (re)builds: row constants copied elsewhere (the graph's edge constants) are stale when it moves
  bool per_batch = false; // acc0 carries per-batch margins (fold8): it changes with every batch of queries
};
struct HalfMirror;   // fp16 + 8-bit mirrors and per-row bounds for the MFMA filter engine (mirror.hpp, built in mirror_build.hip)
struct GraphDev;     // device CSR + traversal scratch (traverse.hip)

// What the C ABI dispatches to: one device index, or a group of them over a hash-sharded table (shard_group.cpp).
class IndexBase {
 public:
  virtual ~IndexBase() {}
  virtual int32_t set_stream(void* s) = 0;
  virtual int32_t synchronize() = 0;
  virtual int32_t attach_rows(const float* rows, int64_t n) = 0;
  virtual int32_t append_rows(const float* rows, int64_t n_new) = 0;
  // rows of one shard of a hash-sharded index (local row l = global row l * shards + shard); a plain index is its own shard 0
  virtual int32_t attach_shard_rows(int32_t shard, const float* rows, int64_t n_local) = 0;
  // an OWNED device copy of the first n rows of `src` (an index of the same kind on the same device(s)): what a build on the side
  // works on while `src` keeps serving and growing
  virtual int32_t clone_rows(IndexBase& src, int64_t n) = 0;
  virtual int32_t set_id_map(int64_t base, int64_t stride) = 0;
  virtual int32_t set_deleted(const uint8_t* bits, int64_t nbytes) = 0;
  virtual int32_t set_int_filter(const void* column, int64_t stride, int32_t width, int32_t op, int64_t constant) = 0;
  virtual int32_t set_filter_program(const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride, int64_t n_rows, int32_t flags = 0) = 0;
  virtual int32_t build(int64_t n, const eps_build_params* p) = 0;
  virtual int32_t set_graph(int64_t n, const int64_t* off, const int64_t* nbr, int64_t nav) = 0;
  virtual int32_t graph_info(int64_t* n, int64_t* edges, int64_t* nav) const = 0;
  virtual int32_t get_graph(int64_t* off, int64_t* nbr) const = 0;
  virtual int32_t save_graph(const char* path) = 0;
  virtual int32_t load_graph(const char* path) = 0;
  virtual int32_t search(const float* queries, int64_t nq, int32_t k, const eps_search_params* p, int64_t* ids, float* dist,
                         int32_t* counts, int32_t walk_limit = 0) = 0;
  // the grouped search (eps_index_set_groups / _search_groups / _groups_info; groups.hip): a single-device index serves it, a shard group refuses
  virtual int32_t set_groups(const int64_t* keys, int64_t n) = 0;
  virtual int32_t search_groups(const float* queries, int64_t nq, int32_t k, const eps_search_params* p, int32_t engine, int32_t page_rows,
                                int64_t scratch_bytes, int64_t* ids_out, float* dist_out, int64_t* group_keys_out, int32_t* counts_out) = 0;
  virtual int32_t groups_info(int64_t* n_groups, int64_t* largest_group, int32_t* last_engines, int64_t* last_scan_queries) = 0;
  virtual int32_t search_group_rows(const float* queries, int64_t nq, int32_t k, int32_t m, const eps_search_params* p, int32_t engine, int32_t page_rows,
                                    int64_t scratch_bytes, int64_t* ids_out, float* dist_out, int64_t* group_keys_out, int32_t* row_counts_out,
                                    int64_t* group_sizes_out, int32_t* counts_out) = 0;
  virtual int32_t search_multi(const float* vectors, const int64_t* q_offsets, int64_t nq, const int64_t* cand_keys, const int64_t* cand_offsets,
                               int64_t n_cand, int32_t k, int64_t scratch_bytes, int64_t* group_keys_out, float* score_out, int32_t* counts_out,
                               int64_t* match_ids_out, float* match_dist_out) = 0;
  virtual int32_t search_diverse(const float* queries, int64_t nq, int32_t k, int32_t fetch_k, float lambda, const int64_t* cand_ids,
                                 const int64_t* cand_offsets, int64_t n_cand, const eps_search_params* p, int64_t* ids_out, float* dist_out,
                                 float* score_out, int32_t* counts_out) = 0;
  virtual int64_t row_count() const = 0;
  virtual int32_t last_stats(eps_search_stats* out) = 0;
  virtual int kernel_times(double* ms_out, int cap) = 0;
  const char* last_error() const { return err_.c_str(); }
  int32_t last_error_class() const { return err_class_; }
  int32_t fail(int32_t code, const std::string& msg, int32_t err_class = 0) {
    err_ = msg;
    err_class_ = err_class;
    return code;
  }
  std::string err_;
  int32_t err_class_ = 0;   // EPS_ERRCLASS_* of the last failure (eps_index_last_error_class)
};

class Index : public IndexBase {
 public:
  Index(int64_t dim, int metric, int device);
  ~Index();

  int32_t init();
  int32_t set_stream(void* s) override;
  int32_t synchronize() override;
  int32_t attach_rows(const float* rows, int64_t n) override;
  int32_t attach_shard_rows(int32_t shard, const float* rows, int64_t n_local) override {
    if (shard != 0) return fail(EPS_USER_ERROR, "attach_shard_rows: not a sharded index (only shard 0 exists)");
    return attach_rows(rows, n_local);
  }
  int32_t clone_rows(IndexBase& src, int64_t n) override;
  // rows of a strided host table: row i at rows + i*pitch_floats (hash-sharded tables: pitch = shards*dim)
  int32_t attach_rows_strided(const float* rows, int64_t n, int64_t pitch_floats, bool copy_device_rows = false);
  int32_t append_rows_strided(const float* rows, int64_t n_new, int64_t pitch_floats);
  int32_t append_rows(const float* rows, int64_t n_new) override;
  int32_t set_id_map(int64_t base, int64_t stride) override;
  int32_t set_deleted(const uint8_t* bits, int64_t nbytes) override;
  int32_t set_int_filter(const void* column, int64_t stride, int32_t width, int32_t op, int64_t constant) override;
  int32_t set_filter_program(const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride, int64_t n_rows, int32_t flags = 0) override;
  int32_t set_filter_program_pitched(const eps_filter_op* ops, int32_t nops, const void* rows, int64_t src_pitch, int64_t row_bytes, int64_t n_rows,
                                     int32_t flags);
  int32_t build(int64_t n, const eps_build_params* p) override;
  int32_t set_graph(int64_t n, const int64_t* off, const int64_t* nbr, int64_t nav) override;
  int32_t graph_info(int64_t* n, int64_t* edges, int64_t* nav) const override;
  int32_t get_graph(int64_t* off, int64_t* nbr) const override;
  int32_t save_graph(const char* path) override;
  int32_t load_graph(const char* path) override;
  int32_t last_stats(eps_search_stats* out) override;
  int32_t load_table(const char* path, const eps_table_layout* layout, int64_t* n_out);
  // walk_limit > 0: candidate-walk form (eps_index_search_walk): k = cap, the tail merge uses searchLimit(walk_limit)
  int32_t search(const float* queries, int64_t nq, int32_t k, const eps_search_params* p, int64_t* ids, float* dist,
                 int32_t* counts, int32_t walk_limit = 0) override;

  // the visible rows in ascending row order, windowed by [skip, skip + limit): SearchByAttribute's full scan (eps_index_select; select.hip)
  int32_t select(int64_t skip, int64_t limit, int64_t* ids_out, int64_t* count_out, int64_t* total_out);
  // every visible row within radius[j] of query j: the total, and the cap closest in (distance, id) order (eps_index_search_range; range.hip)
  int32_t search_range(const float* queries, int64_t nq, const float* radius, int32_t cap, const eps_search_params* p, int64_t* ids_out, float* dist_out,
                       int32_t* counts_out, int64_t* totals_out);

  // the k closest visible rows among the ids the caller names: one list for the batch, or one per query (eps_index_search_among; among.hip)
  int32_t search_among(const float* queries, int64_t nq, const int64_t* cand_ids, const int64_t* cand_offsets, int64_t n_cand, int32_t k,
                       int64_t* ids_out, float* dist_out, int32_t* counts_out);

  // the k closest groups of rows, each by its closest visible row (eps_index_search_groups; groups.hip, plan: groups_host.hpp)
  int32_t set_groups(const int64_t* keys, int64_t n) override;
  int32_t search_groups(const float* queries, int64_t nq, int32_t k, const eps_search_params* p, int32_t engine, int32_t page_rows, int64_t scratch_bytes,
                        int64_t* ids_out, float* dist_out, int64_t* group_keys_out, int32_t* counts_out) override;
  int32_t groups_info(int64_t* n_groups, int64_t* largest_group, int32_t* last_engines, int64_t* last_scan_queries) override;
  // ... and of each of them its m closest visible rows and the number of its visible rows (eps_index_search_group_rows; group_rows.hip, plan:
  // group_rows_host.hpp)
  int32_t search_group_rows(const float* queries, int64_t nq, int32_t k, int32_t m, const eps_search_params* p, int32_t engine, int32_t page_rows,
                            int64_t scratch_bytes, int64_t* ids_out, float* dist_out, int64_t* group_keys_out, int32_t* row_counts_out, int64_t* group_sizes_out,
                            int32_t* counts_out) override;
  // the k closest groups per BAG of vectors, by the sum over the bag of each vector's distance to the group's closest visible row; over every
  // group or over the groups the caller names (eps_index_search_multi; multi.hip, plan: multi_host.hpp)
  int32_t search_multi(const float* vectors, const int64_t* q_offsets, int64_t nq, const int64_t* cand_keys, const int64_t* cand_offsets, int64_t n_cand,
                       int32_t k, int64_t scratch_bytes, int64_t* group_keys_out, float* score_out, int32_t* counts_out, int64_t* match_ids_out,
                       float* match_dist_out) override;

  // k rows of a query's pool - a flat search's fetch_k closest, or search_among's over the caller's lists - by maximal marginal relevance
  // (eps_index_search_diverse; diverse.hip, layout: diverse_host.hpp)
  int32_t search_diverse(const float* queries, int64_t nq, int32_t k, int32_t fetch_k, float lambda, const int64_t* cand_ids, const int64_t* cand_offsets,
                         int64_t n_cand, const eps_search_params* p, int64_t* ids_out, float* dist_out, float* score_out, int32_t* counts_out) override;

  int64_t row_count() const override { return n_rows_; }

  // ---- used by the engine translation units
  int32_t hip_fail(hipError_t e, const char* what);
  FilterSpec filter_spec() const;

  int64_t dim_;
  int metric_;
  int device_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;

  // vector table mirror: row-major float[n_rows_][dim_] (engine/db/table_segment_mvp.cpp:106-111)
  const float* d_rows_ = nullptr;
  DevBuf rows_buf_;          // owns the storage when rows were attached from host memory
  bool rows_owned_ = false;
  int64_t n_rows_ = 0;
  int64_t rows_version_ = 0;  // bumped on attach/append (invalidates the fp16 mirror)
  // FLAT_AUTO, single-query traffic on a table without a mirror: searches seen on this rows version (flat_mfma_profitable with count_call:
  // after a few of them the 8-bit mirror is worth its HBM - the one-pass search answers such a call in a third of the stream scan's time)
  int64_t small_calls_version_ = -1;
  int small_calls_ = 0;
  int64_t scan_limit_ = -1;   // >= 0: flat engines scan rows [0, scan_limit_) only (graph build over a prefix)

  int64_t id_base_ = 0, id_stride_ = 1;

  const uint8_t* d_deleted_ = nullptr;
  DevBuf deleted_buf_;
  const uint8_t* d_fcol_ = nullptr;
  DevBuf fcol_buf_;
  int64_t f_stride_ = 0;
  int32_t f_width_ = 0, f_op_ = 0;
  int64_t f_value_ = 0;
  DevBuf prog_buf_, prog_rows_buf_;   // compiled filter program + (when handed over from the host) the attribute rows
  const uint8_t* d_prog_rows_ = nullptr;
  const void* prog_rows_host_ = nullptr;   // host table the cached device copy mirrors (append-only)
  int64_t prog_rows_stride_ = 0, prog_rows_pitch_ = 0, prog_rows_uploaded_ = 0;
  int64_t loaded_attr_rows_ = 0, loaded_attr_stride_ = 0;   // attribute rows kept by load_table
  int64_t prog_stride_ = 0, prog_rows_n_ = 0;
  int32_t prog_len_ = 0;
  bool prog_uses_dist_ = false;
  bool prefilter_call_ = false;

  // graph (reference layout kept on the host for get/save; device form in GraphDev)
  int64_t n_indexed_ = 0;
  int64_t nav_ = 0;
  std::vector<int64_t> h_off_, h_nbr_;
  GraphDev* graph_ = nullptr;

  HalfMirror* mirror_ = nullptr;

  // scratch
  // out_block_: the result block of whichever call with host result pointers is running (ResultBlock, result_block.hpp: every such call ends in
  // a stream sync and the calls of one index follow one another, so one buffer serves them all)
  DevBuf q_buf_, partial_buf_, run_buf_, out_block_, tmp_buf_, page_buf_;
  // r5: that block goes to the host in ONE copy into page-locked memory and is split there (three pageable device-to-host copies staged separately
  // cost a batch of 1024 ~0.1 ms and a single-vector call three trips through the DMA queue)
  struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~HostBuf();
    bool reserve(size_t bytes);
  } h_out_, h_q_, h_rng_, h_evals_;   // (h_q_: host queries are copied to page-locked memory first, then DMA'd: the runtime's own path for pageable sources is slower)
  DevBuf sel_bits_, sel_scan_;   // select(): visibility bitset; block counts | offsets
  // search_range(): survivor keys [nq][cap]; survivor counts | status | candidates re-ranked (what the host reads back); radii | fall-back query
  // numbers.  h_rng_: the page-locked side of the last two
  DevBuf rng_keys_, rng_cnt_, rng_in_;
  // search_among(), search_diverse(): [pair counter | offsets | a host list's ids]; among_keys: the lists, gather and merge the two share
  DevBuf among_in_;
  int32_t among_keys(const char* who, const float* dq, int64_t nq, const int64_t* cand_ids, const int64_t* cand_offsets, int64_t n_cand, int32_t k,
                     int64_t longest, bool call_syncs, unsigned long long** d_evals_out);
  // search_diverse(): the selected rows' keys [nq][k] (its pool is run_buf_, its pair counter among_in_'s)
  DevBuf div_sel_;
  // search_among(), search_group_rows(): the pairs given a distance are counted on the device.  h_evals_: the counter's page-locked copy - the
  // call's dist_evals, read by last_stats once the call's last event has passed (evals_pending_), so that a call with device results stays
  // asynchronous
  bool evals_pending_ = false;
  int32_t clear_device_evals(unsigned long long* d_evals);           // in front of the kernels that count
  int32_t publish_device_evals(const unsigned long long* d_evals);   // behind them, in front of the call's last event
  // set_groups(): label[n] | key_of_label[G], valid for the table of (grp_version_, grp_rows_).  search_groups(): a page of keys [nq][P]; the
  // result keys [nq][k]; [lo | compacted lo | counts | status | query numbers]; the compacted queries; the scan's table and its merged lists.
  // h_grp_: the word the compaction leaves the host
  DevBuf grp_label_, grp_keys_, grp_page_, grp_res_, grp_state_, grp_q_, grp_table_, grp_run_;
  HostBuf h_grp_;
  int64_t grp_n_groups_ = 0, grp_largest_ = 0, grp_rows_ = -1, grp_version_ = -1, grp_last_scan_queries_ = 0;
  int32_t grp_last_engines_ = 0;
  // search_group_rows(): the rows by group - offsets[G + 1], rows[n] - built at the first call after a set_groups (grp_by_group_) and released with
  // the labels; [pair counter | sizes | work-item prefix] of a pass; the pairs' merged lists
  DevBuf grp_offsets_, grp_rowlist_, grp_work_, grp_rows_run_;
  bool grp_by_group_ = false;
  // search_multi(): [pair counter | bag offsets | table elements and pairs in front of every bag | candidate offsets | a host list's keys]; the
  // candidates' labels; the gather's work-item prefix.  Its tables, partial and merged lists are the scan's (grp_table_, partial_buf_, grp_run_)
  DevBuf multi_in_, multi_label_, multi_prefix_;
  int32_t ensure_rows_by_group(const char* who);
  int32_t groups_ready(const char* who);
  void forget_rows_by_group();
  int32_t groups_representatives(const char* who, const float* dq, int64_t nq, int32_t k, const eps_search_params& p, int32_t engine, int32_t page_rows,
                                 int64_t scratch_bytes);
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
  // main-kernel event pairs of the last KRING search calls (read back after a run without a sync inside it);
  // evk0_/evk1_ alias the pair of the call in progress
  static constexpr int KRING = 64;
  hipEvent_t kring_[KRING][2] = {};
  bool kring_valid_[KRING] = {};
  int64_t kring_seq_ = 0;
  hipEvent_t evk0_ = nullptr, evk1_ = nullptr;
  // event pairs around EVERY filter-stage launch of the call in progress (eps_search_stats::filter_ms_all: the dominant kernel runs
  // once per stage, the ring above times the largest launch only)
  static constexpr int STAGE_EV = 32;
  hipEvent_t stage_ev_[STAGE_EV][2] = {};
  int stage_n_ = 0;
  int kernel_times(double* ms_out, int cap) override;
  int64_t deleted_bytes_ = 0;   // length of the bitset behind d_deleted_
  int64_t fcol_rows_ = 0;       // rows the attribute column behind d_fcol_ covers

  eps_search_stats stats_{};
  void set_main_kernel(int64_t launches, int64_t rows, int64_t queries, int32_t bits) {   // the launch a call reports as its main kernel
    stats_.main_kernel_launches = launches;
    stats_.main_kernel_rows = rows;
    stats_.main_kernel_queries = queries;
    stats_.main_kernel_bits = bits;
  }
  // what search() publishes to the matrix engine for the length of one call (cleared by `call_ = {}` on every way out of it)
  struct CallCtx {
    // what the engine launches right before its final host sync (the result conversion), so that the device works through the round trip;
    // only called when the batch is one slice
    std::function<void()> pre_sync;
    int64_t nq = -1;   // queries of the call that set it (a batch run in slices converts after the last slice instead)
    // ... and where that conversion writes: the matrix engine's last re-rank does it itself (RerankArgs::fin_*) instead of a launch
    int64_t* fin_ids = nullptr;
    float* fin_dist = nullptr;
    int32_t* fin_cnt = nullptr;
  } call_;
  // the conversion has run on the CURRENT contents of the result keys (an engine that rewrites them clears it).  Not part of call_: search()
  // reads it after the engine has returned and call_ is cleared
  bool result_finalized_ = false;

 private:
  int32_t flat_stream(const float* dq, int64_t nq, int k, int64_t row_begin, int64_t row_end, u64* run_keys, int metric = -1, bool filtered = true);
  int32_t flat_stream_page(const float* dq, int64_t nq, int k, int64_t row_begin, int64_t row_end, u64* run_keys, int metric, bool filtered,
                           const u64* lo, int64_t lo_stride);
  // ---- the steps the serving calls share (index_calls.cpp)
  // the flat engine a call of (nq, k) takes for eps_search_params::flat_engine: the matrix engine (MFMA and MFMA_I8 as asked, AUTO where
  // flat_mfma_profitable) or the stream engine, and the matrix engine's operand width (0: the library's choice).  counts_towards_mirror: an AUTO
  // call with few queries counts towards building the 8-bit mirror - a search's business only.  known false: no such engine
  struct FlatChoice {
    bool known, matrix;
    int bits;
  };
  FlatChoice resolve_flat_engine(int flat_engine, int64_t nq, int k, bool counts_towards_mirror);
  // refuses a deleted bitset / filter column / filter program's rows that an append has left shorter than the table
  int32_t check_filters_cover_table(const char* who);
  // a call that reports statistics and takes a slot of the kernel ring (select takes neither: it leaves no trace)
  void begin_timed_call();
  void end_timed_call();   // the slot counts only when a main kernel ran
  // a caller's host array onto the device, on the stream.  The array has been read when the CALL returns (the header's rule): a copy out of
  // page-locked memory is truly asynchronous, so where the call does not end in a stream sync of its own (call_syncs false: device results) the
  // stream is synchronised here.  Pageable memory is staged by the runtime before hipMemcpyAsync returns.
  int32_t copy_host_in(void* dst, const void* src, size_t bytes, bool call_syncs);
  // *dq = queries where they are on the device already, else their upload in q_buf_ (call_syncs: see copy_host_in)
  int32_t stage_queries(const char* who, const float* queries, int64_t nq, const float** dq, bool call_syncs);
  // a host call's result block to the caller's arrays (the parts asked for), and the stream sync that ends the call
  int32_t fetch_to_host(const ResultBlock& rb);
  friend int32_t quant8_view(Index&, Quant8View*);
  friend void quant8_queries(Index&, const Quant8View&, const float*, int64_t, signed char*, float*);
  friend int32_t one_pass_probe(Index&, const float*, int64_t, int, eps_one_pass_form*, u32*, u64*, int32_t*, float*, int32_t*, int32_t*);
  friend int32_t flat_mfma_search(Index&, const float*, int64_t, int, u64*, bool, int);
  friend int32_t flat_mfma_search_slice(Index&, const float*, int64_t, int, u64*, bool, int, int, bool);
  friend struct BuildCtx;   // the stages of graph_build (graph_build.hip)
  friend int32_t select_edges(Index&, const int64_t*, int64_t, const int64_t*, int32_t, int32_t, int32_t, int64_t*, int32_t*);
  friend int32_t inter_insert(Index&, const int64_t*, const int32_t*, int64_t, int32_t, int64_t*, int32_t*);
  friend int32_t graph_search(Index&, const float*, int64_t, int, const eps_search_params&, u64*, int64_t*, int);
  friend int32_t graph_search_impl(Index&, const float*, int64_t, int, const eps_search_params&, u64*, int64_t*, int, int64_t);
};

// A sparse-vector field behind eps_sparse_index_* (sparse_index.cpp; kernels: sparse.hip): a CSR table in HBM, a deleted bitset, an id map, and
// the exact scan.  A handle type of its own: nothing of a dense index applies to it.
class SparseIndex {
 public:
  SparseIndex(int64_t dim, int metric, int device) : device_(device), dim_(dim), metric_(metric) {}
  ~SparseIndex();
  int32_t init();
  int32_t set_stream(void* s);
  int32_t synchronize();
  int32_t attach_csr(const int64_t* offsets, const int32_t* indices, const float* values, int64_t n);
  int64_t row_count() const { return t_.n; }
  int32_t set_id_map(int64_t base, int64_t stride);
  int32_t set_deleted(const uint8_t* bits, int64_t nbytes);
  int32_t search(const int64_t* q_offsets, const int32_t* q_indices, const float* q_values, int64_t nq, int32_t k, int64_t* ids_out, float* dist_out,
                 int32_t* counts_out);
  int32_t last_stats(eps_search_stats* out);
  // the inverted lists of the attached table (sparse_inverted.hip): while they exist a DOT_PRODUCT / COSINE search sums term at a time on them
  int32_t build_inverted();
  int32_t drop_inverted();
  int32_t inverted_info(int64_t* columns, int64_t* postings, int64_t* longest_column, int32_t* last_engine) const;
  int32_t get_inverted(int64_t* col_offsets, int32_t* rows, float* values);
  const char* last_error() const { return err_.c_str(); }
  int32_t fail(int32_t code, const std::string& msg) {
    err_ = msg;
    return code;
  }
  int32_t hip_fail(hipError_t e, const char* what);
  int device_;

 private:
  struct Inverted {   // the table by column, owned by the handle also where the CSR is borrowed
    DevBuf col_offsets, postings;
    bool built = false;
    int64_t nnz = 0, longest = 0;
    void release() {
      col_offsets.release();
      postings.release();
      built = false;
      nnz = longest = 0;
    }
  };
  struct Table {   // a validated table: the three arrays (owned copies of host arrays, or the caller's device arrays) and the rows' sums of squares
    DevBuf off_buf, idx_buf, val_buf, norms;
    const int64_t* offsets = nullptr;
    const int32_t* indices = nullptr;
    const float* values = nullptr;
    int64_t n = 0, nnz = 0, longest = 0;
    void swap(Table& o);
  };
  // one validation launch over device-resident arrays and the read of its verdict (a stream sync)
  int32_t validate(const char* who, const char* what, const int64_t* d_off, const int32_t* d_idx, const float* d_val, int64_t n, int64_t nnz, float* norms,
                   int64_t* longest);
  int64_t dim_;
  int metric_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  Table t_;
  Inverted inv_;
  int32_t last_engine_ = 0;   // 0 none yet, 1 scan, 2 inverted lists
  int64_t id_base_ = 0, id_stride_ = 1;
  const uint8_t* d_deleted_ = nullptr;
  DevBuf deleted_buf_, verdict_buf_, q_buf_, partial_buf_, run_buf_, out_buf_;
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr, evk0_ = nullptr, evk1_ = nullptr;
  eps_search_stats stats_{};
  std::string err_;
};

// engines implemented in their own translation units
// approx = true: no exact re-rank, the top-k is selected on the fp16 keys (kNN-graph construction), filters ignored
// bits: operand width of the filter pass - 8 (int8 mirror; falls back to 16 where the table does not fit an 8-bit grid or the
// candidate lists overflow), 16 (fp16 mirror), 0 = the library's choice
int32_t flat_mfma_search(Index& ix, const float* dq, int64_t nq, int k, u64* run_keys, bool approx = false, int bits = 0);
int32_t flat_mfma_search_slice(Index& ix, const float* dq, int64_t nq, int k, u64* run_keys, bool approx, int cap_scale = 1, int bits = 16,
                               bool auto_bits = false);  // <= 2048 queries
// AUTO heuristic.  count_call: a single-query call on a table without a mirror counts towards building one (Index::small_calls_)
bool flat_mfma_profitable(Index& ix, int64_t nq, int k, bool count_call);
// stage-level entries of the flat matrix engine (eps_index_mirror_view / eps_index_filter_pass): host arrays, no side effects a search could see
int32_t flat_mirror_view(Index& ix, int bits, const float* queries, int64_t nq, eps_mirror_view* v);
int32_t flat_filter_pass(Index& ix, const float* queries, int64_t nq, int bits, int64_t lo, int64_t hi, int64_t cap, int mode, int thr_form, const void* thr,
                         void* T_out, u32* cnt_out, void* cand_out);
// the one-pass search up to and including its pass, and what that pass left behind (eps_index_one_pass_probe; one_pass.hip)
int32_t one_pass_probe(Index& ix, const float* queries, int64_t nq, int k, eps_one_pass_form* form, u32* raw_cnt, u64* raw, int32_t* table, float* qstat,
                       int32_t* kth, int32_t* T_final);
// the matrix form of a radius search (Index::search_range): one filter launch per slice of queries with thresholds from L.radius, then the exact
// tail into the survivor lists L; *cand_total += rows given an exact distance.  *served = false: no usable mirror - nothing was launched
int32_t flat_range_lists(Index& ix, const float* dq, int64_t nq, int bits, const RangeLists& L, unsigned long long* cand_total, bool* served);
int32_t quant8_view(Index& ix, Quant8View* v);
void quant8_queries(Index& ix, const Quant8View& v, const float* dq, int64_t nq, signed char* q8, float* qstat);
void half_mirror_free(HalfMirror* m);
int32_t graph_upload(Index& ix);
void graph_free(GraphDev* g);
// writes result keys [nq][k] and counts
int32_t graph_search(Index& ix, const float* dq, int64_t nq, int k, const eps_search_params& p, u64* run_keys,
                     int64_t* evals, int walk_limit = 0);
int32_t graph_search_impl(Index& ix, const float* dq, int64_t nq, int k, const eps_search_params& p, u64* run_keys, int64_t* evals, int walk_limit,
                          int64_t ecap_min);   // (ecap_min: slots of the filtered traversal's evaluation log, grown on overflow)
// stage-level entry of the build (eps_index_knn_graph / eps_index_link): run a prefix of the stages, on caller-supplied inputs
struct BuildStage {
  const int64_t* knn_in = nullptr;   // [n][K] kNN graph to link (-1 padded) instead of computing one
  int64_t nav_in = -1;               // navigation node to use (-1: the closest row to the centroid)
  int stop_after = 0;                // 1: after the kNN graph (out_ids [n][K]); 2: after Link (out_ids [n][R], out_deg [n]); 0: whole build
  int64_t* out_ids = nullptr;
  int32_t* out_deg = nullptr;
  int64_t* nav_out = nullptr;
};
int32_t graph_build(Index& ix, int64_t n, const eps_build_params& p, const BuildStage* stage = nullptr);
int32_t select_edges(Index& ix, const int64_t* nodes, int64_t m, const int64_t* cands, int32_t cpn, int32_t depth, int32_t R, int64_t* out_ids,
                     int32_t* out_deg);
int32_t inter_insert(Index& ix, const int64_t* ids, const int32_t* deg, int64_t n, int32_t R, int64_t* out_ids, int32_t* out_deg);

bool is_device_ptr(const void* p);
bool is_page_locked_ptr(const void* p);   // host memory of hipHostMalloc / hipHostRegister (torch: pin_memory)

inline eps_build_params build_params_or_default(const eps_build_params* p) {
  eps_build_params bp;
  if (p) bp = *p; else eps_default_build_params(&bp);
  return bp;
}
inline eps_search_params search_params_or_default(const eps_search_params* p) {
  eps_search_params sp;
  if (p) sp = *p; else eps_default_search_params(&sp);
  return sp;
}
inline bool flat_engine_known(int flat_engine) { return flat_engine >= EPS_FLAT_AUTO && flat_engine <= EPS_FLAT_MFMA_I8; }

// for member functions of Index that return a status
#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t e__ = (expr);                           \
    if (e__ != hipSuccess) return hip_fail(e__, #expr); \
  } while (0)

// hash-sharded table over several devices of one process (shard_group.cpp)
IndexBase* make_shard_group(int64_t dim, int metric, const int32_t* devices, int32_t shards, std::string* err);

}  // namespace eps
