// The serving calls of Index (see index.hpp): flat_stream, search, select, search_range, search_among, search_groups, search_group_rows, search_multi, search_diverse, the steps they share (their results: result_block.hpp), and the read-out of their statistics.
#include "index.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace eps {

// ------------------------------------------------------------------------------------------------ the exact stream engine
int32_t Index::flat_stream(const float* dq, int64_t nq, int k, int64_t row_begin, int64_t row_end, u64* run_keys, int metric, bool filtered) {
  if (k <= 1024) return flat_stream_page(dq, nq, k, row_begin, row_end, run_keys, metric, filtered, nullptr, 0);
  // More than 1024 results per query (the reference's BruteForceSearch has no cap: it sorts all n candidates,
  // vec_search_executor.cpp:756-767): pages of 1024 - page p is the scan's 1024 best keys ordered AFTER the last key of page
  // p-1 ((dist, id) keys are unique per row, so the pages are disjoint and their concatenation is the sorted answer).
  if (!page_buf_.reserve((size_t)nq * 1024 * sizeof(u64))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (result page)");
  for (int done = 0; done < k; done += 1024) {
    const int kc = std::min(1024, k - done);
    const int32_t rc = flat_stream_page(dq, nq, kc, row_begin, row_end, page_buf_.as<u64>(), metric, filtered, done ? run_keys + (done - 1) : nullptr, k);
    if (rc != EPS_OK) return rc;
    HIP_TRY(hipMemcpy2DAsync(run_keys + done, (size_t)k * sizeof(u64), page_buf_.p, (size_t)kc * sizeof(u64), (size_t)kc * sizeof(u64), (size_t)nq,
                             hipMemcpyDeviceToDevice, stream_));
  }
  return EPS_OK;
}

int32_t Index::flat_stream_page(const float* dq, int64_t nq, int k, int64_t row_begin, int64_t row_end, u64* run_keys, int metric, bool filtered,
                                const u64* lo, int64_t lo_stride) {
  if (row_end <= row_begin) {
    launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
    return EPS_OK;
  }
  const int W = flat_scan_waves(row_end - row_begin, nq, (int)dim_);
  if (!partial_buf_.reserve((size_t)nq * W * k * sizeof(u64))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (partial lists)");
  FlatScanArgs a;
  a.rows = d_rows_;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.dim = (int)dim_;
  a.metric = metric < 0 ? metric_ : metric;
  a.queries = dq;
  a.nq = nq;
  a.k = k;
  a.f = filter_spec();
  if (!filtered) a.f = no_filter();
  a.partial = partial_buf_.as<u64>();
  a.W = W;
  a.thr_in = nullptr;
  a.lo_in = lo;
  a.lo_stride = lo_stride;
  HIP_TRY(hipEventRecord(evk0_, stream_));
  launch_flat_scan(a, stream_);
  HIP_TRY(hipEventRecord(evk1_, stream_));
  launch_merge_lists(a.partial, W * k, k, nq, run_keys, false, stream_);
  HIP_TRY(hipGetLastError());
  stats_.main_kernel_launches += 1;
  stats_.main_kernel_rows = row_end - row_begin;
  stats_.main_kernel_queries = nq;
  stats_.main_kernel_bits = 32;
  stats_.dist_evals += nq * (row_end - row_begin);
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ the steps the calls share
int32_t Index::check_filters_cover_table(const char* who) {
  if (d_deleted_ && deleted_bytes_ < (n_rows_ + 7) / 8)
    return fail(EPS_USER_ERROR, std::string(who) + ": the deleted bitset is shorter than the table (rows were appended): call set_deleted again");
  if (f_op_ && d_fcol_ && fcol_rows_ < n_rows_)
    return fail(EPS_USER_ERROR, std::string(who) + ": the filter column is shorter than the table (rows were appended): call set_int_filter again");
  if (prog_len_ > 0 && prog_rows_n_ < n_rows_)
    return fail(EPS_USER_ERROR, std::string(who) + ": the filter program's attribute rows are shorter than the table (rows were appended): call set_filter_program again");
  return EPS_OK;
}

void Index::begin_timed_call() {
  std::memset(&stats_, 0, sizeof(stats_));
  stage_n_ = 0;
  evals_pending_ = false;
  kring_seq_ += 1;
  const int slot = (int)(kring_seq_ % KRING);
  evk0_ = kring_[slot][0];
  evk1_ = kring_[slot][1];
  kring_valid_[slot] = false;
}
void Index::end_timed_call() { kring_valid_[kring_seq_ % KRING] = stats_.main_kernel_launches > 0; }

int32_t Index::copy_host_in(void* dst, const void* src, size_t bytes, bool call_syncs) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_));
  if (!call_syncs && is_page_locked_ptr(src)) HIP_TRY(hipStreamSynchronize(stream_));   // the host array may change right after the call returns
  return EPS_OK;
}

int32_t Index::stage_queries(const char* who, const float* queries, int64_t nq, const float** dq, bool call_syncs) {
  *dq = queries;
  if (is_device_ptr(queries)) return EPS_OK;
  const size_t qb = (size_t)nq * dim_ * sizeof(float);
  if (!q_buf_.reserve(qb)) return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of device memory (queries)");
  const bool staging = !(tune_int("EPS_HOST_STAGING", 1) == 0);   // (A/B switch)
  if (staging && qb <= ((size_t)256 << 10) && h_q_.reserve(qb)) {   // (a few vectors: -30 us per call; a 3 MB batch: the runtime's pageable path measured faster than memcpy + DMA)
    // (the previous call's copy out of h_q_ has completed: every call with host queries ends in a stream sync or its results are device-side and
    // the caller orders the stream; a second call on the same index may not start before the first returns - one mutex per index)
    HIP_TRY(hipStreamSynchronize(stream_));
    memcpy(h_q_.p, queries, qb);
    HIP_TRY(hipMemcpyAsync(q_buf_.p, h_q_.p, qb, hipMemcpyHostToDevice, stream_));
  } else {
    const int32_t rc = copy_host_in(q_buf_.p, queries, qb, call_syncs);
    if (rc != EPS_OK) return rc;
  }
  *dq = q_buf_.as<float>();
  return EPS_OK;
}

int32_t Index::fetch_to_host(const ResultBlock& rb) {
  if (!(tune_int("EPS_HOST_STAGING", 1) == 0) && h_out_.reserve(rb.bytes())) {   // one copy into page-locked memory, split on the host
    HIP_TRY(hipMemcpyAsync(h_out_.p, rb.block(), rb.bytes(), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    rb.split(h_out_.p);
  } else {   // (no page-locked memory to be had: the pageable copies)
    for (int i = 0; i < rb.size(); ++i) {
      const ResultBlock::Part& part = rb.part(i);
      if (part.dst) HIP_TRY(hipMemcpyAsync(part.dst, static_cast<const char*>(rb.block()) + part.off, part.bytes, hipMemcpyDeviceToHost, stream_));
    }
    HIP_TRY(hipStreamSynchronize(stream_));
  }
  return EPS_OK;
}

Index::FlatChoice Index::resolve_flat_engine(int flat_engine, int64_t nq, int k, bool counts_towards_mirror) {
  if (!flat_engine_known(flat_engine)) return FlatChoice{false, false, 0};
  const int bits = flat_engine == EPS_FLAT_MFMA ? 16 : (flat_engine == EPS_FLAT_MFMA_I8 ? 8 : 0);   // AUTO: the library picks the operand width too
  const bool matrix = flat_engine == EPS_FLAT_AUTO ? flat_mfma_profitable(*this, nq, k, counts_towards_mirror) : flat_engine != EPS_FLAT_STREAM;
  return FlatChoice{true, matrix, bits};
}

int32_t Index::clear_device_evals(unsigned long long* d_evals) {
  HIP_TRY(hipMemsetAsync(d_evals, 0, 8, stream_));
  return EPS_OK;
}
int32_t Index::publish_device_evals(const unsigned long long* d_evals) {
  HIP_TRY(hipMemcpyAsync(h_evals_.p, d_evals, 8, hipMemcpyDeviceToHost, stream_));
  evals_pending_ = true;
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ search
int32_t Index::search(const float* queries, int64_t nq, int32_t k, const eps_search_params* pp, int64_t* ids,
                      float* dist, int32_t* counts, int32_t walk_limit) {
  const eps_search_params p = search_params_or_default(pp);
  prefilter_call_ = p.prefilter != 0;
  if (nq < 0 || k <= 0) return fail(EPS_USER_ERROR, "search: nq must be >= 0 and k > 0");
  if (nq == 0) return EPS_OK;
  if (!queries || !ids || !dist) return fail(EPS_USER_ERROR, "search: null buffer");
  if (k > (1 << 20)) return fail(EPS_DB_UNSUPPORTED_ERROR, "search: k > 1048576 is not supported");
  if (p.master_queue <= 0 || p.local_queue <= 0 || p.sync_interval <= 0 || p.intra_threads <= 0)
    return fail(EPS_USER_ERROR, "search: queue sizes, sync interval and thread count must be positive");
  HIP_TRY(hipSetDevice(device_));
  begin_timed_call();
  int32_t rc = check_filters_cover_table("search");
  if (rc != EPS_OK) return rc;

  ResultBlock rb;
  const auto r_ids = rb.add(ids, (size_t)nq * k);
  const auto r_dist = rb.add(dist, (size_t)nq * k);
  const auto r_cnt = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr)) return fail(EPS_USER_ERROR, "search: ids_out, dist_out and counts_out must all be host or all be device pointers");
  const bool out_dev = rb.device();

  const float* dq;
  rc = stage_queries("search", queries, nq, &dq, !out_dev);   // (host results: fetch_to_host ends the call in a sync)
  if (rc != EPS_OK) return rc;

  // mode selection of VecSearchExecutor::Search (vec_search_executor.cpp:855-935)
  int mode = p.mode;
  bool cap_local = false;
  if (mode == EPS_MODE_REFERENCE) {
    if (p.prefilter) {
      mode = EPS_MODE_FLAT;
    } else if (n_indexed_ < 512) {  // BruteforceThreshold, vec_search_executor.hpp:28
      mode = EPS_MODE_FLAT;
      cap_local = walk_limit == 0;  // result_size = min(size, limit, L_local_)  (:864); a candidate walk is cut by its caller
    } else {
      mode = EPS_MODE_GRAPH;
    }
  }
  if (mode == EPS_MODE_GRAPH && n_indexed_ <= 0) return fail(EPS_USER_ERROR, "search: graph mode requested but no graph is set");

  if (!run_buf_.reserve((size_t)nq * k * sizeof(u64))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (results)");
  u64* run_keys = run_buf_.as<u64>();
  HIP_TRY(hipEventRecord(ev0_, stream_));

  // results out (decided before the engines run: the matrix engine launches the result conversion itself, in front of its final
  // host sync, so that the device does not idle through that round trip)
  if (!rb.place(out_block_)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (outputs)");
  int64_t* const d_ids = rb.dev(r_ids);
  float* const d_dist = rb.dev(r_dist);
  int32_t* const d_cnt = rb.dev(r_cnt);
  result_finalized_ = false;
  auto finalize = [&]() {
    launch_finalize(run_keys, nq, k, id_base_, id_stride_, d_ids, d_dist, d_cnt, stream_);
    (void)hipEventRecord(ev1_, stream_);
    result_finalized_ = true;
  };

  int keff = k;
  if (mode == EPS_MODE_FLAT) {
    if (cap_local && p.local_queue < keff) keff = (int)p.local_queue;
    if (keff < k) launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
    const FlatChoice fc = resolve_flat_engine(p.flat_engine, nq, keff, true);
    if (!fc.known) return fail(EPS_USER_ERROR, "search: unknown flat engine");
    bool matrix = fc.matrix;
    const int bits = fc.bits;
    // a filter on @distance needs exact distances wherever it is evaluated; the MFMA engine selects its seeds on
    // approximate keys, so such searches stay on the exact stream engine
    if (prog_len_ > 0 && prog_uses_dist_ && !prefilter_call_) matrix = false;
    if (keff > 1024) matrix = false;   // result pages (see flat_stream)
    if (keff == k) {
      if (matrix) {
        // (called by the engine in front of its final sync; again after a fall-back pass.  The callable captures locals of this
        // frame: the guard clears it on every way out, an exception from the engine included)
        struct CallGuard {
          Index& ix;
          ~CallGuard() { ix.call_ = {}; }
        } guard{*this};
        call_ = CallCtx{finalize, nq, d_ids, d_dist, d_cnt};
        rc = flat_mfma_search(*this, dq, nq, k, run_keys, false, bits);
      } else {
        rc = flat_stream(dq, nq, k, 0, n_rows_, run_keys);
      }
    } else {
      // narrower result (L_local cap): compute into a k_eff-wide list, then widen
      if (!tmp_buf_.reserve((size_t)nq * keff * sizeof(u64))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory");
      u64* narrow = tmp_buf_.as<u64>();
      rc = matrix ? flat_mfma_search(*this, dq, nq, keff, narrow, false, bits) : flat_stream(dq, nq, keff, 0, n_rows_, narrow);
      if (rc == EPS_OK)
        HIP_TRY(hipMemcpy2DAsync(run_keys, (size_t)k * sizeof(u64), narrow, (size_t)keff * sizeof(u64),
                                 (size_t)keff * sizeof(u64), (size_t)nq, hipMemcpyDeviceToDevice, stream_));
    }
    if (rc != EPS_OK) return rc;
  } else {
    int64_t evals = 0;
    rc = graph_search(*this, dq, nq, k, p, run_keys, &evals, walk_limit);
    if (rc != EPS_OK) return rc;
  }

  if (!result_finalized_) finalize();
  if (!out_dev) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  end_timed_call();
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ select
// SearchByAttribute's full-scan branch (vec_search_executor.cpp:1016-1029).  Touches nothing a search reads: no statistics, no event of the
// kernel ring, no engine state - only scratch of its own.
int32_t Index::select(int64_t skip, int64_t limit, int64_t* ids_out, int64_t* count_out, int64_t* total_out) {
  if (skip < 0 || limit < 0) return fail(EPS_USER_ERROR, "select: skip and limit must be >= 0");
  if (!count_out || (limit > 0 && n_rows_ > 0 && !ids_out)) return fail(EPS_USER_ERROR, "select: null buffer");
  HIP_TRY(hipSetDevice(device_));
  const int32_t rc = check_filters_cover_table("select");
  if (rc != EPS_OK) return rc;
  const int64_t n = n_rows_;
  // [count | total | ids]: the head a host call reads first.  (Where no id can be written - limit 0, no rows - ids_out is not looked at)
  ResultBlock rb;
  const auto r_count = rb.add(count_out, 1);
  const auto r_total = rb.add(total_out, 1);
  const auto r_ids = rb.add(limit > 0 && n > 0 ? ids_out : nullptr, (size_t)std::min(limit, n));
  if (!rb.one_kind(is_device_ptr)) return fail(EPS_USER_ERROR, "select: ids_out, count_out and total_out must all be host or all be device pointers");
  const bool out_dev = rb.device();
  if (n == 0) {   // an empty table: nothing to judge
    if (out_dev) {
      HIP_TRY(hipMemsetAsync(count_out, 0, sizeof(int64_t), stream_));
      if (total_out) HIP_TRY(hipMemsetAsync(total_out, 0, sizeof(int64_t), stream_));
    } else {
      *count_out = 0;
      if (total_out) *total_out = 0;
    }
    return EPS_OK;
  }
  SelectArgs a;
  a.f = filter_spec();
  a.f.prog_use_dist = 0;   // LogicalEvaluate(root, id): no distance (:1018)
  a.n = n;
  a.skip = std::min(skip, n);   // (no rank reaches n: the window's end cannot overflow)
  a.limit = std::min(limit, n);
  a.id_base = id_base_;
  a.id_stride = id_stride_;
  const int64_t nblocks = select_blocks(n);
  const size_t counts_bytes = ((size_t)nblocks * sizeof(u32) + 7) & ~(size_t)7;
  if (!sel_bits_.reserve((size_t)nblocks * (SEL_ROWS / 8)) || !sel_scan_.reserve(counts_bytes + (size_t)(nblocks + 1) * sizeof(int64_t)) ||
      !rb.place(out_block_))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "select: out of device memory (scratch)");
  a.bits = sel_bits_.as<u64>();
  a.counts = sel_scan_.as<u32>();
  a.offsets = reinterpret_cast<int64_t*>(sel_scan_.as<char>() + counts_bytes);
  a.ids_out = rb.dev(r_ids);
  a.count_out = rb.dev(r_count);
  a.total_out = rb.dev(r_total);
  launch_select(a, stream_);
  HIP_TRY(hipGetLastError());
  if (!out_dev) {   // count and total first (the block's first two parts: 16 bytes): only the ids of the window cross PCIe, not `limit` slots
    int64_t head[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(head, rb.block(), sizeof(head), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    if (head[0] > 0) {
      HIP_TRY(hipMemcpyAsync(ids_out, a.ids_out, (size_t)head[0] * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
      HIP_TRY(hipStreamSynchronize(stream_));
    }
    *count_out = head[0];
    if (total_out) *total_out = head[1];
  }
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ search_range
// Every visible row with exact fp32 distance <= radius[j]: the total, and the cap closest by (distance, id).  One pass finds the survivors - the
// matrix form (one launch of the lower-bound filter + the exact tail, flat_range_lists) or the stream form (range_scan_kernel) - one launch orders
// them (range.hip), one host sync reads every query's status and total (host outputs: a second one brings the results, once).  What is left to the host after it, both counted in overflow_queries:
//   RANGE_RESCAN  the filter's candidate list was too short: the query runs again on the stream form;
//   RANGE_TOPK    more survivors than cap: the cap closest come from flat_stream (k = cap), the total is already counted.
// Reports like a search (statistics, kernel ring); changes nothing a later search can observe.
int32_t Index::search_range(const float* queries, int64_t nq, const float* radius, int32_t cap, const eps_search_params* pp, int64_t* ids, float* dist,
                            int32_t* counts, int64_t* totals) {
  const eps_search_params p = search_params_or_default(pp);
  if (nq < 0) return fail(EPS_USER_ERROR, "search_range: nq must be >= 0");
  if (cap < 1 || cap > RANGE_MAX_CAP) return fail(EPS_USER_ERROR, "search_range: cap must be in [1, 8192]");
  if (nq == 0) return EPS_OK;
  if (!queries || !radius || !ids || !dist) return fail(EPS_USER_ERROR, "search_range: null buffer");
  if (!flat_engine_known(p.flat_engine)) return fail(EPS_USER_ERROR, "search_range: unknown flat engine");
  HIP_TRY(hipSetDevice(device_));
  if (is_device_ptr(radius)) return fail(EPS_USER_ERROR, "search_range: radius must be a host array");
  for (int64_t j = 0; j < nq; ++j)
    if (radius[j] != radius[j]) return fail(EPS_USER_ERROR, "search_range: a radius is NaN");
  int32_t rc = check_filters_cover_table("search_range");
  if (rc != EPS_OK) return rc;
  ResultBlock rb;
  const auto r_ids = rb.add(ids, (size_t)nq * cap);
  const auto r_totals = rb.add(totals, (size_t)nq);
  const auto r_dist = rb.add(dist, (size_t)nq * cap);
  const auto r_counts = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr))
    return fail(EPS_USER_ERROR, "search_range: ids_out, dist_out, counts_out and totals_out must all be host or all be device pointers");
  begin_timed_call();
  prefilter_call_ = false;   // (@distance reads the candidate's exact distance)
  const int64_t n = n_rows_;

  // ---- scratch.  Device: [counts | status | candidates re-ranked], [radii | fall-back query numbers]; page-locked: [radii | read-back | query numbers]
  const size_t rb_bytes = (((size_t)nq * 8 + 7) & ~(size_t)7) + 8, rad_bytes = ((size_t)nq * 4 + 7) & ~(size_t)7;
  if (!rng_keys_.reserve((size_t)nq * cap * sizeof(u64)) || !rng_cnt_.reserve(rb_bytes) || !rng_in_.reserve(2 * rad_bytes) || !rb.place(out_block_))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_range: out of device memory (scratch)");
  if (!h_rng_.reserve(2 * rad_bytes + rb_bytes)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_range: out of page-locked host memory");
  float* h_rad = static_cast<float*>(h_rng_.p);
  u32* h_rb = reinterpret_cast<u32*>(static_cast<char*>(h_rng_.p) + rad_bytes);
  int32_t* h_sel = reinterpret_cast<int32_t*>(static_cast<char*>(h_rng_.p) + rad_bytes + rb_bytes);
  u32* d_cnt = rng_cnt_.as<u32>();
  u32* d_status = d_cnt + nq;
  unsigned long long* d_cand_total = reinterpret_cast<unsigned long long*>(rng_cnt_.as<char>() + rb_bytes - 8);
  int32_t* d_sel = reinterpret_cast<int32_t*>(rng_in_.as<char>() + rad_bytes);

  const float* dq;
  rc = stage_queries("search_range", queries, nq, &dq, true);   // (the sync below)
  if (rc != EPS_OK) return rc;
  HIP_TRY(hipStreamSynchronize(stream_));   // (the previous call's copies out of / into h_rng_ have completed - and this call's copy of host queries)
  memcpy(h_rad, radius, (size_t)nq * 4);
  HIP_TRY(hipMemcpyAsync(rng_in_.p, h_rad, (size_t)nq * 4, hipMemcpyHostToDevice, stream_));
  HIP_TRY(hipMemsetAsync(rng_cnt_.p, 0, rb_bytes, stream_));
  HIP_TRY(hipEventRecord(ev0_, stream_));

  const RangeLists L{rng_keys_.as<u64>(), d_cnt, rng_in_.as<float>(), cap};
  const FilterSpec fs = filter_spec();
  // the stream form over the `m` queries named by sel (null: all of them), in launches of at most 32768 queries (the grid's y extent)
  auto scan = [&](const int32_t* sel, int64_t m) {
    for (int64_t q0 = 0; q0 < m; q0 += 32768) {
      RangeScanArgs a{d_rows_, n, (int)dim_, metric_, dq, std::min<int64_t>(32768, m - q0), sel ? sel + q0 : nullptr, fs, L};
      if (!sel) {   // (query numbers count from the launch's first query)
        a.queries = dq + q0 * dim_;
        a.L = RangeLists{L.keys + q0 * cap, L.cnt + q0, L.radius + q0, cap};
      }
      launch_range_scan(a, stream_);
    }
    stats_.dist_evals += m * n;
  };
  auto order = [&](const int32_t* sel, int64_t m, const u64* topk) {
    launch_range_order(RangeOrderArgs{m, sel, L, topk, d_status, id_base_, id_stride_, rb.dev(r_ids), rb.dev(r_dist), rb.dev(r_counts), rb.dev(r_totals)}, stream_);
  };
  auto read_back = [&]() -> hipError_t {
    const hipError_t er = hipMemcpyAsync(h_rb, rng_cnt_.p, rb_bytes, hipMemcpyDeviceToHost, stream_);   // (status and totals only: the results cross PCIe once, at the end)
    return er == hipSuccess ? hipStreamSynchronize(stream_) : er;
  };
  auto pick = [&](u32 status, std::vector<int32_t>* sel) -> hipError_t {   // the queries left in `status`, their numbers on the device
    sel->clear();
    for (int64_t j = 0; j < nq; ++j)
      if (h_rb[nq + j] == status) sel->push_back((int32_t)j);
    if (sel->empty()) return hipSuccess;
    memcpy(h_sel, sel->data(), sel->size() * 4);
    return hipMemcpyAsync(d_sel, h_sel, sel->size() * 4, hipMemcpyHostToDevice, stream_);
  };

  // ---- the pass
  const FlatChoice fc = resolve_flat_engine(p.flat_engine, nq, 1, false);   // (a filter on @distance too: the exact tail evaluates it)
  bool served = false;
  if (fc.matrix) {
    rc = flat_range_lists(*this, dq, nq, fc.bits, L, d_cand_total, &served);
    if (rc != EPS_OK) return rc;
  }
  if (!served && n > 0) {
    HIP_TRY(hipEventRecord(evk0_, stream_));
    scan(nullptr, nq);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    set_main_kernel(1, n, nq, 32);
  }
  order(nullptr, nq, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(read_back());
  stats_.rerank_rows = (int64_t)*reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(h_rb) + rb_bytes - 8);

  // ---- what the lists could not answer
  const eps_search_stats pass_stats = stats_;
  std::vector<int32_t> sel;
  int64_t fell_back = 0;
  HIP_TRY(pick(RANGE_RESCAN, &sel));
  if (!sel.empty()) {
    fell_back += (int64_t)sel.size();
    launch_range_gather(dq, (int)dim_, d_sel, (int64_t)sel.size(), nullptr, d_cnt, true, stream_);
    scan(d_sel, (int64_t)sel.size());
    order(d_sel, (int64_t)sel.size(), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(read_back());
  }
  std::vector<int32_t> rescanned;
  rescanned.swap(sel);
  HIP_TRY(pick(RANGE_TOPK, &sel));
  if (!sel.empty()) {
    const int64_t m = (int64_t)sel.size();
    fell_back += m;
    for (int32_t j : sel) fell_back -= std::binary_search(rescanned.begin(), rescanned.end(), j) ? 1 : 0;   // (a query counts once)
    if (!tmp_buf_.reserve((size_t)m * dim_ * sizeof(float)) || !run_buf_.reserve((size_t)m * cap * sizeof(u64)))
      return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_range: out of device memory (fall-back)");
    launch_range_gather(dq, (int)dim_, d_sel, m, tmp_buf_.as<float>(), d_cnt, false, stream_);
    // (flat_stream times its scan with the call's main-kernel events: it gets a spare pair - no filter stage of this call uses one - so that
    // main_kernel_ms stays the time of the pass, as the other main_kernel_* fields do)
    hipEvent_t const k0 = evk0_, k1 = evk1_;
    evk0_ = stage_ev_[STAGE_EV - 1][0];
    evk1_ = stage_ev_[STAGE_EV - 1][1];
    rc = flat_stream(tmp_buf_.as<float>(), m, cap, 0, n, run_buf_.as<u64>());
    evk0_ = k0;
    evk1_ = k1;
    if (rc != EPS_OK) return rc;
    order(d_sel, m, run_buf_.as<u64>());
    HIP_TRY(hipGetLastError());
  }
  // the call's main kernel stays the pass
  if (fell_back > 0) set_main_kernel(pass_stats.main_kernel_launches, pass_stats.main_kernel_rows, pass_stats.main_kernel_queries, pass_stats.main_kernel_bits);
  stats_.overflow_queries = fell_back;
  HIP_TRY(hipEventRecord(ev1_, stream_));
  if (!rb.device()) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  end_timed_call();
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ search_among
// The middle of search_among, and the pool of search_diverse's candidate form, after their checks and begin_timed_call: the lists to the device,
// gather, merge - query j's k smallest unique keys over the visible rows its list names in run_buf_[j][k], the call's first event (ev0_) on the
// stream, the pairs' counter cleared (*d_evals_out: the caller publishes it).  longest: as among_lists_check left it
int32_t Index::among_keys(const char* who, const float* dq, int64_t nq, const int64_t* cand_ids, const int64_t* cand_offsets, int64_t n_cand, int32_t k,
                          int64_t longest, bool call_syncs, unsigned long long** d_evals_out) {
  // ---- scratch: [pair counter | offsets | a host list's ids], partial lists, result keys
  const bool ids_dev = n_cand > 0 && is_device_ptr(cand_ids);
  const size_t off_bytes = cand_offsets ? (size_t)(nq + 1) * sizeof(int64_t) : 0, list_bytes = ids_dev ? 0 : (size_t)n_cand * sizeof(int64_t);
  const AmongPlan plan = among_plan(!cand_offsets, nq, longest, k, pick_nq(nq, k, (int)dim_));
  if (!among_in_.reserve(8 + off_bytes + list_bytes) || !partial_buf_.reserve((size_t)nq * plan.W * k * sizeof(u64)) ||
      !run_buf_.reserve((size_t)nq * k * sizeof(u64)))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of device memory (scratch)");
  if (!h_evals_.reserve(8)) return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of page-locked host memory");
  unsigned long long* d_evals = *d_evals_out = among_in_.as<unsigned long long>();
  int64_t* d_off = cand_offsets ? among_in_.as<int64_t>() + 1 : nullptr;
  const int64_t* d_list = cand_ids;
  int32_t rc = clear_device_evals(d_evals);
  if (rc != EPS_OK) return rc;
  if (cand_offsets) {
    rc = copy_host_in(d_off, cand_offsets, off_bytes, call_syncs);
    if (rc != EPS_OK) return rc;
  }
  if (!ids_dev && n_cand > 0) {
    d_list = reinterpret_cast<const int64_t*>(among_in_.as<char>() + 8 + off_bytes);
    rc = copy_host_in(const_cast<int64_t*>(d_list), cand_ids, list_bytes, call_syncs);
    if (rc != EPS_OK) return rc;
  }
  u64* run_keys = run_buf_.as<u64>();
  HIP_TRY(hipEventRecord(ev0_, stream_));

  const bool any = n_cand > 0 && n_rows_ > 0;   // (else no list entry can name a row)
  set_main_kernel(any ? 1 : 0, n_cand, nq, 32);
  if (any) {
    AmongArgs a;
    a.rows = d_rows_;
    a.n_rows = n_rows_;
    a.dim = (int)dim_;
    a.metric = metric_;
    a.queries = dq;
    a.nq = nq;
    a.k = k;
    a.f = filter_spec();
    a.ids = d_list;
    a.offsets = d_off;
    a.n_cand = n_cand;
    a.id_base = id_base_;
    a.id_stride = id_stride_;
    a.plan = plan;
    a.partial = partial_buf_.as<u64>();
    a.evals = d_evals;
    HIP_TRY(hipEventRecord(evk0_, stream_));
    launch_among_gather(a, stream_);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    launch_among_merge(a.partial, plan.W, k, nq, run_keys, stream_);
  } else {
    launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
  }
  return EPS_OK;
}

// The k closest visible rows among the ids the caller names (among.hip): gather, merge, result conversion - no host sync of its own, so a call
// with device results stays asynchronous (the pairs given a distance are counted on the device and read by last_stats).  Reports like a search
// (statistics, kernel ring); changes nothing a later search can observe.
int32_t Index::search_among(const float* queries, int64_t nq, const int64_t* cand_ids, const int64_t* cand_offsets, int64_t n_cand, int32_t k, int64_t* ids,
                            float* dist, int32_t* counts) {
  if (k < 1 || k > AMONG_MAX_K) return fail(EPS_USER_ERROR, "search_among: k must be in [1, 1024]");
  HIP_TRY(hipSetDevice(device_));
  if (cand_offsets && is_device_ptr(cand_offsets)) return fail(EPS_USER_ERROR, "search_among: cand_offsets must be a host array");
  const char* why;
  int64_t longest = 0;
  if (among_lists_check(cand_offsets, nq, n_cand, &longest, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_among: ") + why);
  if (nq == 0) return EPS_OK;
  if (!queries || !ids || !dist || (n_cand > 0 && !cand_ids)) return fail(EPS_USER_ERROR, "search_among: null buffer");
  ResultBlock rb;
  const auto r_ids = rb.add(ids, (size_t)nq * k);
  const auto r_dist = rb.add(dist, (size_t)nq * k);
  const auto r_cnt = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr)) return fail(EPS_USER_ERROR, "search_among: ids_out, dist_out and counts_out must all be host or all be device pointers");
  const bool out_dev = rb.device();
  int32_t rc = check_filters_cover_table("search_among");
  if (rc != EPS_OK) return rc;
  begin_timed_call();
  prefilter_call_ = false;   // (@distance reads the candidate's exact distance)

  const float* dq;
  rc = stage_queries("search_among", queries, nq, &dq, !out_dev);
  if (rc != EPS_OK) return rc;

  if (!rb.place(out_block_)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_among: out of device memory (scratch)");
  unsigned long long* d_evals = nullptr;
  rc = among_keys("search_among", dq, nq, cand_ids, cand_offsets, n_cand, k, longest, !out_dev, &d_evals);
  if (rc != EPS_OK) return rc;
  const u64* run_keys = run_buf_.as<u64>();
  launch_finalize(run_keys, nq, k, id_base_, id_stride_, rb.dev(r_ids), rb.dev(r_dist), rb.dev(r_cnt), stream_);
  rc = publish_device_evals(d_evals);
  if (rc != EPS_OK) return rc;
  HIP_TRY(hipEventRecord(ev1_, stream_));
  if (!out_dev) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  end_timed_call();
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ search_diverse
// k rows of every query's pool by maximal marginal relevance (diverse.hip, layout: diverse_host.hpp).  The pool - fetch_k keys per query in
// run_buf_ - is one page of the flat engine a search of (nq, fetch_k) would take, or search_among's gather and merge over the caller's lists; then
// one launch of the selection kernel and the result conversion.  No host sync of its own (the matrix engine keeps the ones a search has).  Reports
// like a search; changes nothing a later call can observe.
int32_t Index::search_diverse(const float* queries, int64_t nq, int32_t k, int32_t fetch_k, float lambda, const int64_t* cand_ids, const int64_t* cand_offsets,
                              int64_t n_cand, const eps_search_params* pp, int64_t* ids, float* dist, float* score, int32_t* counts) {
  const eps_search_params p = search_params_or_default(pp);
  const char* why;
  if (diverse_args_check(nq, k, fetch_k, lambda, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_diverse: ") + why);
  if (!flat_engine_known(p.flat_engine)) return fail(EPS_USER_ERROR, "search_diverse: unknown flat engine");
  HIP_TRY(hipSetDevice(device_));
  const bool cand = cand_ids != nullptr;
  if (!cand && (cand_offsets || n_cand != 0)) return fail(EPS_USER_ERROR, "search_diverse: null buffer");   // (a list without its ids)
  if (cand_offsets && is_device_ptr(cand_offsets)) return fail(EPS_USER_ERROR, "search_diverse: cand_offsets must be a host array");
  int64_t longest = 0;
  if (cand && among_lists_check(cand_offsets, nq, n_cand, &longest, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_diverse: ") + why);
  if (nq == 0) return EPS_OK;
  if (!queries || !ids || !dist) return fail(EPS_USER_ERROR, "search_diverse: null buffer");
  ResultBlock rb;
  const auto r_ids = rb.add(ids, (size_t)nq * k);
  const auto r_dist = rb.add(dist, (size_t)nq * k);
  const auto r_score = rb.add(score, (size_t)nq * k);
  const auto r_cnt = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr))
    return fail(EPS_USER_ERROR, "search_diverse: ids_out, dist_out, score_out and counts_out must all be host or all be device pointers");
  const bool out_dev = rb.device();
  int32_t rc = check_filters_cover_table("search_diverse");
  if (rc != EPS_OK) return rc;
  begin_timed_call();
  prefilter_call_ = false;   // (@distance reads the row's exact distance)

  const float* dq;
  rc = stage_queries("search_diverse", queries, nq, &dq, !out_dev);
  if (rc != EPS_OK) return rc;
  if (!div_sel_.reserve((size_t)nq * k * sizeof(u64)) || !rb.place(out_block_))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_diverse: out of device memory (scratch)");

  // ---- the pool: run_buf_[nq][fetch_k], ascending keys, KEY_EMPTY behind them
  unsigned long long* d_evals = nullptr;
  if (cand) {
    rc = among_keys("search_diverse", dq, nq, cand_ids, cand_offsets, n_cand, fetch_k, longest, !out_dev, &d_evals);
    if (rc != EPS_OK) return rc;
  } else {
    if (!among_in_.reserve(8) || !run_buf_.reserve((size_t)nq * fetch_k * sizeof(u64)))
      return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_diverse: out of device memory (scratch)");
    if (!h_evals_.reserve(8)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_diverse: out of page-locked host memory");
    d_evals = among_in_.as<unsigned long long>();
    rc = clear_device_evals(d_evals);
    if (rc != EPS_OK) return rc;
    HIP_TRY(hipEventRecord(ev0_, stream_));
    // the flat engine a search of (nq, fetch_k) would take; all of them carry the stream scan's bits
    const FlatChoice fc = resolve_flat_engine(p.flat_engine, nq, fetch_k, false);
    // (a filter on @distance needs exact distances where it is evaluated; an empty table: the stream page's fill)
    const bool matrix = fc.matrix && !(prog_len_ > 0 && prog_uses_dist_) && n_rows_ > 0;
    rc = matrix ? flat_mfma_search(*this, dq, nq, fetch_k, run_buf_.as<u64>(), false, fc.bits)
                : flat_stream_page(dq, nq, fetch_k, 0, n_rows_, run_buf_.as<u64>(), -1, true, nullptr, 0);
    if (rc != EPS_OK) return rc;
  }

  DiverseArgs a;
  a.rows = d_rows_;
  a.dim = (int)dim_;
  a.metric = metric_;
  a.pool = run_buf_.as<u64>();
  a.nq = nq;
  a.fetch_k = fetch_k;
  a.k = k;
  a.lam = lambda;
  a.mu = 1.0f - lambda;
  a.sel_keys = div_sel_.as<u64>();
  a.score = rb.dev(r_score);
  a.evals = d_evals;
  HIP_TRY(hipEventRecord(evk0_, stream_));
  launch_diverse_select(a, stream_);
  HIP_TRY(hipEventRecord(evk1_, stream_));
  set_main_kernel(1, fetch_k, nq, 32);
  launch_finalize(a.sel_keys, nq, k, id_base_, id_stride_, rb.dev(r_ids), rb.dev(r_dist), rb.dev(r_cnt), stream_);
  rc = publish_device_evals(d_evals);   // (the pool's and the selection's pairs: last_stats adds them)
  if (rc != EPS_OK) return rc;
  HIP_TRY(hipEventRecord(ev1_, stream_));
  if (!out_dev) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  end_timed_call();
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ set_groups, search_groups
// One int64 key per row -> dense labels (groups_relabel, on the host: a set-up step) kept on the device next to the keys they stand for.
int32_t Index::set_groups(const int64_t* keys, int64_t n) {
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));   // (a call in flight may read the labels this one replaces)
  grp_rows_ = -1;   // forgotten, also where the call fails below
  forget_rows_by_group();
  grp_n_groups_ = grp_largest_ = 0;
  if (!keys) return EPS_OK;
  if (n != n_rows_) return fail(EPS_USER_ERROR, "set_groups: n must equal the table's row count");
  std::vector<int64_t> from_device, key_of_label;
  std::vector<int32_t> label((size_t)n);
  if (n > 0 && is_device_ptr(keys)) {
    from_device.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(from_device.data(), keys, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    keys = from_device.data();
  }
  int64_t largest = 0;
  const int64_t G = groups_relabel(keys, n, label.data(), &key_of_label, &largest);
  if (n > 0) {
    if (!grp_label_.reserve((size_t)n * sizeof(int32_t)) || !grp_keys_.reserve((size_t)G * sizeof(int64_t)))
      return fail(EPS_INFRA_UNEXPECTED_ERROR, "set_groups: out of device memory");
    HIP_TRY(hipMemcpyAsync(grp_label_.p, label.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipMemcpyAsync(grp_keys_.p, key_of_label.data(), (size_t)G * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));   // (the vectors end with this call)
  }
  grp_n_groups_ = G;
  grp_largest_ = largest;
  grp_rows_ = n;
  grp_version_ = rows_version_;
  return EPS_OK;
}

int32_t Index::groups_info(int64_t* n_groups, int64_t* largest_group, int32_t* last_engines, int64_t* last_scan_queries) {
  if (n_groups) *n_groups = grp_rows_ >= 0 ? grp_n_groups_ : 0;
  if (largest_group) *largest_group = grp_rows_ >= 0 ? grp_largest_ : 0;
  if (last_engines) *last_engines = grp_last_engines_;
  if (last_scan_queries) *last_scan_queries = grp_last_scan_queries_;
  return EPS_OK;
}

// The k closest groups per query (groups.hip).  Pages: a round is a page of keys per unfinished query, groups_first_kernel over it, and one host
// sync that reads how many queries are left.  Scan: the table once per 4 queries into the (query, label) slots, c queries at a time.  AUTO:
// GROUPS_AUTO_ROUNDS rounds of pages, then the scan for the queries still unfinished, named by number as search_range's fall-backs are.
// Reports like a search (statistics, kernel ring); changes nothing a later search can observe.
int32_t Index::search_groups(const float* queries, int64_t nq, int32_t k, const eps_search_params* pp, int32_t engine, int32_t page_rows, int64_t scratch_bytes,
                             int64_t* ids, float* dist, int64_t* group_keys, int32_t* counts) {
  const eps_search_params p = search_params_or_default(pp);
  const char* why;
  if (groups_args_check(nq, k, engine, page_rows, scratch_bytes, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_groups: ") + why);
  if (!flat_engine_known(p.flat_engine)) return fail(EPS_USER_ERROR, "search_groups: unknown flat engine");
  if (nq == 0) return EPS_OK;
  HIP_TRY(hipSetDevice(device_));
  int32_t rc = groups_ready("search_groups");
  if (rc != EPS_OK) return rc;
  if (!queries || !ids || !dist || !group_keys) return fail(EPS_USER_ERROR, "search_groups: null buffer");
  ResultBlock rb;
  const auto r_ids = rb.add(ids, (size_t)nq * k);
  const auto r_gk = rb.add(group_keys, (size_t)nq * k);
  const auto r_dist = rb.add(dist, (size_t)nq * k);
  const auto r_cnt = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr))
    return fail(EPS_USER_ERROR, "search_groups: ids_out, dist_out, group_keys_out and counts_out must all be host or all be device pointers");
  const bool out_dev = rb.device();
  rc = check_filters_cover_table("search_groups");
  if (rc != EPS_OK) return rc;
  begin_timed_call();
  prefilter_call_ = false;   // (@distance reads the row's exact distance)

  const float* dq;
  rc = stage_queries("search_groups", queries, nq, &dq, !out_dev);
  if (rc != EPS_OK) return rc;
  if (!rb.place(out_block_)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_groups: out of device memory (scratch)");
  rc = groups_representatives("search_groups", dq, nq, k, p, engine, page_rows, scratch_bytes);
  if (rc != EPS_OK) return rc;
  const u64* res = grp_res_.as<u64>();
  launch_finalize(res, nq, k, id_base_, id_stride_, rb.dev(r_ids), rb.dev(r_dist), rb.dev(r_cnt), stream_);
  launch_groups_keys(res, nq, k, grp_label_.as<int32_t>(), grp_keys_.as<int64_t>(), rb.dev(r_gk), stream_);
  HIP_TRY(hipEventRecord(ev1_, stream_));
  if (!out_dev) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  end_timed_call();
  return EPS_OK;
}

// The first phase of search_groups and search_group_rows, after their checks and begin_timed_call: the engines, which leave query j's
// representatives in grp_res_[j][k] - ascending keys, KEY_EMPTY behind them - and the call's first event (ev0_) on the stream.
int32_t Index::groups_representatives(const char* who, const float* dq, int64_t nq, int32_t k, const eps_search_params& p, int32_t engine, int32_t page_rows,
                                      int64_t scratch_bytes) {
  int32_t rc;
  grp_last_engines_ = 0;
  grp_last_scan_queries_ = 0;
  // ---- scratch: result keys; [lo | compacted lo | counts | status | query numbers]; a page; the compacted queries
  const int64_t n = n_rows_, G = grp_n_groups_;
  const int P = groups_page_rows(k, page_rows);
  const bool pages = engine != EPS_GROUPS_SCAN && n > 0;
  if (!grp_res_.reserve((size_t)nq * k * sizeof(u64)) || !grp_state_.reserve((size_t)nq * 28) ||
      (pages && (!grp_page_.reserve((size_t)nq * P * sizeof(u64)) || !grp_q_.reserve((size_t)nq * dim_ * sizeof(float)))))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of device memory (scratch)");
  if (!h_grp_.reserve(8)) return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of page-locked host memory");
  u64* res = grp_res_.as<u64>();
  u64* d_lo = grp_state_.as<u64>();
  u64* d_clo = d_lo + nq;
  u32* d_rescnt = reinterpret_cast<u32*>(d_clo + nq);
  u32* d_status = d_rescnt + nq;
  int32_t* d_qsel = reinterpret_cast<int32_t*>(d_status + nq);
  u32* h_left = static_cast<u32*>(h_grp_.p);
  const int32_t* label = grp_label_.as<int32_t>();
  launch_fill_u64(res, nq * k, KEY_EMPTY, stream_);
  HIP_TRY(hipMemsetAsync(d_rescnt, 0, (size_t)nq * 8, stream_));   // (counts and status)
  HIP_TRY(hipEventRecord(ev0_, stream_));

  int64_t left = n > 0 ? nq : 0;   // queries without their answer yet; after a round of pages d_qsel names them
  bool named = false;
  if (pages) {
    u64* page = grp_page_.as<u64>();
    for (int round = 0; left > 0 && (engine == EPS_GROUPS_PAGES || round < GROUPS_AUTO_ROUNDS); ++round) {
      if (round == 0) {   // the flat engine a search of (nq, P) would take; all of them carry the stream scan's bits
        const FlatChoice fc = resolve_flat_engine(p.flat_engine, nq, P, false);   // (known: the callers have refused any other)
        const bool matrix = fc.matrix && !(prog_len_ > 0 && prog_uses_dist_);   // (a filter on @distance needs exact distances where it is evaluated)
        rc = matrix ? flat_mfma_search(*this, dq, nq, P, page, false, fc.bits) : flat_stream_page(dq, nq, P, 0, n, page, -1, true, nullptr, 0);
      } else {
        launch_groups_gather(dq, (int)dim_, d_lo, d_qsel, left, grp_q_.as<float>(), d_clo, stream_);
        rc = flat_stream_page(grp_q_.as<float>(), left, P, 0, n, page, -1, true, d_clo, 1);
      }
      if (rc != EPS_OK) return rc;
      launch_groups_first(GroupsFirstArgs{page, P, left, named ? d_qsel : nullptr, label, k, res, d_rescnt, d_status, d_lo}, stream_);
      launch_groups_compact(d_status, nq, d_qsel, h_left, stream_);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(stream_));   // the round's one sync
      left = (int64_t)*h_left;
      named = true;
    }
    grp_last_engines_ |= 1 << EPS_GROUPS_PAGES;
  }
  if (left > 0 && engine != EPS_GROUPS_PAGES) {
    const GroupsScanPlan plan = groups_scan_plan(left, G, k, scratch_bytes);
    if (!grp_table_.reserve((size_t)groups_table_bytes(plan, G)) || !partial_buf_.reserve((size_t)plan.c * plan.W * k * sizeof(u64)) ||
        !grp_run_.reserve((size_t)plan.c * k * sizeof(u64)))
      return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of device memory (the scan's table)");
    u64* best = grp_table_.as<u64>();
    const FilterSpec fs = filter_spec();
    for (int64_t i0 = 0; i0 < left; i0 += plan.c) {
      const int64_t mc = std::min(plan.c, left - i0);
      launch_fill_u64(best, mc * G, KEY_EMPTY, stream_);
      GroupsScanArgs a;
      a.rows = d_rows_;
      a.n = n;
      a.dim = (int)dim_;
      a.metric = metric_;
      a.queries = named ? dq : dq + i0 * dim_;   // (unnamed: query numbers count from the chunk's first)
      a.m = mc;
      a.qsel = named ? d_qsel + i0 : nullptr;
      a.f = fs;
      a.label = label;
      a.best = best;
      a.G = G;
      a.W = flat_scan_waves(n, mc, (int)dim_);
      HIP_TRY(hipEventRecord(evk0_, stream_));
      launch_groups_min_scan(a, stream_);
      HIP_TRY(hipEventRecord(evk1_, stream_));
      launch_groups_table_topk(best, G, mc, k, plan, partial_buf_.as<u64>(), stream_);
      launch_among_merge(partial_buf_.as<u64>(), plan.W, k, mc, grp_run_.as<u64>(), stream_);
      launch_groups_scatter(grp_run_.as<u64>(), k, a.qsel, mc, named ? res : res + i0 * k, stream_);
      set_main_kernel(1, n, mc, 32);   // (the last chunk's)
    }
    stats_.dist_evals += left * n;
    grp_last_engines_ |= 1 << EPS_GROUPS_SCAN;
    grp_last_scan_queries_ = left;
  }
  return EPS_OK;
}

// no groups set / labels of another table: the refusals search_groups and search_group_rows share.  Stale labels take the rows by group with them
int32_t Index::groups_ready(const char* who) {
  if (grp_rows_ < 0) return fail(EPS_USER_ERROR, std::string(who) + ": no groups are set: call set_groups first");
  if (grp_version_ != rows_version_ || grp_rows_ != n_rows_) {
    forget_rows_by_group();
    return fail(EPS_USER_ERROR, std::string(who) + ": the group labels are stale (rows were attached or appended): call set_groups again");
  }
  return EPS_OK;
}

void Index::forget_rows_by_group() {
  if (!grp_by_group_ && !grp_offsets_.p && !grp_rowlist_.p) return;
  (void)hipStreamSynchronize(stream_);   // (a call in flight may read them)
  grp_offsets_.release();
  grp_rowlist_.release();
  grp_by_group_ = false;
}

// The rows by group (offsets[G + 1], rows[n]; group_rows.hip) for the calls that walk a group's rows: built at the first such call after a
// set_groups - histogram, scan, scatter, one stream sync - and kept until the labels go
int32_t Index::ensure_rows_by_group(const char* who) {
  const int64_t n = n_rows_, G = grp_n_groups_;
  if (grp_by_group_ || n <= 0) return EPS_OK;
  DevBuf cursor;
  if (!grp_offsets_.reserve((size_t)(G + 1) * sizeof(int64_t)) || !grp_rowlist_.reserve((size_t)n * sizeof(int32_t)) || !cursor.reserve((size_t)G * sizeof(u32))) {
    forget_rows_by_group();
    return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + ": out of device memory (the rows by group)");
  }
  HIP_TRY(hipMemsetAsync(cursor.p, 0, (size_t)G * sizeof(u32), stream_));
  launch_group_rows_build(grp_label_.as<int32_t>(), n, G, cursor.as<u32>(), grp_offsets_.as<int64_t>(), grp_rowlist_.as<int32_t>(), stream_);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream_));   // (the cursors end here)
  grp_by_group_ = true;
  return EPS_OK;
}

// The k closest groups per query and the m closest visible rows of each (group_rows.hip, plan: group_rows_host.hpp).  Phase 1 is search_groups'
// (groups_representatives); phase 2 - work list, gather, merge, result conversion - reads what phase 1 left on the device and has no host sync of
// its own, so with EPS_GROUPS_SCAN and device results the call stays asynchronous.  The rows by group (offsets[G + 1], rows[n]) are built on the
// device at the first call after a set_groups.  Reports like a search; changes nothing a later call can observe.
int32_t Index::search_group_rows(const float* queries, int64_t nq, int32_t k, int32_t m, const eps_search_params* pp, int32_t engine, int32_t page_rows,
                                 int64_t scratch_bytes, int64_t* ids, float* dist, int64_t* group_keys, int32_t* row_counts, int64_t* group_sizes,
                                 int32_t* counts) {
  const eps_search_params p = search_params_or_default(pp);
  const char* why;
  if (group_rows_args_check(nq, k, m, engine, page_rows, scratch_bytes, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_group_rows: ") + why);
  if (!flat_engine_known(p.flat_engine)) return fail(EPS_USER_ERROR, "search_group_rows: unknown flat engine");
  if (nq == 0) return EPS_OK;
  HIP_TRY(hipSetDevice(device_));
  int32_t rc = groups_ready("search_group_rows");
  if (rc != EPS_OK) return rc;
  if (!queries || !ids || !dist || !group_keys || !row_counts) return fail(EPS_USER_ERROR, "search_group_rows: null buffer");
  const size_t km = (size_t)k * m;
  ResultBlock rb;
  const auto r_ids = rb.add(ids, (size_t)nq * km);
  const auto r_gk = rb.add(group_keys, (size_t)nq * k);
  const auto r_gs = rb.add(group_sizes, (size_t)nq * k);
  const auto r_dist = rb.add(dist, (size_t)nq * km);
  const auto r_rc = rb.add(row_counts, (size_t)nq * k);
  const auto r_cnt = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr)) return fail(EPS_USER_ERROR, "search_group_rows: the output buffers must all be host or all be device pointers");
  const bool out_dev = rb.device();
  rc = check_filters_cover_table("search_group_rows");
  if (rc != EPS_OK) return rc;

  const int64_t n = n_rows_;
  rc = ensure_rows_by_group("search_group_rows");
  if (rc != EPS_OK) return rc;
  begin_timed_call();
  prefilter_call_ = false;   // (@distance reads the row's exact distance)

  const float* dq;
  rc = stage_queries("search_group_rows", queries, nq, &dq, !out_dev);
  if (rc != EPS_OK) return rc;

  // ---- scratch: [pair counter | sizes | prefix] of a pass, its partial lists and merged lists; host results' device block
  const GroupRowsPlan plan = group_rows_plan(nq, k, m, n > 0 ? n : 1, grp_largest_ > 0 ? grp_largest_ : 1);
  const int64_t pass_pairs = plan.slice * k;
  if (!grp_work_.reserve(8 + (size_t)(2 * pass_pairs + 1) * sizeof(u32)) || !partial_buf_.reserve((size_t)plan.items * m * sizeof(u64)) ||
      !grp_rows_run_.reserve((size_t)pass_pairs * m * sizeof(u64)) || !rb.place(out_block_))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_group_rows: out of device memory (scratch)");
  if (!h_evals_.reserve(8)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_group_rows: out of page-locked host memory");
  unsigned long long* d_evals = grp_work_.as<unsigned long long>();
  u32* d_sizes = reinterpret_cast<u32*>(d_evals + 1);
  // (device results: null where the caller passed null - group_sizes, counts - and the kernel skips them)
  int64_t* const d_gs = rb.dev(r_gs);
  int32_t* const d_cnt = rb.dev(r_cnt);

  rc = groups_representatives("search_group_rows", dq, nq, k, p, engine, page_rows, scratch_bytes);
  if (rc != EPS_OK) return rc;
  const u64* res = grp_res_.as<u64>();
  rc = clear_device_evals(d_evals);
  if (rc != EPS_OK) return rc;
  for (int64_t q0 = 0; q0 < nq; q0 += plan.slice) {
    GroupRowsArgs a;
    a.rows = d_rows_;
    a.dim = (int)dim_;
    a.metric = metric_;
    a.queries = dq + q0 * dim_;
    a.pairs = std::min(plan.slice, nq - q0) * k;
    a.k = k;
    a.m = m;
    a.f = filter_spec();
    a.res_keys = res + q0 * k;
    a.label = grp_label_.as<int32_t>();
    a.offsets = grp_offsets_.as<int64_t>();
    a.group_rows = grp_rowlist_.as<int32_t>();
    a.chunk = plan.chunk;
    a.sizes = d_sizes;
    a.prefix = d_sizes + pass_pairs;
    a.partial = partial_buf_.as<u64>();
    a.items = plan.items;
    a.waves = plan.waves;
    a.run_keys = grp_rows_run_.as<u64>();
    a.evals = d_evals;
    HIP_TRY(hipMemsetAsync(d_sizes, 0, (size_t)a.pairs * sizeof(u32), stream_));
    if (n > 0) {
      HIP_TRY(hipEventRecord(evk0_, stream_));
      launch_group_rows_gather(a, stream_);
      HIP_TRY(hipEventRecord(evk1_, stream_));
      launch_group_rows_merge(a, stream_);
    } else {   // no row: no group
      launch_fill_u64(a.run_keys, a.pairs * m, KEY_EMPTY, stream_);
    }
    launch_group_rows_finalize(a, id_base_, id_stride_, rb.dev(r_ids) + q0 * km, rb.dev(r_dist) + q0 * km, rb.dev(r_rc) + q0 * k,
                               d_gs ? d_gs + q0 * k : nullptr, d_cnt ? d_cnt + q0 : nullptr, stream_);
  }
  launch_groups_keys(res, nq, k, grp_label_.as<int32_t>(), grp_keys_.as<int64_t>(), rb.dev(r_gk), stream_);
  if (n > 0) set_main_kernel(1, n, nq, 32);
  rc = publish_device_evals(d_evals);   // (the second phase's pairs: last_stats adds them)
  if (rc != EPS_OK) return rc;
  HIP_TRY(hipEventRecord(ev1_, stream_));
  if (!out_dev) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  end_timed_call();
  return EPS_OK;
}

// ------------------------------------------------------------------------------------------------ search_multi
// The k closest groups per bag of vectors by the sum of each vector's distance to the group's closest visible row (multi.hip, plan: multi_host.hpp).
// cand_keys null: the whole-table form - search_groups' scan with the vectors of whole bags as its pseudo-queries, then sums, top-k and the answer
// read from the table.  Else the candidate form: labels of the named keys, work list, gather into a table per (bag, candidate) pair, then the same
// sums, top-k and answer.  No host sync of its own in either form.  Reports like a search; changes nothing a later call can observe.
int32_t Index::search_multi(const float* vectors, const int64_t* q_offsets, int64_t nq, const int64_t* cand_keys, const int64_t* cand_offsets, int64_t n_cand,
                            int32_t k, int64_t scratch_bytes, int64_t* group_keys, float* score, int32_t* counts, int64_t* match_ids, float* match_dist) {
  const char* why;
  if (multi_args_check(nq, k, n_cand, scratch_bytes, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_multi: ") + why);
  if (nq == 0) return EPS_OK;
  HIP_TRY(hipSetDevice(device_));
  if (!q_offsets) return fail(EPS_USER_ERROR, "search_multi: null buffer");
  if (is_device_ptr(q_offsets)) return fail(EPS_USER_ERROR, "search_multi: q_offsets must be a host array");
  int64_t T = 0, t_max = 0, longest = 0;
  if (multi_bags_check(q_offsets, nq, &T, &t_max, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_multi: ") + why);
  const bool cand = cand_keys != nullptr;
  if (!cand && (cand_offsets || n_cand > 0)) return fail(EPS_USER_ERROR, "search_multi: null buffer");   // (a list without its keys)
  if (cand_offsets && is_device_ptr(cand_offsets)) return fail(EPS_USER_ERROR, "search_multi: cand_offsets must be a host array");
  if (cand && among_lists_check(cand_offsets, nq, n_cand, &longest, &why) != EPS_OK) return fail(EPS_USER_ERROR, std::string("search_multi: ") + why);
  int32_t rc = groups_ready("search_multi");
  if (rc != EPS_OK) return rc;
  if ((T > 0 && !vectors) || !group_keys || !score || (match_ids == nullptr) != (match_dist == nullptr)) return fail(EPS_USER_ERROR, "search_multi: null buffer");
  ResultBlock rb;
  const auto r_gk = rb.add(group_keys, (size_t)nq * k);
  const auto r_mid = rb.add(match_ids, match_ids ? (size_t)T * k : 0);
  const auto r_score = rb.add(score, (size_t)nq * k);
  const auto r_md = rb.add(match_dist, match_dist ? (size_t)T * k : 0);
  const auto r_cnt = rb.add(counts, (size_t)nq);
  if (!rb.one_kind(is_device_ptr)) return fail(EPS_USER_ERROR, "search_multi: the output buffers must all be host or all be device pointers");
  const bool out_dev = rb.device();
  rc = check_filters_cover_table("search_multi");
  if (rc != EPS_OK) return rc;

  // ---- the plan, and the refusal of a bag that cannot be served whole - before any launch
  const int64_t n = n_rows_, G = grp_n_groups_;
  std::vector<int64_t> h_in((size_t)(nq + 1) * (cand ? (cand_offsets ? 4 : 3) : 1));   // [q_off | elements in front | pairs in front | cand_off]
  int64_t* const h_qoff = h_in.data();
  int64_t* const h_elems = cand ? h_qoff + (nq + 1) : h_qoff;
  int64_t* const h_pairs = cand ? h_elems + (nq + 1) : nullptr;
  std::memcpy(h_qoff, q_offsets, (size_t)(nq + 1) * sizeof(int64_t));
  int64_t largest_bytes = t_max * G * 8;
  if (cand) {
    if (cand_offsets) std::memcpy(h_pairs + (nq + 1), cand_offsets, (size_t)(nq + 1) * sizeof(int64_t));
    h_elems[0] = h_pairs[0] = 0;
    largest_bytes = 0;
    for (int64_t j = 0; j < nq; ++j) {   // (T, n_cand < 2^31: the totals stay below 2^62)
      const int64_t nc = cand_offsets ? cand_offsets[j + 1] - cand_offsets[j] : n_cand, t = q_offsets[j + 1] - q_offsets[j];
      h_pairs[j + 1] = h_pairs[j] + nc;
      h_elems[j + 1] = h_elems[j] + nc * t;
      largest_bytes = std::max(largest_bytes, nc * t * 8);
    }
  }
  int64_t cap_bytes = 0;
  if (!multi_scratch_cap(scratch_bytes, largest_bytes, &cap_bytes))
    return fail(EPS_DB_UNSUPPORTED_ERROR, "search_multi: a bag's own table needs " + std::to_string(largest_bytes) + " bytes, scratch_bytes allows " +
                                              std::to_string(scratch_bytes) + " (a bag is never cut)");
  const MultiTopkPlan plan = multi_topk_plan(cand ? longest : G, k);
  const int64_t cap_a = cand ? cap_bytes / 8 : multi_table_vectors(cap_bytes, G);
  if (cand) {
    rc = ensure_rows_by_group("search_multi");
    if (rc != EPS_OK) return rc;
  }
  begin_timed_call();
  prefilter_call_ = false;   // (@distance reads the row's exact distance)

  const float* dq = vectors;
  if (T > 0) {
    rc = stage_queries("search_multi", vectors, T, &dq, !out_dev);
    if (rc != EPS_OK) return rc;
  }

  // ---- scratch: [pair counter | the offsets above | a host list's keys], the candidates' labels; per pass: table, work list, partial and merged lists
  int64_t pass_elems = 0, pass_pairs = 0, pass_bags = 0;
  for (int64_t j0 = 0; j0 < nq;) {
    const int64_t j1 = multi_slice_end(h_elems, cap_a, h_pairs, MULTI_MAX_PAIRS, nq, j0, plan.bags);
    pass_elems = std::max(pass_elems, (h_elems[j1] - h_elems[j0]) * (cand ? 1 : G));
    if (cand) pass_pairs = std::max(pass_pairs, h_pairs[j1] - h_pairs[j0]);
    pass_bags = std::max(pass_bags, j1 - j0);
    j0 = j1;
  }
  const bool keys_dev = cand && n_cand > 0 && is_device_ptr(cand_keys);
  const size_t in_bytes = h_in.size() * sizeof(int64_t), list_bytes = (cand && !keys_dev) ? (size_t)n_cand * sizeof(int64_t) : 0;
  if (!multi_in_.reserve(8 + in_bytes + list_bytes) || !grp_table_.reserve((size_t)pass_elems * sizeof(u64)) ||
      !partial_buf_.reserve((size_t)pass_bags * plan.W * k * sizeof(u64)) || !grp_run_.reserve((size_t)pass_bags * k * sizeof(u64)) ||
      (cand && (!multi_label_.reserve((size_t)n_cand * sizeof(int32_t)) || !multi_prefix_.reserve((size_t)(pass_pairs + 1) * sizeof(unsigned long long)))) ||
      !rb.place(out_block_))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_multi: out of device memory (scratch)");
  if (!h_evals_.reserve(8)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "search_multi: out of page-locked host memory");
  unsigned long long* d_evals = multi_in_.as<unsigned long long>();
  int64_t* const d_in = multi_in_.as<int64_t>() + 1;
  rc = clear_device_evals(d_evals);
  if (rc != EPS_OK) return rc;
  rc = copy_host_in(d_in, h_in.data(), in_bytes, !out_dev);
  if (rc != EPS_OK) return rc;
  const int64_t* d_keys = cand_keys;
  if (cand && !keys_dev && n_cand > 0) {
    d_keys = reinterpret_cast<const int64_t*>(multi_in_.as<char>() + 8 + in_bytes);
    rc = copy_host_in(const_cast<int64_t*>(d_keys), cand_keys, list_bytes, !out_dev);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(ev0_, stream_));
  if (cand) launch_multi_labels(d_keys, n_cand, grp_keys_.as<int64_t>(), G, multi_label_.as<int32_t>(), stream_);

  MultiArgs a;
  a.rows = d_rows_;
  a.dim = (int)dim_;
  a.metric = metric_;
  a.f = filter_spec();
  a.vectors = dq;
  a.q_off = d_in;
  a.k = k;
  a.G = G;
  a.table = grp_table_.as<u64>();
  a.base_off = cand ? d_in + (nq + 1) : d_in;
  a.plan = plan;
  a.partial = partial_buf_.as<u64>();
  a.run_keys = grp_run_.as<u64>();
  a.cand_label = cand ? multi_label_.as<int32_t>() : nullptr;
  if (cand && n_cand == 0) a.cand_label = reinterpret_cast<const int32_t*>(d_in);   // (never read: no bag has a candidate; non-null marks the form)
  a.cand_off = cand_offsets ? d_in + 3 * (nq + 1) : nullptr;
  a.n_cand = n_cand;
  a.offsets = grp_offsets_.as<int64_t>();
  a.group_rows = grp_rowlist_.as<int32_t>();
  a.prefix = multi_prefix_.as<unsigned long long>();
  a.evals = d_evals;
  int64_t launches = 0, vectors_scanned = 0;
  for (int64_t j0 = 0; j0 < nq;) {
    const int64_t j1 = multi_slice_end(h_elems, cap_a, h_pairs, MULTI_MAX_PAIRS, nq, j0, plan.bags);
    a.j0 = j0;
    a.bags = j1 - j0;
    const int64_t elems = (h_elems[j1] - h_elems[j0]) * (cand ? 1 : G);
    a.pairs = cand ? h_pairs[j1] - h_pairs[j0] : 0;
    if (elems > 0 && n > 0) {
      launch_fill_u64(a.table, elems, KEY_EMPTY, stream_);
      HIP_TRY(hipEventRecord(evk0_, stream_));
      if (cand) {
        a.waves = std::min<int64_t>(MULTI_MAX_WAVES, a.pairs * multi_pair_items(grp_largest_, t_max));   // (pairs < 2^31, items < 2^31)
        launch_multi_gather(a, stream_);
      } else {
        const int64_t m = h_qoff[j1] - h_qoff[j0];
        GroupsScanArgs g;
        g.rows = d_rows_;
        g.n = n;
        g.dim = (int)dim_;
        g.metric = metric_;
        g.queries = dq + h_qoff[j0] * dim_;
        g.m = m;
        g.qsel = nullptr;
        g.f = a.f;
        g.label = grp_label_.as<int32_t>();
        g.best = a.table;
        g.G = G;
        g.W = flat_scan_waves(n, m, (int)dim_);
        launch_groups_min_scan(g, stream_);
        vectors_scanned += m;
      }
      HIP_TRY(hipEventRecord(evk1_, stream_));
      launches = 1;
    }
    launch_multi_sum_topk(a, stream_);
    launch_among_merge(a.partial, plan.W, k, a.bags, a.run_keys, stream_);
    launch_multi_finalize(a, grp_keys_.as<int64_t>(), id_base_, id_stride_, rb.dev(r_gk), rb.dev(r_score), rb.dev(r_cnt),
                          match_ids ? rb.dev(r_mid) : nullptr, match_ids ? rb.dev(r_md) : nullptr, stream_);   // (no matches asked for: their parts are empty)
    j0 = j1;
  }
  set_main_kernel(launches, cand ? n_cand : n, cand ? nq : vectors_scanned, 32);
  stats_.dist_evals += vectors_scanned * n;
  rc = publish_device_evals(d_evals);   // (the gather's pairs: last_stats adds them)
  if (rc != EPS_OK) return rc;
  HIP_TRY(hipEventRecord(ev1_, stream_));
  if (!out_dev) {
    rc = fetch_to_host(rb);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  end_timed_call();
  return EPS_OK;
}

int32_t Index::last_stats(eps_search_stats* out) {
  eps_search_stats s = stats_;
  // event timings are read lazily: the caller may have left the work in flight
  if (ev0_ && hipEventSynchronize(ev1_) == hipSuccess) {
    if (evals_pending_) s.dist_evals += (int64_t)*static_cast<const unsigned long long*>(h_evals_.p);   // (counted on the device, copied out in front of ev1_)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) s.kernel_ms = ms;
    if (s.main_kernel_launches > 0 && hipEventElapsedTime(&ms, evk0_, evk1_) == hipSuccess) s.main_kernel_ms = ms;
    double all = 0.0;
    for (int i = 0; i < stage_n_; ++i)
      if (hipEventElapsedTime(&ms, stage_ev_[i][0], stage_ev_[i][1]) == hipSuccess) all += ms;
    s.filter_ms_all = all;
  }
  (void)hipGetLastError();
  *out = s;
  return EPS_OK;
}

// main-kernel milliseconds of the most recent search calls (oldest first); synchronises the stream
int Index::kernel_times(double* ms_out, int cap) {
  if (!ms_out || cap <= 0) return 0;
  if (hipSetDevice(device_) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int n = 0;
  const int64_t first = std::max<int64_t>(1, kring_seq_ - std::min<int64_t>(cap, KRING) + 1);
  for (int64_t q = first; q <= kring_seq_; ++q) {
    const int slot = (int)(q % KRING);
    if (!kring_valid_[slot]) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, kring_[slot][0], kring_[slot][1]) == hipSuccess) ms_out[n++] = ms;
    else (void)hipGetLastError();
  }
  return n;
}

}  // namespace eps
