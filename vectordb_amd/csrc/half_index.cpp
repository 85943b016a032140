// Host side of the half-vector index (eps_half_index_*, see index.hpp; limits, rounding, refusals, the launch plan and the seed rule: half_host.hpp;
// kernels: half.hip).
#include "index.hpp"

#include <cstring>
#include <string>
#include <utility>

namespace eps {

HalfIndex::~HalfIndex() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t e : {ev0_, ev1_, evk0_, evk1_})
    if (e) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int32_t HalfIndex::hip_fail(hipError_t e, const char* what) {
  (void)hipGetLastError();
  return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

int32_t HalfIndex::init() {   // (Index::init's rules)
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "no HIP device available: libepsilla_gfx950 has no CPU fallback");
  }
  if (device_ < 0 || device_ >= count) return fail(EPS_USER_ERROR, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device_));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  own_stream_ = true;
  HIP_TRY(hipEventCreate(&ev0_));
  HIP_TRY(hipEventCreate(&ev1_));
  HIP_TRY(hipEventCreate(&evk0_));
  HIP_TRY(hipEventCreate(&evk1_));
  half_scan_allow_lds();
  HIP_TRY(hipGetLastError());
  if (!hit_buf_.reserve(16)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "out of device memory");
  return EPS_OK;
}

int32_t HalfIndex::set_stream(void* s) {
  HIP_TRY(hipSetDevice(device_));
  if (stream_) HIP_TRY(hipStreamSynchronize(stream_));
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
  own_stream_ = false;
  if (s) {
    stream_ = static_cast<hipStream_t>(s);
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  return EPS_OK;
}

int32_t HalfIndex::synchronize() {
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

// The handle always owns its table: the stored form (padded rows, norm terms) is not what the caller has.  Device elements are read in place by the
// prepare launch; host elements go through a staging buffer in slabs.  src_float: rows of floats, rounded to the handle's type by the same launch
int32_t HalfIndex::attach(const void* src, int64_t n, int64_t stride_elems, int src_float) {
  const char* who = src_float ? "attach_floats: " : "attach_rows: ";
  if (const char* why = half_attach_refusal(dim_, src, n, stride_elems)) return fail(EPS_USER_ERROR, std::string(who) + why);
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));   // (no search of the previous table is in flight when it goes)
  const int64_t n_pad = half_pad_rows(n);
  const int64_t es = src_float ? 4 : 2;     // bytes of a source element
  DevBuf t, tt;
  if (!t.reserve((size_t)(n_pad > 0 ? n_pad : 1) * d_pad_ * 2) || !tt.reserve((size_t)(n_pad > 0 ? n_pad : 1) * 4))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + "out of device memory");
  if (n > 0 && is_device_ptr(src)) {
    launch_half_prepare(src, src_float, n, n_pad, dim_, stride_elems, metric_, bf16_, t.as<uint16_t>(), tt.as<float>(), stream_);
    HIP_TRY(hipGetLastError());
  } else if (n > 0) {
    int64_t slab = ((int64_t)64 << 20) / (dim_ * es) / HALF_WAVE_ROWS * HALF_WAVE_ROWS;   // rows staged at once: 64 MB, whole rounds
    slab = slab > n_pad ? n_pad : slab;
    if (!stage_buf_.reserve((size_t)slab * dim_ * es)) return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(who) + "out of device memory (staging)");
    const char* base = static_cast<const char*>(src);
    for (int64_t r = 0; r < n; r += slab) {   // (stream order: a slab is prepared before the next copy overwrites it)
      const int64_t c = n - r < slab ? n - r : slab;
      const int64_t c_pad = n_pad - r < slab ? n_pad - r : slab;   // the last slab also writes the zero rows behind n
      HIP_TRY(hipMemcpy2DAsync(stage_buf_.p, (size_t)(dim_ * es), base + r * stride_elems * es, (size_t)(stride_elems * es), (size_t)(dim_ * es), (size_t)c,
                               hipMemcpyHostToDevice, stream_));
      launch_half_prepare(stage_buf_.p, src_float, c, c_pad, dim_, dim_, metric_, bf16_, t.as<uint16_t>() + r * d_pad_, tt.as<float>() + r, stream_);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipStreamSynchronize(stream_));   // the caller's rows are the caller's again
  std::swap(table_buf_.p, t.p);
  std::swap(table_buf_.cap, t.cap);
  std::swap(term_buf_.p, tt.p);
  std::swap(term_buf_.cap, tt.cap);
  n_ = n;
  d_deleted_ = nullptr;   // a new table: the bitset of the previous one is forgotten
  return EPS_OK;
}

// x [m][dim] floats -> halves_out [m][dim], both host - the call synchronises - or both device - asynchronous on the handle's stream
int32_t HalfIndex::convert_floats(const float* x, int64_t m, void* halves_out) {
  if (m < 0 || m > HALF_MAX_ROWS) return fail(EPS_USER_ERROR, "convert_floats: m must be in [0, 2^31 - 1]");
  if (m == 0) return EPS_OK;
  if (!x || !halves_out) return fail(EPS_USER_ERROR, "convert_floats: null buffer");
  HIP_TRY(hipSetDevice(device_));
  const bool dev = is_device_ptr(x);
  if (is_device_ptr(halves_out) != dev) return fail(EPS_USER_ERROR, "convert_floats: x and halves_out must both be host or both be device pointers");
  const int64_t count = m * dim_;
  if (dev) {
    launch_half_convert(x, count, bf16_, static_cast<uint16_t*>(halves_out), stream_);
    HIP_TRY(hipGetLastError());
    return EPS_OK;
  }
  HIP_TRY(hipStreamSynchronize(stream_));
  if (!stage_buf_.reserve((size_t)count * 4) || !out_buf_.reserve((size_t)count * 2))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "convert_floats: out of device memory");
  HIP_TRY(hipMemcpyAsync(stage_buf_.p, x, (size_t)count * 4, hipMemcpyHostToDevice, stream_));
  launch_half_convert(stage_buf_.as<float>(), count, bf16_, out_buf_.as<uint16_t>(), stream_);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(halves_out, out_buf_.p, (size_t)count * 2, hipMemcpyDeviceToHost, stream_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

int32_t HalfIndex::set_id_map(int64_t base, int64_t stride) {
  if (stride <= 0) return fail(EPS_USER_ERROR, "set_id_map: stride must be positive");
  id_base_ = base;
  id_stride_ = stride;
  return EPS_OK;
}

int32_t HalfIndex::set_deleted(const uint8_t* bits, int64_t nbytes) {
  HIP_TRY(hipSetDevice(device_));
  if (!bits || nbytes <= 0) {
    d_deleted_ = nullptr;
    return EPS_OK;
  }
  if (nbytes < (n_ + 7) / 8) return fail(EPS_USER_ERROR, "set_deleted: bitset shorter than ceil(rows/8) bytes");
  if (is_device_ptr(bits)) {
    d_deleted_ = bits;
    return EPS_OK;
  }
  HIP_TRY(hipStreamSynchronize(stream_));   // (a search in flight reads the previous copy)
  if (!deleted_buf_.reserve((size_t)nbytes)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "set_deleted: out of device memory");
  HIP_TRY(hipMemcpyAsync(deleted_buf_.p, bits, (size_t)nbytes, hipMemcpyHostToDevice, stream_));
  HIP_TRY(hipStreamSynchronize(stream_));   // the host bitset may change right after we return
  d_deleted_ = deleted_buf_.as<uint8_t>();
  return EPS_OK;
}

int32_t HalfIndex::search(const void* queries, int64_t nq, int32_t k, int64_t* ids, float* dist, int32_t* counts) {
  if (const char* why = half_search_refusal(nq, k)) return fail(EPS_USER_ERROR, std::string("search: ") + why);
  if (nq == 0) return EPS_OK;
  if (!queries || !ids || !dist) return fail(EPS_USER_ERROR, "search: null buffer");
  HIP_TRY(hipSetDevice(device_));
  const bool dev = is_device_ptr(queries);
  if (is_device_ptr(ids) != dev || is_device_ptr(dist) != dev || (counts && is_device_ptr(counts) != dev))
    return fail(EPS_USER_ERROR, "search: queries, ids_out, dist_out and counts_out must all be host or all be device pointers");

  // ---- scratch: a host batch's halves, the stored queries and their terms, the seed bounds, partial lists, result keys, host results' device
  // block.  Device buffers: no host synchronisation - the scratch of the previous call is reused in stream order
  const int64_t n = n_;
  const HalfPlan plan = half_plan(n, dim_, nq, k);
  const int64_t seed_rows = half_seed_rows(n, dim_, nq, k);
  const HalfPlan seed_plan = half_plan(seed_rows, dim_, nq, k);
  const size_t partial_bytes = (size_t)(seed_rows > 0 && seed_plan.partial_bytes > plan.partial_bytes ? seed_plan.partial_bytes : plan.partial_bytes);
  const size_t raw_bytes = (size_t)nq * dim_ * 2;
  const size_t ids_bytes = (size_t)nq * k * sizeof(int64_t), dist_bytes = (size_t)nq * k * sizeof(float), out_bytes = ids_bytes + dist_bytes + (size_t)nq * sizeof(int32_t);
  if (!dev) HIP_TRY(hipStreamSynchronize(stream_));
  if (!partial_buf_.reserve(partial_bytes) || !run_buf_.reserve((size_t)plan.run_bytes) || !q_buf_.reserve((size_t)nq * d_pad_ * 2) ||
      !qterm_buf_.reserve((size_t)nq * 4) || !seed_buf_.reserve((size_t)nq * 4) || (!dev && (!stage_buf_.reserve(raw_bytes) || !out_buf_.reserve(out_bytes))))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (scratch)");
  const void* d_raw = queries;
  int64_t* d_ids = ids;
  float* d_dist = dist;
  int32_t* d_cnt = counts;
  if (!dev) {
    HIP_TRY(hipMemcpyAsync(stage_buf_.p, queries, raw_bytes, hipMemcpyHostToDevice, stream_));
    d_raw = stage_buf_.p;
    d_ids = out_buf_.as<int64_t>();
    d_dist = reinterpret_cast<float*>(out_buf_.as<char>() + ids_bytes);
    d_cnt = reinterpret_cast<int32_t*>(out_buf_.as<char>() + ids_bytes + dist_bytes);
  }
  std::memset(&stats_, 0, sizeof(stats_));
  u64* run_keys = run_buf_.as<u64>();
  HIP_TRY(hipEventRecord(ev0_, stream_));
  stats_.main_kernel_rows = n;
  stats_.main_kernel_queries = nq;
  stats_.main_kernel_bits = 16;
  stats_.dist_evals = (n + seed_rows) * nq;
  stats_.expansions = plan.cols * 100 + plan.kpl;   // the form of the scan
  stats_.overflow_queries = seed_rows > 0;          // the thresholds were seeded
  stats_.i8_folded = seed_rows;                     // rows of the prefix
  launch_fill_u64(hit_buf_.as<u64>(), 2, 0ull, stream_);
  if (n > 0) {
    launch_half_prepare(d_raw, 0, nq, nq, dim_, dim_, metric_, bf16_, q_buf_.as<uint16_t>(), qterm_buf_.as<float>(), stream_);
    HalfScanArgs a;
    a.rows = table_buf_.as<uint16_t>();
    a.row_term = term_buf_.as<float>();
    a.d_pad = (int)d_pad_;
    a.metric = metric_;
    a.is_bf16 = bf16_;
    a.queries = q_buf_.as<uint16_t>();
    a.query_term = qterm_buf_.as<float>();
    a.nq = nq;
    a.k = k;
    a.deleted = d_deleted_;
    a.partial = partial_buf_.as<u64>();
    a.seed = nullptr;
    if (seed_rows > 0) {   // the prefix's top-k, its k-th distance as every slice's first bound
      a.n = seed_rows;
      a.plan = seed_plan;
      a.hit_rounds = hit_buf_.as<u64>() + 1;
      launch_half_scan(a, stream_);
      launch_merge_lists(a.partial, (int)(seed_plan.slices * k), k, nq, run_keys, false, stream_);
      launch_half_seed(run_keys, nq, k, seed_buf_.as<u32>(), stream_);
      a.seed = seed_buf_.as<u32>();
    }
    a.n = n;
    a.plan = plan;
    a.hit_rounds = hit_buf_.as<u64>();
    HIP_TRY(hipEventRecord(evk0_, stream_));
    launch_half_scan(a, stream_);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    launch_merge_lists(a.partial, (int)(plan.slices * k), k, nq, run_keys, false, stream_);
    stats_.main_kernel_launches = plan.launches;
    stats_.filter_rows_all = plan.rounds;
  } else {
    launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
  }
  launch_half_finalize(run_keys, nq, k, id_base_, id_stride_, d_ids, d_dist, d_cnt, stream_);
  HIP_TRY(hipEventRecord(ev1_, stream_));
  HIP_TRY(hipGetLastError());
  if (!dev) {
    HIP_TRY(hipMemcpyAsync(ids, d_ids, ids_bytes, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(dist, d_dist, dist_bytes, hipMemcpyDeviceToHost, stream_));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, d_cnt, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
  }
  return EPS_OK;
}

int32_t HalfIndex::last_stats(eps_search_stats* out) {
  eps_search_stats s = stats_;
  if (ev0_ && s.main_kernel_queries > 0 && hipEventSynchronize(ev1_) == hipSuccess) {   // (read lazily: the caller may have left the work in flight)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) s.kernel_ms = ms;
    if (s.main_kernel_launches > 0 && hipEventElapsedTime(&ms, evk0_, evk1_) == hipSuccess) s.main_kernel_ms = ms;
    u64 hits[2] = {0, 0};   // (the call is complete: nothing writes the counters until the next search zeroes them)
    if (hipMemcpy(hits, hit_buf_.p, 16, hipMemcpyDeviceToHost) == hipSuccess) {
      s.rerank_rows = (int64_t)hits[0];
      s.i8_declined = (int64_t)hits[1];   // hit rounds of the seed pass, whose slices all start open
    }
  }
  (void)hipGetLastError();
  *out = s;
  return EPS_OK;
}

}  // namespace eps
