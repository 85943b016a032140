// Host side of the byte-vector index (eps_byte_index_*, see index.hpp; limits, terms, refusals and the launch plan: byte_host.hpp; kernels: byte.hip).
#include "index.hpp"

#include <cstring>
#include <string>
#include <utility>

namespace eps {

ByteIndex::~ByteIndex() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t e : {ev0_, ev1_, evk0_, evk1_})
    if (e) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int32_t ByteIndex::hip_fail(hipError_t e, const char* what) {
  (void)hipGetLastError();
  return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

int32_t ByteIndex::init() {   // (Index::init's rules)
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
  byte_scan_allow_lds();
  HIP_TRY(hipGetLastError());
  if (!hit_buf_.reserve(8)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "out of device memory");
  return EPS_OK;
}

int32_t ByteIndex::set_stream(void* s) {
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

int32_t ByteIndex::synchronize() {
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

// The handle always owns its table: the stored form (padded rows, shifted unsigned bytes, row terms) is not what the caller has.  Device bytes are
// read in place by the prepare launch; host bytes go through a staging buffer in slabs.
int32_t ByteIndex::attach_rows(const void* bytes, int64_t n, int64_t stride_bytes) {
  if (const char* why = byte_attach_refusal(dim_, bytes, n, stride_bytes)) return fail(EPS_USER_ERROR, std::string("attach_rows: ") + why);
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));   // (no search of the previous table is in flight when it goes)
  const int64_t n_pad = byte_pad_rows(n);
  DevBuf t, tt;
  if (!t.reserve((size_t)(n_pad > 0 ? n_pad : 1) * d_pad_) || !tt.reserve((size_t)(n_pad > 0 ? n_pad : 1) * 4))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_rows: out of device memory");
  const uint8_t* src = static_cast<const uint8_t*>(bytes);
  if (n > 0 && is_device_ptr(bytes)) {
    launch_byte_prepare(src, n, n_pad, dim_, stride_bytes, metric_, unsigned_, 0, t.as<signed char>(), tt.as<int32_t>(), stream_);
    HIP_TRY(hipGetLastError());
  } else if (n > 0) {
    int64_t slab = ((int64_t)64 << 20) / dim_ / BYTE_WAVE_ROWS * BYTE_WAVE_ROWS;   // rows staged at once: 64 MB, whole rounds
    slab = slab > n_pad ? n_pad : slab;
    if (!stage_buf_.reserve((size_t)slab * dim_)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_rows: out of device memory (staging)");
    for (int64_t r = 0; r < n; r += slab) {   // (stream order: a slab is prepared before the next copy overwrites it)
      const int64_t c = n - r < slab ? n - r : slab;
      const int64_t c_pad = n_pad - r < slab ? n_pad - r : slab;   // the last slab also writes the zero rows behind n
      HIP_TRY(hipMemcpy2DAsync(stage_buf_.p, (size_t)dim_, src + r * stride_bytes, (size_t)stride_bytes, (size_t)dim_, (size_t)c, hipMemcpyHostToDevice, stream_));
      launch_byte_prepare(stage_buf_.as<uint8_t>(), c, c_pad, dim_, dim_, metric_, unsigned_, 0, t.as<signed char>() + r * d_pad_, tt.as<int32_t>() + r, stream_);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipStreamSynchronize(stream_));   // the caller's bytes are the caller's again
  std::swap(table_buf_.p, t.p);
  std::swap(table_buf_.cap, t.cap);
  std::swap(term_buf_.p, tt.p);
  std::swap(term_buf_.cap, tt.cap);
  n_ = n;
  d_deleted_ = nullptr;   // a new table: the bitset of the previous one is forgotten
  return EPS_OK;
}

int32_t ByteIndex::set_id_map(int64_t base, int64_t stride) {
  if (stride <= 0) return fail(EPS_USER_ERROR, "set_id_map: stride must be positive");
  id_base_ = base;
  id_stride_ = stride;
  return EPS_OK;
}

int32_t ByteIndex::set_deleted(const uint8_t* bits, int64_t nbytes) {
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

int32_t ByteIndex::search(const void* queries, int64_t nq, int32_t k, int64_t* ids, int32_t* dist, int32_t* counts) {
  if (const char* why = byte_search_refusal(nq, k)) return fail(EPS_USER_ERROR, std::string("search: ") + why);
  if (nq == 0) return EPS_OK;
  if (!queries || !ids || !dist) return fail(EPS_USER_ERROR, "search: null buffer");
  HIP_TRY(hipSetDevice(device_));
  const bool dev = is_device_ptr(queries);
  if (is_device_ptr(ids) != dev || is_device_ptr(dist) != dev || (counts && is_device_ptr(counts) != dev))
    return fail(EPS_USER_ERROR, "search: queries, ids_out, dist_out and counts_out must all be host or all be device pointers");

  // ---- scratch: a host batch's bytes, the stored queries and their terms, partial lists, result keys, host results' device block.  Device
  // buffers: no host synchronisation - the scratch of the previous call is reused in stream order
  const int64_t n = n_;
  const BytePlan plan = byte_plan(n, dim_, nq, k);
  const size_t raw_bytes = (size_t)nq * dim_;
  const size_t ids_bytes = (size_t)nq * k * sizeof(int64_t), dist_bytes = (size_t)nq * k * sizeof(int32_t), out_bytes = ids_bytes + dist_bytes + (size_t)nq * sizeof(int32_t);
  if (!dev) HIP_TRY(hipStreamSynchronize(stream_));
  if (!partial_buf_.reserve((size_t)plan.partial_bytes) || !run_buf_.reserve((size_t)plan.run_bytes) || !q_buf_.reserve((size_t)nq * d_pad_) ||
      !qterm_buf_.reserve((size_t)nq * 4) || (!dev && (!stage_buf_.reserve(raw_bytes) || !out_buf_.reserve(out_bytes))))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (scratch)");
  const uint8_t* d_raw = static_cast<const uint8_t*>(queries);
  int64_t* d_ids = ids;
  int32_t* d_dist = dist;
  int32_t* d_cnt = counts;
  if (!dev) {
    HIP_TRY(hipMemcpyAsync(stage_buf_.p, queries, raw_bytes, hipMemcpyHostToDevice, stream_));
    d_raw = stage_buf_.as<uint8_t>();
    d_ids = out_buf_.as<int64_t>();
    d_dist = reinterpret_cast<int32_t*>(out_buf_.as<char>() + ids_bytes);
    d_cnt = reinterpret_cast<int32_t*>(out_buf_.as<char>() + ids_bytes + dist_bytes);
  }
  std::memset(&stats_, 0, sizeof(stats_));
  u64* run_keys = run_buf_.as<u64>();
  HIP_TRY(hipEventRecord(ev0_, stream_));
  stats_.main_kernel_rows = n;
  stats_.main_kernel_queries = nq;
  stats_.main_kernel_bits = 8;
  stats_.dist_evals = n * nq;
  stats_.expansions = plan.cols * 100 + plan.kpl;   // the form of the scan
  launch_fill_u64(hit_buf_.as<u64>(), 1, 0ull, stream_);
  if (n > 0) {
    launch_byte_prepare(d_raw, nq, nq, dim_, dim_, metric_, unsigned_, 1, q_buf_.as<signed char>(), qterm_buf_.as<int32_t>(), stream_);
    ByteScanArgs a;
    a.rows = table_buf_.as<signed char>();
    a.row_term = term_buf_.as<int32_t>();
    a.n = n;
    a.d_pad = (int)d_pad_;
    a.shift = byte_dot_shift(metric_);
    a.queries = q_buf_.as<signed char>();
    a.query_term = qterm_buf_.as<int32_t>();
    a.nq = nq;
    a.k = k;
    a.deleted = d_deleted_;
    a.plan = plan;
    a.partial = partial_buf_.as<u64>();
    a.hit_rounds = hit_buf_.as<u64>();
    HIP_TRY(hipEventRecord(evk0_, stream_));
    launch_byte_scan(a, stream_);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    launch_merge_lists(a.partial, (int)(plan.slices * k), k, nq, run_keys, false, stream_);
    stats_.main_kernel_launches = plan.launches;
    stats_.filter_rows_all = plan.rounds;
  } else {
    launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
  }
  launch_byte_finalize(run_keys, nq, k, id_base_, id_stride_, d_ids, d_dist, d_cnt, stream_);
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

int32_t ByteIndex::last_stats(eps_search_stats* out) {
  eps_search_stats s = stats_;
  if (ev0_ && s.main_kernel_queries > 0 && hipEventSynchronize(ev1_) == hipSuccess) {   // (read lazily: the caller may have left the work in flight)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) s.kernel_ms = ms;
    if (s.main_kernel_launches > 0 && hipEventElapsedTime(&ms, evk0_, evk1_) == hipSuccess) s.main_kernel_ms = ms;
    u64 hits = 0;   // (the call is complete: nothing writes the counter until the next search zeroes it)
    if (hipMemcpy(&hits, hit_buf_.p, 8, hipMemcpyDeviceToHost) == hipSuccess) s.rerank_rows = (int64_t)hits;
  }
  (void)hipGetLastError();
  *out = s;
  return EPS_OK;
}

}  // namespace eps
