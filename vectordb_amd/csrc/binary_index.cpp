// Host side of the binary-vector index (eps_binary_index_*, see index.hpp; limits, refusals and the launch plan: binary_host.hpp; kernels: binary.hip).
#include "index.hpp"

#include <cstring>
#include <string>
#include <utility>

namespace eps {

BinaryIndex::~BinaryIndex() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t e : {ev0_, ev1_, evk0_, evk1_})
    if (e) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int32_t BinaryIndex::hip_fail(hipError_t e, const char* what) {
  (void)hipGetLastError();
  return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

int32_t BinaryIndex::init() {   // (Index::init's rules)
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
  return EPS_OK;
}

int32_t BinaryIndex::set_stream(void* s) {
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

int32_t BinaryIndex::synchronize() {
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

int32_t BinaryIndex::attach_rows(const uint32_t* words, int64_t n, int64_t stride_words) {
  if (const char* why = binary_attach_refusal(dim_, words, n, stride_words)) return fail(EPS_USER_ERROR, std::string("attach_rows: ") + why);
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));   // (no search of the previous table is in flight when it goes)
  if (n > 0 && is_device_ptr(words)) {      // borrowed
    table_buf_.release();
    rows_ = words;
    stride_ = stride_words;
  } else {
    const int64_t own = binary_owned_stride(W_);
    DevBuf t;
    if (!t.reserve((size_t)(n > 0 ? n : 1) * own * 4)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_rows: out of device memory");
    if (n > 0 && stride_words == own)
      HIP_TRY(hipMemcpyAsync(t.p, words, (size_t)n * own * 4, hipMemcpyHostToDevice, stream_));
    else if (n > 0)
      HIP_TRY(hipMemcpy2DAsync(t.p, (size_t)own * 4, words, (size_t)stride_words * 4, (size_t)W_ * 4, (size_t)n, hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));   // the host words may change right after we return
    std::swap(table_buf_.p, t.p);
    std::swap(table_buf_.cap, t.cap);
    rows_ = table_buf_.as<uint32_t>();
    stride_ = own;
  }
  n_ = n;
  d_deleted_ = nullptr;   // a new table: the bitset of the previous one is forgotten
  return EPS_OK;
}

int32_t BinaryIndex::pack_to(const float* x, bool x_dev, int64_t m, uint32_t* words, int64_t stride) {
  if (x_dev) {
    launch_binary_pack(x, m, dim_, words, stride, stream_);
    HIP_TRY(hipGetLastError());
    return EPS_OK;
  }
  int64_t slab = ((int64_t)64 << 20) / (dim_ * 4);   // rows staged at once: 64 MB of floats
  slab = slab < 1 ? 1 : (slab > m ? m : slab);
  if (!stage_buf_.reserve((size_t)slab * dim_ * 4)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "out of device memory (staging)");
  for (int64_t r = 0; r < m; r += slab) {   // (stream order: a slab is packed before the next copy overwrites it)
    const int64_t c = m - r < slab ? m - r : slab;
    HIP_TRY(hipMemcpyAsync(stage_buf_.p, x + r * dim_, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_));
    launch_binary_pack(stage_buf_.as<float>(), c, dim_, words + r * stride, stride, stream_);
    HIP_TRY(hipGetLastError());
  }
  return EPS_OK;
}

int32_t BinaryIndex::attach_signs(const float* rows, int64_t n) {
  if (const char* why = binary_attach_refusal(dim_, rows, n, W_)) return fail(EPS_USER_ERROR, std::string("attach_signs: ") + why);
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  const int64_t own = binary_owned_stride(W_);
  DevBuf t;
  if (!t.reserve((size_t)(n > 0 ? n : 1) * own * 4)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_signs: out of device memory");
  if (n > 0) {
    const int32_t rc = pack_to(rows, is_device_ptr(rows), n, t.as<uint32_t>(), own);
    if (rc != EPS_OK) return rc;
  }
  HIP_TRY(hipStreamSynchronize(stream_));   // the floats are the caller's again
  std::swap(table_buf_.p, t.p);
  std::swap(table_buf_.cap, t.cap);
  rows_ = table_buf_.as<uint32_t>();
  stride_ = own;
  n_ = n;
  d_deleted_ = nullptr;
  return EPS_OK;
}

int32_t BinaryIndex::pack_signs(const float* x, int64_t m, uint32_t* words_out) {
  if (m < 0) return fail(EPS_USER_ERROR, "pack_signs: m must be >= 0");
  if (m == 0) return EPS_OK;
  if (!x || !words_out) return fail(EPS_USER_ERROR, "pack_signs: null buffer");
  HIP_TRY(hipSetDevice(device_));
  const bool dev = is_device_ptr(x);
  if (is_device_ptr(words_out) != dev) return fail(EPS_USER_ERROR, "pack_signs: x and words_out must both be host or both be device arrays");
  if (dev) return pack_to(x, true, m, words_out, W_);   // asynchronous on the handle's stream
  HIP_TRY(hipStreamSynchronize(stream_));
  const size_t bytes = (size_t)m * W_ * 4;
  if (!out_buf_.reserve(bytes)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "pack_signs: out of device memory");
  const int32_t rc = pack_to(x, false, m, out_buf_.as<uint32_t>(), W_);
  if (rc != EPS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(words_out, out_buf_.p, bytes, hipMemcpyDeviceToHost, stream_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

int32_t BinaryIndex::set_id_map(int64_t base, int64_t stride) {
  if (stride <= 0) return fail(EPS_USER_ERROR, "set_id_map: stride must be positive");
  id_base_ = base;
  id_stride_ = stride;
  return EPS_OK;
}

int32_t BinaryIndex::set_deleted(const uint8_t* bits, int64_t nbytes) {
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

int32_t BinaryIndex::search(const uint32_t* queries, int64_t nq, int32_t k, int64_t* ids, int32_t* dist, int32_t* counts) {
  if (const char* why = binary_search_refusal(nq, k)) return fail(EPS_USER_ERROR, std::string("search: ") + why);
  if (nq == 0) return EPS_OK;
  if (!queries || !ids || !dist) return fail(EPS_USER_ERROR, "search: null buffer");
  HIP_TRY(hipSetDevice(device_));
  const bool dev = is_device_ptr(queries);
  if (is_device_ptr(ids) != dev || is_device_ptr(dist) != dev || (counts && is_device_ptr(counts) != dev))
    return fail(EPS_USER_ERROR, "search: queries, ids_out, dist_out and counts_out must all be host or all be device pointers");

  // ---- scratch: a host batch's words, partial lists, result keys, host results' device block.  Device buffers: no host synchronisation - the
  // scratch of the previous call is reused in stream order
  const int64_t n = n_;
  const BinaryPlan plan = binary_plan(n, nq, k);
  const size_t q_bytes = (size_t)nq * W_ * 4;
  const size_t ids_bytes = (size_t)nq * k * sizeof(int64_t), dist_bytes = (size_t)nq * k * sizeof(int32_t), out_bytes = ids_bytes + dist_bytes + (size_t)nq * sizeof(int32_t);
  if (!dev) HIP_TRY(hipStreamSynchronize(stream_));
  if (!partial_buf_.reserve((size_t)plan.partial_bytes) || !run_buf_.reserve((size_t)plan.run_bytes) ||
      (!dev && (!q_buf_.reserve(q_bytes) || !out_buf_.reserve(out_bytes))))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (scratch)");
  const uint32_t* d_q = queries;
  int64_t* d_ids = ids;
  int32_t* d_dist = dist;
  int32_t* d_cnt = counts;
  if (!dev) {
    HIP_TRY(hipMemcpyAsync(q_buf_.p, queries, q_bytes, hipMemcpyHostToDevice, stream_));
    d_q = q_buf_.as<uint32_t>();
    d_ids = out_buf_.as<int64_t>();
    d_dist = reinterpret_cast<int32_t*>(out_buf_.as<char>() + ids_bytes);
    d_cnt = reinterpret_cast<int32_t*>(out_buf_.as<char>() + ids_bytes + dist_bytes);
  }
  std::memset(&stats_, 0, sizeof(stats_));
  u64* run_keys = run_buf_.as<u64>();
  HIP_TRY(hipEventRecord(ev0_, stream_));
  stats_.main_kernel_rows = n;
  stats_.main_kernel_queries = nq;
  stats_.main_kernel_bits = 1;
  stats_.dist_evals = n * nq;
  if (n > 0) {
    BinaryScanArgs a;
    a.rows = rows_;
    a.n = n;
    a.stride = stride_;
    a.W = (int)W_;
    a.tail_mask = binary_tail_mask(dim_);
    a.vec = (stride_ % 4 == 0) && ((reinterpret_cast<uintptr_t>(rows_) & 15) == 0);
    a.queries = d_q;
    a.nq = nq;
    a.k = k;
    a.deleted = d_deleted_;
    a.plan = plan;
    a.partial = partial_buf_.as<u64>();
    HIP_TRY(hipEventRecord(evk0_, stream_));
    launch_binary_scan(a, stream_);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    launch_merge_lists(a.partial, (int)(plan.slices * k), k, nq, run_keys, false, stream_);
    stats_.main_kernel_launches = plan.launches;
  } else {
    launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
  }
  launch_binary_finalize(run_keys, nq, k, id_base_, id_stride_, d_ids, d_dist, d_cnt, stream_);
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

int32_t BinaryIndex::last_stats(eps_search_stats* out) {
  eps_search_stats s = stats_;
  if (ev0_ && s.main_kernel_queries > 0 && hipEventSynchronize(ev1_) == hipSuccess) {   // (read lazily: the caller may have left the work in flight)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) s.kernel_ms = ms;
    if (s.main_kernel_launches > 0 && hipEventElapsedTime(&ms, evk0_, evk1_) == hipSuccess) s.main_kernel_ms = ms;
  }
  (void)hipGetLastError();
  *out = s;
  return EPS_OK;
}

}  // namespace eps
