// Host side of the sparse-vector index (eps_sparse_index_*, see index.hpp; limits, checks and the launch plan: sparse_host.hpp; kernels: sparse.hip;
// the inverted lists: sparse_inv_host.hpp, sparse_inverted.hip).
#include "index.hpp"

#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace eps {

SparseIndex::~SparseIndex() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t e : {ev0_, ev1_, evk0_, evk1_})
    if (e) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int32_t SparseIndex::hip_fail(hipError_t e, const char* what) {
  (void)hipGetLastError();
  return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

int32_t SparseIndex::init() {   // (Index::init's rules)
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
  if (!verdict_buf_.reserve(sizeof(SparseVerdict))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "out of device memory");
  return EPS_OK;
}

int32_t SparseIndex::set_stream(void* s) {
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

int32_t SparseIndex::synchronize() {
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

void SparseIndex::Table::swap(Table& o) {
  std::swap(off_buf.p, o.off_buf.p);
  std::swap(off_buf.cap, o.off_buf.cap);
  std::swap(idx_buf.p, o.idx_buf.p);
  std::swap(idx_buf.cap, o.idx_buf.cap);
  std::swap(val_buf.p, o.val_buf.p);
  std::swap(val_buf.cap, o.val_buf.cap);
  std::swap(norms.p, o.norms.p);
  std::swap(norms.cap, o.norms.cap);
  std::swap(offsets, o.offsets);
  std::swap(indices, o.indices);
  std::swap(values, o.values);
  std::swap(n, o.n);
  std::swap(nnz, o.nnz);
  std::swap(longest, o.longest);
}

int32_t SparseIndex::validate(const char* who, const char* what, const int64_t* d_off, const int32_t* d_idx, const float* d_val, int64_t n, int64_t nnz,
                              float* norms, int64_t* longest) {
  SparseVerdict v{~0ull, 0ull};
  HIP_TRY(hipMemcpyAsync(verdict_buf_.p, &v, sizeof(v), hipMemcpyHostToDevice, stream_));
  SparseValidateArgs a;
  a.offsets = d_off;
  a.indices = d_idx;
  a.values = d_val;
  a.n = n;
  a.nnz = nnz;
  a.dim = dim_;
  a.norms = norms;
  a.verdict = verdict_buf_.as<SparseVerdict>();
  launch_sparse_validate(a, stream_);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&v, verdict_buf_.p, sizeof(v), hipMemcpyDeviceToHost, stream_));
  HIP_TRY(hipStreamSynchronize(stream_));
  if (v.first_bad != ~0ull)
    return fail(EPS_USER_ERROR, std::string(who) + ": " + what + " " + std::to_string((long long)(v.first_bad >> 3)) + ": " + sparse_bad_text((int32_t)(v.first_bad & 7)));
  if (longest) *longest = (int64_t)v.longest;
  return EPS_OK;
}

int32_t SparseIndex::attach_csr(const int64_t* offsets, const int32_t* indices, const float* values, int64_t n) {
  if (n < 0) return fail(EPS_USER_ERROR, "attach_csr: n must be >= 0");
  if (n > SPARSE_MAX_ROWS) return fail(EPS_USER_ERROR, "attach_csr: more than 2^31 - 1 rows per index");
  if (!offsets) return fail(EPS_USER_ERROR, "attach_csr: offsets is null (n + 1 entries, offsets[0] = 0)");
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));   // (no search of the previous table is in flight when its arrays go)
  const bool dev = is_device_ptr(offsets);
  int64_t nnz = 0;
  if (dev) HIP_TRY(hipMemcpy(&nnz, offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost));   // the one value read back: it sizes the other two arrays
  else nnz = offsets[n];
  if (nnz < 0) return fail(EPS_USER_ERROR, "attach_csr: offsets[n] must be >= 0");
  if (n == 0 && nnz != 0) return fail(EPS_USER_ERROR, std::string("attach_csr: row 0: ") + sparse_bad_text(SPARSE_BAD_FIRST));
  if (nnz > 0) {
    if (!indices || !values) return fail(EPS_USER_ERROR, "attach_csr: null buffer");
    if (is_device_ptr(indices) != dev || is_device_ptr(values) != dev)
      return fail(EPS_USER_ERROR, "attach_csr: offsets, indices and values must all be host or all be device arrays");
  }
  Table t;
  t.n = n;
  t.nnz = nnz;
  if (!t.norms.reserve((size_t)(n > 0 ? n : 1) * sizeof(float))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_csr: out of device memory");
  if (dev) {
    t.offsets = offsets;
    t.indices = indices;
    t.values = values;
  } else {
    const size_t ob = (size_t)(n + 1) * sizeof(int64_t), ib = (size_t)nnz * sizeof(int32_t), vb = (size_t)nnz * sizeof(float);
    if (!t.off_buf.reserve(ob) || !t.idx_buf.reserve(ib ? ib : 16) || !t.val_buf.reserve(vb ? vb : 16))
      return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_csr: out of device memory");
    HIP_TRY(hipMemcpyAsync(t.off_buf.p, offsets, ob, hipMemcpyHostToDevice, stream_));
    if (ib) HIP_TRY(hipMemcpyAsync(t.idx_buf.p, indices, ib, hipMemcpyHostToDevice, stream_));
    if (vb) HIP_TRY(hipMemcpyAsync(t.val_buf.p, values, vb, hipMemcpyHostToDevice, stream_));
    t.offsets = t.off_buf.as<int64_t>();
    t.indices = t.idx_buf.as<int32_t>();
    t.values = t.val_buf.as<float>();
  }
  // the table becomes visible to a search only after the device pass found it well-formed; a refused table leaves the previous one in place
  const int32_t rc = validate("attach_csr", "row", t.offsets, t.indices, t.values, n, nnz, t.norms.as<float>(), &t.longest);
  if (rc != EPS_OK) return rc;
  t_.swap(t);
  d_deleted_ = nullptr;   // a new table: the bitset of the previous one is forgotten
  inv_.release();         // ... and its inverted lists
  return EPS_OK;
}

int32_t SparseIndex::set_id_map(int64_t base, int64_t stride) {
  if (stride <= 0) return fail(EPS_USER_ERROR, "set_id_map: stride must be positive");
  id_base_ = base;
  id_stride_ = stride;
  return EPS_OK;
}

int32_t SparseIndex::set_deleted(const uint8_t* bits, int64_t nbytes) {
  HIP_TRY(hipSetDevice(device_));
  if (!bits || nbytes <= 0) {
    d_deleted_ = nullptr;
    return EPS_OK;
  }
  if (nbytes < (t_.n + 7) / 8) return fail(EPS_USER_ERROR, "set_deleted: bitset shorter than ceil(rows/8) bytes");
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

int32_t SparseIndex::search(const int64_t* q_offsets, const int32_t* q_indices, const float* q_values, int64_t nq, int32_t k, int64_t* ids, float* dist,
                            int32_t* counts) {
  if (k < 1 || k > SPARSE_MAX_K) return fail(EPS_USER_ERROR, "search: k must be in [1, 1024]");
  if (nq < 0) return fail(EPS_USER_ERROR, "search: nq must be >= 0");
  if (nq == 0) return EPS_OK;
  if (nq > SPARSE_MAX_ROWS) return fail(EPS_USER_ERROR, "search: more than 2^31 - 1 queries");
  HIP_TRY(hipSetDevice(device_));
  if (!q_offsets || !ids || !dist) return fail(EPS_USER_ERROR, "search: null buffer");
  if (is_device_ptr(q_offsets)) return fail(EPS_USER_ERROR, "search: q_offsets must be a host array");
  int64_t qnnz = 0, longest = 0, bad = -1;
  int32_t kind = 0;
  if (sparse_offsets_check(q_offsets, nq, &qnnz, &longest, &bad, &kind) != EPS_OK)
    return fail(EPS_USER_ERROR, "search: query " + std::to_string((long long)bad) + ": " + sparse_bad_text(kind));
  if (longest > SPARSE_MAX_QUERY_NNZ) {
    int64_t j = 0;
    while (q_offsets[j + 1] - q_offsets[j] <= SPARSE_MAX_QUERY_NNZ) ++j;
    return fail(EPS_DB_UNSUPPORTED_ERROR, "search: query " + std::to_string((long long)j) + " has " + std::to_string((long long)(q_offsets[j + 1] - q_offsets[j])) +
                                              " non-zeros; at most " + std::to_string((long long)SPARSE_MAX_QUERY_NNZ) + " per query are supported");
  }
  bool q_dev = false;
  if (qnnz > 0) {
    if (!q_indices || !q_values) return fail(EPS_USER_ERROR, "search: null buffer");
    q_dev = is_device_ptr(q_indices);
    if (is_device_ptr(q_values) != q_dev) return fail(EPS_USER_ERROR, "search: q_indices and q_values must both be host or both be device arrays");
  }
  const bool out_dev = is_device_ptr(ids);
  if (out_dev != is_device_ptr(dist) || (counts && out_dev != is_device_ptr(counts)))
    return fail(EPS_USER_ERROR, "search: ids_out, dist_out and counts_out must all be host or all be device pointers");
  if (!q_dev && qnnz > 0 && sparse_rows_check(q_offsets, q_indices, nq, dim_, &bad, &kind) != EPS_OK)
    return fail(EPS_USER_ERROR, "search: query " + std::to_string((long long)bad) + ": " + sparse_bad_text(kind));

  // ---- scratch: [q_offsets | a host batch's indices | values], partial lists, result keys, host results' device block
  const int64_t n = t_.n;
  const bool inverted = inv_.built;   // (build_inverted refuses EUCLIDEAN; drop_inverted sends the handle back to the scan)
  const SparseInvPlan iplan = sparse_inv_plan(n, nq, k, longest);
  const SparsePlan plan = inverted ? iplan.rows : sparse_plan(n, nq, k, longest);
  const size_t off_bytes = (size_t)(nq + 1) * sizeof(int64_t), el_bytes = q_dev ? 0 : (size_t)qnnz * 4;
  const size_t ids_bytes = (size_t)nq * k * sizeof(int64_t), dist_bytes = (size_t)nq * k * sizeof(float), out_bytes = ids_bytes + dist_bytes + (size_t)nq * sizeof(int32_t);
  HIP_TRY(hipStreamSynchronize(stream_));   // (the previous call's staging is read; its pageable copies are complete)
  if (!q_buf_.reserve(off_bytes + 2 * el_bytes + 16) || !partial_buf_.reserve((size_t)nq * plan.W * k * sizeof(u64)) ||
      !run_buf_.reserve((size_t)nq * k * sizeof(u64)) || (!out_dev && !out_buf_.reserve(out_bytes)))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "search: out of device memory (scratch)");
  int64_t* d_qoff = q_buf_.as<int64_t>();
  const int32_t* d_qidx = q_indices;
  const float* d_qval = q_values;
  HIP_TRY(hipMemcpyAsync(d_qoff, q_offsets, off_bytes, hipMemcpyHostToDevice, stream_));
  if (!q_dev && qnnz > 0) {
    char* base = q_buf_.as<char>() + off_bytes;
    HIP_TRY(hipMemcpyAsync(base, q_indices, el_bytes, hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipMemcpyAsync(base + el_bytes, q_values, el_bytes, hipMemcpyHostToDevice, stream_));
    d_qidx = reinterpret_cast<const int32_t*>(base);
    d_qval = reinterpret_cast<const float*>(base + el_bytes);
  }
  if (q_dev) {   // device-resident queries: one small launch, and the read of its verdict, in front of the scan
    const int32_t rc = validate("search", "query", d_qoff, d_qidx, d_qval, nq, qnnz, nullptr, nullptr);
    if (rc != EPS_OK) return rc;
  }
  std::memset(&stats_, 0, sizeof(stats_));
  u64* run_keys = run_buf_.as<u64>();
  int64_t* d_ids = ids;
  float* d_dist = dist;
  int32_t* d_cnt = counts;
  if (!out_dev) {
    d_ids = out_buf_.as<int64_t>();
    d_dist = reinterpret_cast<float*>(out_buf_.as<char>() + ids_bytes);
    d_cnt = reinterpret_cast<int32_t*>(out_buf_.as<char>() + ids_bytes + dist_bytes);
  }
  last_engine_ = inverted ? 2 : 1;
  HIP_TRY(hipEventRecord(ev0_, stream_));
  stats_.main_kernel_rows = n;
  stats_.main_kernel_queries = nq;
  stats_.main_kernel_bits = 32;
  stats_.dist_evals = n * nq;
  if (n > 0 && inverted) {
    SparseInvArgs a;
    a.col_offsets = inv_.col_offsets.as<int64_t>();
    a.postings = inv_.postings.as<SparsePosting>();
    a.norms = t_.norms.as<float>();
    a.n = n;
    a.metric = metric_;
    a.q_offsets = d_qoff;
    a.q_indices = d_qidx;
    a.q_values = d_qval;
    a.nq = nq;
    a.k = k;
    a.f = no_filter();
    a.f.deleted = d_deleted_;
    a.plan = iplan;
    a.partial = partial_buf_.as<u64>();
    HIP_TRY(hipEventRecord(evk0_, stream_));
    launch_sparse_inverted(a, stream_);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    launch_among_merge(a.partial, plan.W, k, nq, run_keys, stream_);
    stats_.main_kernel_launches = (nq + SPARSE_GRID_Y - 1) / SPARSE_GRID_Y;
  } else if (n > 0) {
    SparseScanArgs a;
    a.offsets = t_.offsets;
    a.indices = t_.indices;
    a.values = t_.values;
    a.norms = t_.norms.as<float>();
    a.n = n;
    a.metric = metric_;
    a.q_offsets = d_qoff;
    a.q_indices = d_qidx;
    a.q_values = d_qval;
    a.nq = nq;
    a.k = k;
    a.f = no_filter();
    a.f.deleted = d_deleted_;
    a.plan = plan;
    a.partial = partial_buf_.as<u64>();
    HIP_TRY(hipEventRecord(evk0_, stream_));
    launch_sparse_scan(a, stream_);
    HIP_TRY(hipEventRecord(evk1_, stream_));
    launch_among_merge(a.partial, plan.W, k, nq, run_keys, stream_);
    stats_.main_kernel_launches = (plan.tiles + SPARSE_GRID_Y - 1) / SPARSE_GRID_Y;
  } else {
    launch_fill_u64(run_keys, nq * k, KEY_EMPTY, stream_);
  }
  launch_finalize(run_keys, nq, k, id_base_, id_stride_, d_ids, d_dist, d_cnt, stream_);
  HIP_TRY(hipEventRecord(ev1_, stream_));
  HIP_TRY(hipGetLastError());
  if (!out_dev) {
    HIP_TRY(hipMemcpyAsync(ids, d_ids, ids_bytes, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(dist, d_dist, dist_bytes, hipMemcpyDeviceToHost, stream_));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, d_cnt, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
  }
  return EPS_OK;
}

// ---- the inverted lists
int32_t SparseIndex::build_inverted() {
  if (!t_.offsets) return fail(EPS_USER_ERROR, "build_inverted: no table attached");
  if (metric_ == EPS_METRIC_EUCLIDEAN)
    return fail(EPS_DB_UNSUPPORTED_ERROR, "build_inverted: EUCLIDEAN is served by the scan only: L2 adds the unmatched squares of both sides in merged order, which has no "
                                          "term-at-a-time form");
  if (dim_ > SPARSE_INV_MAX_DIM)
    return fail(EPS_DB_UNSUPPORTED_ERROR, "build_inverted: dim " + std::to_string((long long)dim_) + " is above the limit of " + std::to_string((long long)SPARSE_INV_MAX_DIM) +
                                              " columns (2^24): the column directory is dense");
  SparseInvBytes bytes;
  if (!sparse_inv_bytes(dim_, t_.nnz, &bytes)) return fail(EPS_DB_UNSUPPORTED_ERROR, "build_inverted: more than 2^40 non-zeros");
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));   // (no search on the previous image is in flight when it goes)
  inv_.release();                           // calling it twice rebuilds; a failure below leaves no image and the scan goes on answering
  Inverted im;
  DevBuf pairs, keys_a, keys_b, table;   // freed when the build ends
  const auto some = [](int64_t b) { return (size_t)(b ? b : 16); };
  if (!im.col_offsets.reserve((size_t)bytes.directory) || !im.postings.reserve(some(bytes.postings)) || !pairs.reserve(some(bytes.pairs)) ||
      !keys_a.reserve(some(bytes.keys_a)) || !keys_b.reserve(some(bytes.keys_b)) || !table.reserve((size_t)bytes.table))
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "build_inverted: out of device memory (the image costs 8 * nnz + 8 * (dim + 1) bytes, the build up to 16 * nnz more)");
  SparseInvBuildArgs a;
  a.offsets = t_.offsets;
  a.indices = t_.indices;
  a.values = t_.values;
  a.n = t_.n;
  a.nnz = t_.nnz;
  a.dim = dim_;
  a.col_offsets = im.col_offsets.as<int64_t>();
  a.postings = im.postings.as<SparsePosting>();
  a.pairs = pairs.as<SparsePosting>();
  a.keys_a = keys_a.as<int32_t>();
  a.keys_b = keys_b.as<int32_t>();
  a.table = table.as<u64>();
  a.longest = &verdict_buf_.as<SparseVerdict>()->longest;
  HIP_TRY(launch_sparse_inv_build(a, stream_));
  unsigned long long longest = 0;
  HIP_TRY(hipMemcpyAsync(&longest, a.longest, sizeof(longest), hipMemcpyDeviceToHost, stream_));
  HIP_TRY(hipStreamSynchronize(stream_));
  std::swap(inv_.col_offsets.p, im.col_offsets.p);
  std::swap(inv_.col_offsets.cap, im.col_offsets.cap);
  std::swap(inv_.postings.p, im.postings.p);
  std::swap(inv_.postings.cap, im.postings.cap);
  inv_.built = true;
  inv_.nnz = t_.nnz;
  inv_.longest = (int64_t)longest;
  return EPS_OK;
}

int32_t SparseIndex::drop_inverted() {
  if (!inv_.built) return EPS_OK;
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  inv_.release();
  return EPS_OK;
}

int32_t SparseIndex::inverted_info(int64_t* columns, int64_t* postings, int64_t* longest_column, int32_t* last_engine) const {
  if (columns) *columns = inv_.built ? dim_ : 0;   // entries of the directory; 0: no image
  if (postings) *postings = inv_.nnz;
  if (longest_column) *longest_column = inv_.longest;
  if (last_engine) *last_engine = last_engine_;
  return EPS_OK;
}

int32_t SparseIndex::get_inverted(int64_t* col_offsets, int32_t* rows, float* values) {
  if (!inv_.built) return fail(EPS_USER_ERROR, "get_inverted: no inverted lists (build_inverted first)");
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  if (col_offsets) HIP_TRY(hipMemcpy(col_offsets, inv_.col_offsets.p, (size_t)(dim_ + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rows || values) && inv_.nnz > 0) {
    std::vector<SparsePosting> host((size_t)inv_.nnz);
    HIP_TRY(hipMemcpy(host.data(), inv_.postings.p, host.size() * sizeof(SparsePosting), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < host.size(); ++i) {
      if (rows) rows[i] = host[i].row;
      if (values) values[i] = host[i].value;
    }
  }
  return EPS_OK;
}

int32_t SparseIndex::last_stats(eps_search_stats* out) {
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
