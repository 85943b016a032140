// The C ABI of libepsilla_gfx950 (include/epsilla_gfx950.h): argument checks, dispatch to IndexBase / Index, and no exception across it.
#include "index.hpp"

#include <cstdio>
#include <new>
#include <string>

using eps::Index;
using eps::IndexBase;

// No C++ exception crosses the C ABI: allocation failures and anything else thrown below map to the reference's
// status codes (utils/error.hpp:11-41) with the text in eps_index_last_error.
static int32_t map_exception(IndexBase* ix) {
  try {
    throw;
  } catch (const std::bad_alloc&) {
    return ix ? ix->fail(EPS_INFRA_UNEXPECTED_ERROR, "out of host memory") : EPS_INFRA_UNEXPECTED_ERROR;
  } catch (const std::exception& e) {
    return ix ? ix->fail(EPS_DB_UNEXPECTED_ERROR, std::string("unexpected: ") + e.what()) : EPS_DB_UNEXPECTED_ERROR;
  } catch (...) {
    return ix ? ix->fail(EPS_DB_UNEXPECTED_ERROR, "unexpected exception") : EPS_DB_UNEXPECTED_ERROR;
  }
}
#define IX(h) reinterpret_cast<IndexBase*>(h)
#define CIX(h) reinterpret_cast<const IndexBase*>(h)
#define GUARD(h, expr)             \
  do {                             \
    if (!(h)) return EPS_USER_ERROR; \
    try {                          \
      return (expr);               \
    } catch (...) {                \
      return map_exception(IX(h)); \
    }                              \
  } while (0)
// The entries that only a single-device index serves: `f(Index&)` runs with the index's device current; a sharded handle is refused with the
// entry's own text and error class.
template <class F>
static int32_t on_single_device(eps_index* h, const char* refusal, int32_t err_class, F&& f) {
  if (!h) return EPS_USER_ERROR;
  Index* ix = dynamic_cast<Index*>(IX(h));
  if (!ix) return IX(h)->fail(EPS_DB_UNSUPPORTED_ERROR, refusal, err_class);
  try {
    if (hipSetDevice(ix->device_) != hipSuccess) return ix->fail(EPS_INFRA_UNEXPECTED_ERROR, "hipSetDevice");
    return f(*ix);
  } catch (...) {
    return map_exception(ix);
  }
}

// A sparse-vector handle (eps_sparse_index): the same rule - no exception crosses the ABI, the text stays in the handle.
#define SIX(h) reinterpret_cast<eps::SparseIndex*>(h)
template <class F>
static int32_t on_sparse(eps_sparse_index* h, F&& f) {
  if (!h) return EPS_USER_ERROR;
  eps::SparseIndex* ix = SIX(h);
  try {
    return f(*ix);
  } catch (const std::bad_alloc&) {
    return ix->fail(EPS_INFRA_UNEXPECTED_ERROR, "out of host memory");
  } catch (const std::exception& e) {
    return ix->fail(EPS_DB_UNEXPECTED_ERROR, std::string("unexpected: ") + e.what());
  } catch (...) {
    return ix->fail(EPS_DB_UNEXPECTED_ERROR, "unexpected exception");
  }
}

// The merges have no handle to keep a message in: a refusal names its reason on stderr, as a failed eps_index_create does.
static int32_t merge_refused(const char* entry, const char* why, int32_t rc) {
  std::fprintf(stderr, "%s: %s\n", entry, why);
  return rc;
}
// what merge_host.hpp's staging runs on: the current device, one stream
struct HipMergeDev {
  hipStream_t s;
  bool is_device(const void* p) { return eps::is_device_ptr(p); }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    return p;
  }
  void free(void* p) { (void)hipFree(p); }
  bool h2d(void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess; }
  bool d2h(void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) == hipSuccess; }
  void launch(const eps::MergeRankArgs& a) { eps::launch_merge_rank(a, s); }
  bool sync() { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }
};

extern "C" {

void eps_default_search_params(eps_search_params* p) {
  if (!p) return;
  p->mode = EPS_MODE_REFERENCE;
  p->flat_engine = EPS_FLAT_AUTO;
  p->prefilter = 0;         // Config::PreFilter{false}
  p->intra_threads = 4;     // Config::IntraQueryThreads{4}      (config/config.hpp:18)
  p->master_queue = 500;    // Config::MasterQueueSize{500}      (:19)
  p->local_queue = 500;     // Config::LocalQueueSize{500}       (:20)
  p->sync_interval = 15;    // Config::GlobalSyncInterval{15}    (:21)
  p->filter_in_traversal = 0;
  p->reserved = 0;
}

void eps_default_build_params(eps_build_params* p) {
  if (!p) return;
  p->search_length = 45;  // NSGConfig(45, 50, 300, 100), db/ann_graph_segment.cpp:29
  p->out_degree = 50;
  p->candidate_pool_size = 300;
  p->knng = 100;
  p->seed = 100;  // nsg.cpp:19
  p->reserved = 0;
}

int32_t eps_index_create(int64_t dim, int32_t metric, int32_t device, eps_index** out) {
  if (!out) return EPS_USER_ERROR;
  *out = nullptr;
  if (dim <= 0 || dim > 8192 || metric < 0 || metric > 2) return EPS_USER_ERROR;  // one query must fit in LDS next to the queues
  try {
    Index* ix = new Index(dim, metric, device);
    const int32_t rc = ix->init();
    if (rc != EPS_OK) {
      std::fprintf(stderr, "eps_index_create: %s\n", ix->last_error());
      delete ix;
      return rc;
    }
    *out = reinterpret_cast<eps_index*>(static_cast<IndexBase*>(ix));
    return EPS_OK;
  } catch (...) {
    return map_exception(nullptr);
  }
}
int32_t eps_index_create_sharded(int64_t dim, int32_t metric, const int32_t* devices, int32_t shards, eps_index** out) {
  if (!out) return EPS_USER_ERROR;
  *out = nullptr;
  if (dim <= 0 || dim > 8192 || metric < 0 || metric > 2 || !devices || shards <= 0 || shards > 16) return EPS_USER_ERROR;
  try {
    std::string err;
    IndexBase* g = eps::make_shard_group(dim, metric, devices, shards, &err);
    if (!g) {
      std::fprintf(stderr, "eps_index_create_sharded: %s\n", err.c_str());
      return EPS_INFRA_UNEXPECTED_ERROR;
    }
    *out = reinterpret_cast<eps_index*>(g);
    return EPS_OK;
  } catch (...) {
    return map_exception(nullptr);
  }
}
int32_t eps_index_destroy(eps_index* h) {
  try {
    delete reinterpret_cast<IndexBase*>(h);
    return EPS_OK;
  } catch (...) {
    return map_exception(nullptr);
  }
}
const char* eps_index_last_error(const eps_index* h) { return h ? CIX(h)->last_error() : "null handle"; }
int32_t eps_index_last_error_class(const eps_index* h) { return h ? CIX(h)->last_error_class() : EPS_ERRCLASS_OTHER; }
int32_t eps_index_set_stream(eps_index* h, void* s) { GUARD(h, IX(h)->set_stream(s)); }
int32_t eps_index_synchronize(eps_index* h) { GUARD(h, IX(h)->synchronize()); }
int32_t eps_index_attach_rows(eps_index* h, const float* rows, int64_t n) { GUARD(h, IX(h)->attach_rows(rows, n)); }
int32_t eps_index_append_rows(eps_index* h, const float* rows, int64_t n) { GUARD(h, IX(h)->append_rows(rows, n)); }
int32_t eps_index_attach_shard_rows(eps_index* h, int32_t shard, const float* rows, int64_t n_local) { GUARD(h, IX(h)->attach_shard_rows(shard, rows, n_local)); }
int32_t eps_index_clone_rows(eps_index* dst, eps_index* src, int64_t n) {
  if (!src) return EPS_USER_ERROR;
  GUARD(dst, IX(dst)->clone_rows(*IX(src), n));
}
int64_t eps_index_row_count(const eps_index* h) { return h ? CIX(h)->row_count() : -1; }
int32_t eps_index_set_id_map(eps_index* h, int64_t b, int64_t s) { GUARD(h, IX(h)->set_id_map(b, s)); }
int32_t eps_index_set_deleted(eps_index* h, const uint8_t* bits, int64_t nbytes) { GUARD(h, IX(h)->set_deleted(bits, nbytes)); }
int32_t eps_index_set_int_filter(eps_index* h, const void* col, int64_t stride, int32_t width, int32_t op, int64_t c) {
  GUARD(h, IX(h)->set_int_filter(col, stride, width, op, c));
}
int32_t eps_index_set_filter_program(eps_index* h, const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride, int64_t n_rows) {
  GUARD(h, IX(h)->set_filter_program(ops, nops, rows, stride, n_rows, 0));
}
int32_t eps_index_set_filter_program_ex(eps_index* h, const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride, int64_t n_rows,
                                        int32_t flags) {
  GUARD(h, IX(h)->set_filter_program(ops, nops, rows, stride, n_rows, flags));
}
int32_t eps_index_search_walk(eps_index* h, const float* q, int64_t nq, int32_t limit, int32_t cap, const eps_search_params* p, int64_t* ids,
                              float* dist, int32_t* counts) {
  if (limit <= 0 || cap < limit) return EPS_USER_ERROR;
  GUARD(h, IX(h)->search(q, nq, cap, p, ids, dist, counts, limit));
}
int32_t eps_index_select_edges(eps_index* h, const int64_t* nodes, int64_t m, const int64_t* cands, int32_t cands_per_node, int32_t depth,
                               int32_t out_degree, int64_t* out_ids, int32_t* out_deg) {
  return on_single_device(h, "select_edges: single-device indices only", EPS_ERRCLASS_OTHER, [&](Index& ix) {
    return eps::select_edges(ix, nodes, m, cands, cands_per_node, depth, out_degree, out_ids, out_deg);
  });
}
int32_t eps_index_inter_insert(eps_index* h, const int64_t* ids, const int32_t* deg, int64_t n, int32_t out_degree, int64_t* out_ids,
                               int32_t* out_deg) {
  return on_single_device(h, "inter_insert: single-device indices only", EPS_ERRCLASS_OTHER,
                          [&](Index& ix) { return eps::inter_insert(ix, ids, deg, n, out_degree, out_ids, out_deg); });
}
int32_t eps_index_knn_graph(eps_index* h, int64_t n, const eps_build_params* p, int64_t* out_ids) {
  if (!out_ids) return EPS_USER_ERROR;
  return on_single_device(h, "knn_graph: single-device indices only", EPS_ERRCLASS_OTHER, [&](Index& ix) {
    if (n < 2 || n > ix.row_count()) return ix.fail(EPS_USER_ERROR, "knn_graph: n must be in [2, rows]");
    eps::BuildStage st;
    st.stop_after = 1;
    st.out_ids = out_ids;
    return eps::graph_build(ix, n, eps::build_params_or_default(p), &st);
  });
}
int32_t eps_index_link(eps_index* h, int64_t n, const int64_t* knn, int64_t navigation_point, const eps_build_params* p, int64_t* out_ids,
                       int32_t* out_deg, int64_t* nav_out) {
  if (!out_ids || !out_deg) return EPS_USER_ERROR;
  return on_single_device(h, "link: single-device indices only", EPS_ERRCLASS_OTHER, [&](Index& ix) {
    if (n < 2 || n > ix.row_count()) return ix.fail(EPS_USER_ERROR, "link: n must be in [2, rows]");
    eps::BuildStage st;
    st.knn_in = knn;
    st.nav_in = navigation_point;
    st.stop_after = 2;
    st.out_ids = out_ids;
    st.out_deg = out_deg;
    st.nav_out = nav_out;
    return eps::graph_build(ix, n, eps::build_params_or_default(p), &st);
  });
}
int32_t eps_index_mirror_view(eps_index* h, int32_t bits, const float* queries, int64_t nq, eps_mirror_view* view) {
  if (!view) return EPS_USER_ERROR;
  return on_single_device(h, "mirror_view: single-device indices only", EPS_ERRCLASS_OTHER,
                          [&](Index& ix) { return eps::flat_mirror_view(ix, bits, queries, nq, view); });
}
int32_t eps_index_filter_pass(eps_index* h, const float* queries, int64_t nq, int32_t bits, int64_t row_lo, int64_t row_hi, int64_t cap, int32_t mode,
                              int32_t thr_form, const void* thr, void* T_out, uint32_t* cnt_out, void* cand_out) {
  return on_single_device(h, "filter_pass: single-device indices only", EPS_ERRCLASS_OTHER, [&](Index& ix) {
    return eps::flat_filter_pass(ix, queries, nq, bits, row_lo, row_hi, cap, mode, thr_form, thr, T_out, cnt_out, cand_out);
  });
}
int32_t eps_index_one_pass_probe(eps_index* h, const float* queries, int64_t nq, int32_t k, eps_one_pass_form* form, uint32_t* raw_cnt, uint64_t* raw,
                                 int32_t* table, float* qstat, int32_t* kth, int32_t* T_final) {
  return on_single_device(h, "one_pass_probe: single-device indices only", EPS_ERRCLASS_OTHER, [&](Index& ix) {
    return eps::one_pass_probe(ix, queries, nq, k, form, raw_cnt, reinterpret_cast<eps::u64*>(raw), table, qstat, kth, T_final);
  });
}
int32_t eps_index_load_table(eps_index* h, const char* path, const eps_table_layout* layout, int64_t* n_out) {
  return on_single_device(h, "load_table: single-device indices only", EPS_ERRCLASS_OTHER, [&](Index& ix) { return ix.load_table(path, layout, n_out); });
}
int32_t eps_index_build(eps_index* h, int64_t n, const eps_build_params* p) { GUARD(h, IX(h)->build(n, p)); }
int32_t eps_index_set_graph(eps_index* h, int64_t n, const int64_t* off, const int64_t* nbr, int64_t nav) {
  GUARD(h, IX(h)->set_graph(n, off, nbr, nav));
}
int32_t eps_index_graph_info(const eps_index* h, int64_t* n, int64_t* e, int64_t* nav) { return h ? CIX(h)->graph_info(n, e, nav) : EPS_USER_ERROR; }
int32_t eps_index_get_graph(const eps_index* h, int64_t* off, int64_t* nbr) { return h ? CIX(h)->get_graph(off, nbr) : EPS_USER_ERROR; }
int32_t eps_index_save_graph(eps_index* h, const char* path) { GUARD(h, IX(h)->save_graph(path)); }
int32_t eps_index_load_graph(eps_index* h, const char* path) { GUARD(h, IX(h)->load_graph(path)); }
int32_t eps_index_search(eps_index* h, const float* q, int64_t nq, int32_t k, const eps_search_params* p, int64_t* ids,
                         float* dist, int32_t* counts) {
  GUARD(h, IX(h)->search(q, nq, k, p, ids, dist, counts));
}
int32_t eps_index_select(eps_index* h, int64_t skip, int64_t limit, int64_t* ids_out, int64_t* count_out, int64_t* total_out) {
  return on_single_device(h, "select: single-device indices only (a sharded table is not served)", EPS_ERRCLASS_OTHER,
                          [&](Index& ix) { return ix.select(skip, limit, ids_out, count_out, total_out); });
}
int32_t eps_index_search_range(eps_index* h, const float* q, int64_t nq, const float* radius, int32_t cap, const eps_search_params* p, int64_t* ids,
                               float* dist, int32_t* counts, int64_t* totals) {
  return on_single_device(h, "search_range: single-device indices only (a sharded table is not served)", EPS_ERRCLASS_OTHER,
                          [&](Index& ix) { return ix.search_range(q, nq, radius, cap, p, ids, dist, counts, totals); });
}
int32_t eps_index_search_among(eps_index* h, const float* q, int64_t nq, const int64_t* cand_ids, const int64_t* cand_offsets, int64_t n_cand, int32_t k,
                               int64_t* ids, float* dist, int32_t* counts) {
  return on_single_device(h, "search_among: single-device indices only (a sharded table is not served)", EPS_ERRCLASS_OTHER,
                          [&](Index& ix) { return ix.search_among(q, nq, cand_ids, cand_offsets, n_cand, k, ids, dist, counts); });
}
int32_t eps_index_set_groups(eps_index* h, const int64_t* keys, int64_t n) { GUARD(h, IX(h)->set_groups(keys, n)); }
int32_t eps_index_search_groups(eps_index* h, const float* q, int64_t nq, int32_t k, const eps_search_params* p, int32_t engine, int32_t page_rows,
                                int64_t scratch_bytes, int64_t* ids, float* dist, int64_t* group_keys, int32_t* counts) {
  GUARD(h, IX(h)->search_groups(q, nq, k, p, engine, page_rows, scratch_bytes, ids, dist, group_keys, counts));
}
int32_t eps_index_search_group_rows(eps_index* h, const float* q, int64_t nq, int32_t k, int32_t m, const eps_search_params* p, int32_t engine, int32_t page_rows,
                                    int64_t scratch_bytes, int64_t* ids, float* dist, int64_t* group_keys, int32_t* row_counts, int64_t* group_sizes,
                                    int32_t* counts) {
  GUARD(h, IX(h)->search_group_rows(q, nq, k, m, p, engine, page_rows, scratch_bytes, ids, dist, group_keys, row_counts, group_sizes, counts));
}
int32_t eps_index_search_multi(eps_index* h, const float* vectors, const int64_t* q_offsets, int64_t nq, const int64_t* cand_keys, const int64_t* cand_offsets,
                               int64_t n_cand, int32_t k, int64_t scratch_bytes, int64_t* group_keys, float* score, int32_t* counts, int64_t* match_ids,
                               float* match_dist) {
  GUARD(h, IX(h)->search_multi(vectors, q_offsets, nq, cand_keys, cand_offsets, n_cand, k, scratch_bytes, group_keys, score, counts, match_ids, match_dist));
}
int32_t eps_index_search_diverse(eps_index* h, const float* queries, int64_t nq, int32_t k, int32_t fetch_k, float lambda, const int64_t* cand_ids,
                                 const int64_t* cand_offsets, int64_t n_cand, const eps_search_params* p, int64_t* ids, float* dist, float* score,
                                 int32_t* counts) {
  GUARD(h, IX(h)->search_diverse(queries, nq, k, fetch_k, lambda, cand_ids, cand_offsets, n_cand, p, ids, dist, score, counts));
}
int32_t eps_index_groups_info(eps_index* h, int64_t* n_groups, int64_t* largest_group, int32_t* last_engines, int64_t* last_scan_queries) {
  GUARD(h, IX(h)->groups_info(n_groups, largest_group, last_engines, last_scan_queries));
}
int32_t eps_index_last_stats(const eps_index* h, eps_search_stats* out) {
  if (!h || !out) return EPS_USER_ERROR;
  return const_cast<IndexBase*>(CIX(h))->last_stats(out);
}
int32_t eps_index_kernel_times(eps_index* h, double* ms_out, int32_t cap) { return h ? IX(h)->kernel_times(ms_out, cap) : 0; }

int32_t eps_normalize_rows(float* rows, int64_t n, int64_t dim, int32_t only_if_nonzero, int32_t device, void* stream) {
  if (n < 0 || dim <= 0 || (n > 0 && !rows)) return EPS_USER_ERROR;
  if (n == 0) return EPS_OK;
  if (hipSetDevice(device) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (eps::is_device_ptr(rows)) {
    eps::launch_normalize(rows, n, (int)dim, only_if_nonzero != 0, s);
    return hipGetLastError() == hipSuccess ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
  }
  float* d = nullptr;
  const size_t bytes = (size_t)n * dim * sizeof(float);
  if (hipMalloc(&d, bytes) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  bool ok = hipMemcpyAsync(d, rows, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  if (ok) eps::launch_normalize(d, n, (int)dim, only_if_nonzero != 0, s);
  ok = ok && hipMemcpyAsync(rows, d, bytes, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  (void)hipFree(d);
  return ok ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

int32_t eps_merge_topk(const float* dist, const int64_t* ids, int32_t shards, int64_t nq, int32_t k, float* out_dist,
                       int64_t* out_ids, int32_t device, void* stream) {
  if (!dist || !ids || !out_dist || !out_ids || shards <= 0 || shards > 16 || nq < 0 || k <= 0) return EPS_USER_ERROR;
  if (nq == 0) return EPS_OK;
  if (hipSetDevice(device) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool dev = eps::is_device_ptr(dist);
  if (dev != eps::is_device_ptr(ids) || dev != eps::is_device_ptr(out_dist) || dev != eps::is_device_ptr(out_ids)) return EPS_USER_ERROR;
  if (dev) {
    eps::launch_merge_shards(dist, ids, shards, nq, k, out_dist, out_ids, s);
    return hipGetLastError() == hipSuccess ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
  }
  const size_t in_n = (size_t)shards * nq * k, out_n = (size_t)nq * k;
  char* d = nullptr;
  if (hipMalloc(&d, in_n * 12 + out_n * 12 + 64) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  int64_t* d_ids = reinterpret_cast<int64_t*>(d);
  int64_t* d_oids = d_ids + in_n;
  float* d_dist = reinterpret_cast<float*>(d_oids + out_n);
  float* d_odist = d_dist + in_n;
  bool ok = hipMemcpyAsync(d_ids, ids, in_n * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
            hipMemcpyAsync(d_dist, dist, in_n * 4, hipMemcpyHostToDevice, s) == hipSuccess;
  if (ok) eps::launch_merge_shards(d_dist, d_ids, shards, nq, k, d_odist, d_oids, s);
  ok = ok && hipMemcpyAsync(out_ids, d_oids, out_n * 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
       hipMemcpyAsync(out_dist, d_odist, out_n * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
       hipStreamSynchronize(s) == hipSuccess;
  (void)hipFree(d);
  return ok ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

// the same merge over ONE gathered buffer: shard s contributed `shard_stride_bytes` bytes holding int64 ids[nq][k] at
// offset 0 and float dist[nq][k] at `dist_offset_bytes` (what a single all-gather of a packed per-rank buffer delivers)
int32_t eps_merge_topk_packed(const void* gathered, int64_t shard_stride_bytes, int64_t dist_offset_bytes, int32_t shards, int64_t nq,
                              int32_t k, float* out_dist, int64_t* out_ids, int32_t device, void* stream) {
  if (!gathered || !out_dist || !out_ids || shards <= 0 || shards > 16 || nq < 0 || k <= 0) return EPS_USER_ERROR;
  if (shard_stride_bytes < dist_offset_bytes + nq * k * 4 || dist_offset_bytes < nq * k * 8 || (dist_offset_bytes & 3) || (shard_stride_bytes & 7))
    return EPS_USER_ERROR;
  if (nq == 0) return EPS_OK;
  if (!eps::is_device_ptr(gathered) || !eps::is_device_ptr(out_dist) || !eps::is_device_ptr(out_ids)) return EPS_USER_ERROR;
  if (hipSetDevice(device) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  const char* base = static_cast<const char*>(gathered);
  eps::launch_merge_shards(reinterpret_cast<const float*>(base + dist_offset_bytes), reinterpret_cast<const int64_t*>(base), shards, nq, k,
                           out_dist, out_ids, static_cast<hipStream_t>(stream), shard_stride_bytes);
  return hipGetLastError() == hipSuccess ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

// ---- the merges of radius answers and ordered selects (merge_lists.hip; checks and host staging: merge_host.hpp)
int32_t eps_merge_range(const int64_t* ids, const float* dist, const int32_t* counts, const int64_t* totals, int32_t shards, int64_t nq, int32_t cap,
                        int64_t* out_ids, float* out_dist, int32_t* out_counts, int64_t* out_totals, int32_t device, void* stream) {
  const char* why;
  const int32_t rc = eps::merge_range_check(shards, nq, cap, &why);
  if (rc != EPS_OK) return merge_refused("eps_merge_range", why, rc);
  if (nq == 0) return EPS_OK;
  if (!ids || !dist || !counts || !totals || !out_ids || !out_dist) return merge_refused("eps_merge_range", "null pointer", EPS_USER_ERROR);
  if (hipSetDevice(device) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  HipMergeDev dev{static_cast<hipStream_t>(stream)};
  const void* ptrs[] = {ids, dist, counts, totals, out_ids, out_dist, out_counts, out_totals};
  const int side = eps::merge_side(dev, ptrs, 8);
  if (side < 0) return merge_refused("eps_merge_range", "lists and results must all be host or all be device buffers", EPS_USER_ERROR);
  if (side == 0) return eps::merge_range_host(dev, ids, dist, counts, totals, shards, nq, cap, out_ids, out_dist, out_counts, out_totals);
  const int64_t nk = nq * cap;
  dev.launch(eps::merge_range_args(ids, nk * 8, dist, nk * 4, counts, nq * 4, totals, nq * 8, shards, nq, cap, out_ids, out_dist, out_counts, out_totals));
  return hipGetLastError() == hipSuccess ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

int64_t eps_range_pack_bytes(int64_t nq, int32_t cap) {
  if (nq < 0 || cap < 1 || cap > eps::MERGE_MAX_CAP || !eps::merge_sizes_ok(1, nq, cap)) return -1;
  return eps::range_pack(nq, cap).bytes;
}

int32_t eps_merge_range_packed(const void* gathered, int64_t shard_stride_bytes, int32_t shards, int64_t nq, int32_t cap, int64_t* out_ids, float* out_dist,
                               int32_t* out_counts, int64_t* out_totals, int32_t device, void* stream) {
  const char* why;
  const int32_t rc = eps::merge_range_check(shards, nq, cap, &why);
  if (rc != EPS_OK) return merge_refused("eps_merge_range_packed", why, rc);
  if (shard_stride_bytes < eps::range_pack(nq, cap).bytes || (shard_stride_bytes & 7))
    return merge_refused("eps_merge_range_packed", "shard_stride_bytes must be a multiple of 8 and at least eps_range_pack_bytes", EPS_USER_ERROR);
  if (nq == 0) return EPS_OK;
  if (!gathered || !out_ids || !out_dist) return merge_refused("eps_merge_range_packed", "null pointer", EPS_USER_ERROR);
  if (hipSetDevice(device) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  HipMergeDev dev{static_cast<hipStream_t>(stream)};
  const void* ptrs[] = {gathered, out_ids, out_dist, out_counts, out_totals};
  if (eps::merge_side(dev, ptrs, 5) != 1) return merge_refused("eps_merge_range_packed", "the gathered buffer and the results are device buffers", EPS_USER_ERROR);
  dev.launch(eps::merge_range_args_packed(gathered, shard_stride_bytes, shards, nq, cap, out_ids, out_dist, out_counts, out_totals));
  return hipGetLastError() == hipSuccess ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

int32_t eps_merge_select(const int64_t* ids, const int64_t* counts, const int64_t* totals, int32_t shards, int64_t len, int64_t skip, int64_t limit,
                         int64_t* out_ids, int64_t* count_out, int64_t* total_out, int32_t device, void* stream) {
  const char* why;
  const int32_t rc = eps::merge_select_check((ids || len == 0) && counts && totals && (out_ids || limit == 0) && count_out, shards, len, skip, limit, &why);
  if (rc != EPS_OK) return merge_refused("eps_merge_select", why, rc);
  if (hipSetDevice(device) != hipSuccess) return EPS_INFRA_UNEXPECTED_ERROR;
  HipMergeDev dev{static_cast<hipStream_t>(stream)};
  const void* ptrs[] = {len ? ids : nullptr, counts, totals, limit ? out_ids : nullptr, count_out, total_out};
  const int side = eps::merge_side(dev, ptrs, 6);
  if (side < 0) return merge_refused("eps_merge_select", "lists and results must all be host or all be device buffers", EPS_USER_ERROR);
  if (side == 0) return eps::merge_select_host(dev, ids, counts, totals, shards, len, skip, limit, out_ids, count_out, total_out);
  dev.launch(eps::merge_select_args(ids, counts, totals, shards, len, skip, limit, out_ids, count_out, total_out));
  return hipGetLastError() == hipSuccess ? EPS_OK : EPS_INFRA_UNEXPECTED_ERROR;
}

// ---- sparse-vector fields (sparse_index.cpp; kernels: sparse.hip, sparse_inverted.hip)
int32_t eps_sparse_index_create(int64_t dim, int32_t metric, int32_t device, eps_sparse_index** out) {
  if (!out) return EPS_USER_ERROR;
  *out = nullptr;
  if (dim < 1 || dim > eps::SPARSE_MAX_DIM || metric < 0 || metric > 2) return EPS_USER_ERROR;
  try {
    eps::SparseIndex* ix = new eps::SparseIndex(dim, metric, device);
    const int32_t rc = ix->init();
    if (rc != EPS_OK) {
      std::fprintf(stderr, "eps_sparse_index_create: %s\n", ix->last_error());
      delete ix;
      return rc;
    }
    *out = reinterpret_cast<eps_sparse_index*>(ix);
    return EPS_OK;
  } catch (...) {
    return map_exception(nullptr);
  }
}
int32_t eps_sparse_index_destroy(eps_sparse_index* h) {
  if (!h) return EPS_USER_ERROR;
  try {
    delete SIX(h);
    return EPS_OK;
  } catch (...) {
    return map_exception(nullptr);
  }
}
const char* eps_sparse_index_last_error(const eps_sparse_index* h) { return h ? reinterpret_cast<const eps::SparseIndex*>(h)->last_error() : "null handle"; }
int32_t eps_sparse_index_set_stream(eps_sparse_index* h, void* s) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.set_stream(s); });
}
int32_t eps_sparse_index_synchronize(eps_sparse_index* h) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.synchronize(); });
}
int32_t eps_sparse_index_attach_csr(eps_sparse_index* h, const int64_t* offsets, const int32_t* indices, const float* values, int64_t n) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.attach_csr(offsets, indices, values, n); });
}
int64_t eps_sparse_index_row_count(const eps_sparse_index* h) { return h ? reinterpret_cast<const eps::SparseIndex*>(h)->row_count() : -1; }
int32_t eps_sparse_index_set_id_map(eps_sparse_index* h, int64_t b, int64_t s) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.set_id_map(b, s); });
}
int32_t eps_sparse_index_set_deleted(eps_sparse_index* h, const uint8_t* bits, int64_t nbytes) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.set_deleted(bits, nbytes); });
}
int32_t eps_sparse_index_search(eps_sparse_index* h, const int64_t* q_offsets, const int32_t* q_indices, const float* q_values, int64_t nq, int32_t k,
                                int64_t* ids, float* dist, int32_t* counts) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.search(q_offsets, q_indices, q_values, nq, k, ids, dist, counts); });
}
int32_t eps_sparse_index_last_stats(const eps_sparse_index* h, eps_search_stats* out) {
  if (!h || !out) return EPS_USER_ERROR;
  return SIX(const_cast<eps_sparse_index*>(h))->last_stats(out);
}
int32_t eps_sparse_index_build_inverted(eps_sparse_index* h) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.build_inverted(); });
}
int32_t eps_sparse_index_drop_inverted(eps_sparse_index* h) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.drop_inverted(); });
}
int32_t eps_sparse_index_inverted_info(const eps_sparse_index* h, int64_t* columns, int64_t* postings, int64_t* longest_column, int32_t* last_engine) {
  if (!h) return EPS_USER_ERROR;
  return reinterpret_cast<const eps::SparseIndex*>(h)->inverted_info(columns, postings, longest_column, last_engine);
}
int32_t eps_sparse_index_get_inverted(eps_sparse_index* h, int64_t* col_offsets, int32_t* rows, float* values) {
  return on_sparse(h, [&](eps::SparseIndex& ix) { return ix.get_inverted(col_offsets, rows, values); });
}

int32_t eps_set_tuning(const char* name, const char* value) {
  eps::tune_set(name, value);
  return EPS_OK;
}

}  // extern "C"
