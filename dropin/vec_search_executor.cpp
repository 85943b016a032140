// Implementation of the drop-in VecSearchExecutor (include/db/execution/vec_search_executor.hpp) over the C ABI.
// Reference behaviour followed: engine/db/execution/vec_search_executor.cpp:29-73 (ctor), :833-935 (Search),
// :937-1033 (SearchByAttribute).  The distance / traversal / top-k work is eps_index_search on the MI355X; what
// stays here is glue that needs the DBMS's own types: incremental upload of appended rows, the deleted bitset, and
// the filter compiler: the parsed filter (ExprNode array) is lowered to a device predicate program over
// the packed attribute rows - int / float / bool attributes, constants, arithmetic, comparisons, AND / OR / NOT and
// @distance, with the reference's evaluation rules (expr_evaluator.cpp:127-258) - which the device applies exactly where
// the reference applies deleted_ / LogicalEvaluate.  Filters with leaves only the host can evaluate (strings, LIKE, IN,
// NEARBY) run as in the reference: the device returns the <= L candidates of the post-filter walk (:905-927) and
// LogicalEvaluate is called on those, O(L) per query, not O(N).
#include "db/execution/vec_search_executor.hpp"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <map>
#include <mutex>
#include <stdexcept>
#include <tuple>

#include "dist_func.hpp"
#include "epsilla_gfx950.h"

namespace vectordb {
namespace engine {
namespace execution {

using vectordb::query::expr::ExprEvaluator;
using vectordb::query::expr::ExprNode;
using vectordb::query::expr::ExprNodePtr;
using vectordb::query::expr::NodeType;

// One in-flight Search() call waiting to be served by the micro-batcher.
struct Pending {
  const float* query;
  vectordb::engine::TableSegmentMVP* segment;
  int32_t k;
  // executor state the batch must agree on
  const void* graph_owner;
  int64_t graph_n, start_point;
  int64_t* off;
  int64_t* nbr;
  int T;
  int64_t L, Lq, I;
  bool prefilter;
  std::vector<eps_filter_op> program;   // compiled device filter (empty = unfiltered); part of the batch key
  // results
  std::vector<int64_t> ids;
  std::vector<float> dist;
  int32_t count = 0;
  bool done = false;
  std::string error;
};

struct DeviceField;
std::shared_ptr<DeviceField> AcquireFieldForBuild(const float* column, int64_t dim, int metric);

struct DeviceField {
  std::mutex mu;
  // micro-batcher: concurrent Search() calls of the pool's executors are coalesced into one
  // eps_index_search with nq > 1 by whichever caller finds the device idle
  std::mutex qmu;
  std::condition_variable qcv;
  std::deque<Pending*> queue;
  bool busy = false;
  eps_index* h = nullptr;
  const float* column = nullptr;
  int64_t dim = 0;
  int metric = 0;
  int64_t attached = 0;            // rows already in HBM
  const void* graph_owner = nullptr;  // ANNGraphSegment whose CSR is on the device
  int64_t graph_n = -1;
  bool sharded = false;            // several GPUs (EPS_DEVICES): every shard searches its rows, the per-shard top-k lists are merged
  const void* shard_graph_owner = nullptr;   // sharded: the ANNGraphSegment whose per-shard graphs the shards hold (BuildGraphOnMirror)
  int64_t shard_graph_n = -1;
  std::vector<uint8_t> mask;       // scratch: deleted | !filter, for filters evaluated on the host
  std::vector<int32_t> devices;    // the device list the mirror was created on (a rebuild's side copy lives on the same devices)
  // A rebuild works on a SIDE index (a device copy of rows [0, n), eps_index_clone_rows) while this one keeps serving; the finished
  // index waits here until the first search of the NEW segment's executors adopts it (BuildGraphOnMirror / Adopt below).
  eps_index* pending_h = nullptr;
  const void* pending_owner = nullptr;
  int64_t pending_n = -1;
  const void* retired_owner = nullptr;   // the segment whose graph the adopted index replaced: its last executors run on the new graph
  ~DeviceField() {
    if (h) eps_index_destroy(h);
    if (pending_h) eps_index_destroy(pending_h);
  }
};

// eps_index_search for the adapter.  The reference accepts SearchQueueSize / LocalQueueSize up to 10^7 and IntraQueryThreads up to 128 at any
// out-degree (config/config.hpp:29, 37-44); the device traversal runs queues up to 2^20 keys and IntraQueryThreads x out-degree <= 2048
// (csrc/traverse.hip) and REFUSES the rest (EPS_DB_UNSUPPORTED_ERROR) rather than run another configuration.  The reference would never
// answer such a Search with an error, so the adapter answers it with the exact scan (the result every graph configuration approximates; the
// reference's result-count caps are applied by the callers as for any search) and says so once.  VERDICT r4 #10.
static int32_t SearchOrExactScan(eps_index* h, const float* q, int64_t nq, int32_t k, eps_search_params* p, int64_t* ids, float* dist, int32_t* cnt) {
  int32_t rc = eps_index_search(h, q, nq, k, p, ids, dist, cnt);
  if (rc == EPS_DB_UNSUPPORTED_ERROR && p->mode != EPS_MODE_FLAT) {
    const char* why = eps_index_last_error(h);
    if (eps_index_last_error_class(h) == EPS_ERRCLASS_DEVICE_RANGE) {   // (the library's own classification, not its wording: ADVICE r5)
      static std::atomic<bool> said{false};
      if (!said.exchange(true))
        fprintf(stderr, "[gfx950 executor] %s - this configuration is answered by the exact scan (recall 1.0) from now on\n", why);
      eps_search_params flat = *p;
      flat.mode = EPS_MODE_FLAT;
      rc = eps_index_search(h, q, nq, k, &flat, ids, dist, cnt);
    }
  }
  return rc;
}

// dev.mu held.  A search of the segment `owner` arrives: if the rebuild that produced that segment left its index waiting, it becomes
// the serving index now - the rows appended since the build's snapshot are added from the host column (only they cross PCIe), the
// old index is released.  Returns an error text or "".
static std::string AdoptPendingBuild(DeviceField& dev, const void* owner, int64_t dim) {
  if (!dev.pending_h || dev.pending_owner != owner) return "";
  if (dev.attached > dev.pending_n) {
    if (eps_index_append_rows(dev.pending_h, dev.column + dev.pending_n * dim, dev.attached - dev.pending_n) != EPS_OK)
      return std::string("gfx950 executor: row upload (adopting the rebuilt index): ") + eps_index_last_error(dev.pending_h);
  }
  eps_index* old = dev.h;
  dev.h = dev.pending_h;
  dev.pending_h = nullptr;
  dev.retired_owner = dev.sharded ? dev.shard_graph_owner : dev.graph_owner;
  if (dev.sharded) {
    dev.shard_graph_owner = owner;
    dev.shard_graph_n = dev.pending_n;
  } else {
    dev.graph_owner = owner;
    dev.graph_n = dev.pending_n;
  }
  dev.pending_owner = nullptr;
  dev.pending_n = -1;
  eps_index_destroy(old);
  return "";
}

namespace {
std::mutex g_mu;
std::map<std::tuple<const float*, int64_t, int>, std::weak_ptr<DeviceField>> g_fields;

std::shared_ptr<DeviceField> AcquireField(const float* column, int64_t dim, int metric) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto key = std::make_tuple(column, dim, metric);
  auto it = g_fields.find(key);
  if (it != g_fields.end()) {
    if (auto sp = it->second.lock()) return sp;
  }
  auto sp = std::make_shared<DeviceField>();
  sp->column = column;
  sp->dim = dim;
  sp->metric = metric;
  // EPS_DEVICES="0,1,2,3": the field's table is hash-sharded over those GPUs of this process (eps_index_create_sharded);
  // unset or one ordinal: one index on that device
  std::vector<int32_t> devices;
  if (const char* env = getenv("EPS_DEVICES")) {
    for (const char* p = env; *p;) {
      char* end = nullptr;
      const long v = strtol(p, &end, 10);
      if (end == p) break;
      devices.push_back((int32_t)v);
      p = *end == ',' ? end + 1 : end;
    }
  }
  if (devices.empty()) devices.push_back(0);
  sp->devices = devices;
  if (devices.size() > 1) {
    if (eps_index_create_sharded(dim, metric, devices.data(), (int32_t)devices.size(), &sp->h) != EPS_OK) return nullptr;
    sp->sharded = true;
  } else if (eps_index_create(dim, metric, devices[0], &sp->h) != EPS_OK) {
    return nullptr;  // no gfx950 device: Search() reports it
  }
  g_fields[key] = sp;
  return sp;
}

}  // namespace
std::shared_ptr<DeviceField> AcquireFieldForBuild(const float* column, int64_t dim, int metric) { return AcquireField(column, dim, metric); }
namespace {

// ---- filter compiler: ExprNode tree -> eps_filter_op postfix program -------------------------------------------------
struct Compiler {
  const std::vector<ExprNodePtr>& nodes;
  vectordb::engine::TableSegmentMVP* seg;
  std::vector<eps_filter_op> out;
  bool host_only = false;   // met a leaf only the host can evaluate

  void Push(int op, int arg = 0, double dval = 0.0) {
    eps_filter_op o;
    o.op = op;
    o.arg = arg;
    o.ival = 0;
    o.dval = dval;
    out.push_back(o);
  }
  bool Valid(size_t i) const { return i < nodes.size() && nodes[i]; }
  int Offset(const std::string& name) {
    auto it = seg->field_name_mem_offset_map_.find(name);
    if (it == seg->field_name_mem_offset_map_.end()) {
      host_only = true;   // (unknown field: let the reference's evaluator decide)
      return 0;
    }
    return (int)it->second;
  }
  // NumEvaluate (expr_evaluator.cpp:127-165): `dist` = whether @distance is live at this position
  void Num(size_t i, bool dist) {
    if (!Valid(i)) return Push(EPS_FOP_PUSH_CONST, 0, 0.0);
    const ExprNode& n = *nodes[i];
    switch (n.node_type) {
      case NodeType::IntConst: return Push(EPS_FOP_PUSH_CONST, 0, (double)n.int_value);
      case NodeType::DoubleConst: return Push(EPS_FOP_PUSH_CONST, 0, n.double_value);
      case NodeType::Int1Attr: return Push(EPS_FOP_PUSH_I8, Offset(n.field_name));
      case NodeType::Int2Attr: return Push(EPS_FOP_PUSH_I16, Offset(n.field_name));
      case NodeType::Int4Attr: return Push(EPS_FOP_PUSH_I32, Offset(n.field_name));
      case NodeType::Int8Attr: return Push(EPS_FOP_PUSH_I64, Offset(n.field_name));
      case NodeType::DoubleAttr:
      case NodeType::FloatAttr:
        if (n.field_name == "@distance") return dist ? Push(EPS_FOP_PUSH_DIST) : Push(EPS_FOP_PUSH_CONST, 0, 0.0);
        return Push(n.node_type == NodeType::DoubleAttr ? EPS_FOP_PUSH_F64 : EPS_FOP_PUSH_F32, Offset(n.field_name));
      case NodeType::Add:
      case NodeType::Subtract:
      case NodeType::Multiply:
      case NodeType::Divide:
      case NodeType::Module:
        if (n.left != (size_t)-1 && n.right != (size_t)-1) {
          Num(n.left, dist);
          Num(n.right, dist);
          return Push(n.node_type == NodeType::Add ? EPS_FOP_ADD : n.node_type == NodeType::Subtract ? EPS_FOP_SUB
                      : n.node_type == NodeType::Multiply ? EPS_FOP_MUL : n.node_type == NodeType::Divide ? EPS_FOP_DIV : EPS_FOP_MOD);
        }
        return Push(EPS_FOP_PUSH_CONST, 0, 0.0);
      default:
        return Push(EPS_FOP_PUSH_CONST, 0, 0.0);   // NumEvaluate's `return 0.0`
    }
  }
  // LogicalEvaluate (:170-258).  Children of AND / OR / NOT and boolean EQ / NE are evaluated WITHOUT the distance
  // (LogicalEvaluate(child, cand) -> distance 0, :184, :207-208, :217-218).
  void Logical(size_t i, bool dist) {
    if (!Valid(i)) return Push(EPS_FOP_PUSH_CONST, 0, 0.0);
    const ExprNode& n = *nodes[i];
    switch (n.node_type) {
      case NodeType::BoolConst: return Push(EPS_FOP_PUSH_CONST, 0, n.bool_value ? 1.0 : 0.0);
      case NodeType::BoolAttr: return Push(EPS_FOP_PUSH_BOOL, Offset(n.field_name));
      case NodeType::NOT:
        Logical(n.left, false);
        return Push(EPS_FOP_NOT);
      case NodeType::IN:
      case NodeType::LIKE:
      case NodeType::FunctionCall:
        host_only = true;
        return Push(EPS_FOP_PUSH_CONST, 0, 0.0);
      default: break;
    }
    if (n.left == (size_t)-1 || n.right == (size_t)-1 || !Valid(n.left) || !Valid(n.right)) return Push(EPS_FOP_PUSH_CONST, 0, 0.0);
    switch (n.node_type) {
      case NodeType::EQ:
      case NodeType::NE: {
        const auto vt = nodes[n.left]->value_type;
        if (vt == vectordb::query::expr::ValueType::STRING) {
          host_only = true;
          return Push(EPS_FOP_PUSH_CONST, 0, 0.0);
        }
        if (vt == vectordb::query::expr::ValueType::BOOL) {
          Logical(n.left, false);
          Logical(n.right, false);
          return Push(n.node_type == NodeType::EQ ? EPS_FOP_EQ_BOOL : EPS_FOP_NE_BOOL);
        }
        Num(n.left, dist);
        Num(n.right, dist);
        return Push(n.node_type == NodeType::EQ ? EPS_FOP_EQ : EPS_FOP_NE);
      }
      case NodeType::AND:
      case NodeType::OR:
        Logical(n.left, false);
        Logical(n.right, false);
        return Push(n.node_type == NodeType::AND ? EPS_FOP_AND : EPS_FOP_OR);
      case NodeType::GT:
      case NodeType::GTE:
      case NodeType::LT:
      case NodeType::LTE:
        Num(n.left, dist);
        Num(n.right, dist);
        return Push(n.node_type == NodeType::GT ? EPS_FOP_GT : n.node_type == NodeType::GTE ? EPS_FOP_GE
                    : n.node_type == NodeType::LT ? EPS_FOP_LT : EPS_FOP_LE);
      default:
        return Push(EPS_FOP_PUSH_CONST, 0, 0.0);   // LogicalEvaluate's `return false`
    }
  }
};
}  // namespace

// dev.mu held.  What a device call of an executor finds in HBM before it runs: the rows appended since the last call, the index a
// rebuild left waiting for this segment, and this executor's graph.  Throws like Search().
static void SyncRowsAndGraph(DeviceField& dev, VecSearchExecutor& ex, vectordb::engine::TableSegmentMVP* table_segment) {
  auto fail = [&](const char* what) { throw std::runtime_error(std::string("gfx950 executor: ") + what + ": " + eps_index_last_error(dev.h)); };
  // rows [0, record_number_) are immutable once written (SURVEY §8b "Ownership"): upload only the new tail
  const int64_t total_vector = table_segment->record_number_;
  if (total_vector > dev.attached) {
    const float* base = std::get<DenseVectorColumnDataContainer>(ex.vector_column_);
    const int32_t rc = dev.attached == 0 ? eps_index_attach_rows(dev.h, base, total_vector)
                                         : eps_index_append_rows(dev.h, base + dev.attached * ex.dimension_, total_vector - dev.attached);
    if (rc != EPS_OK) fail("row upload");
    dev.attached = total_vector;
  }
  {
    const std::string aerr = AdoptPendingBuild(dev, ex.ann_index_->OwnerKey(), ex.dimension_);
    if (!aerr.empty()) throw std::runtime_error(aerr);
  }
  // (an executor of the segment a rebuild just replaced finishes on the new graph: uploading its old CSR again would only be undone by
  // the next search of the new segment)
  if (!dev.sharded && ex.ann_index_->OwnerKey() != dev.retired_owner &&
      (dev.graph_owner != ex.ann_index_->OwnerKey() || dev.graph_n != ex.total_indexed_vector_)) {
    if (eps_index_set_graph(dev.h, ex.total_indexed_vector_, ex.offset_table_, ex.neighbor_list_, ex.start_search_point_) != EPS_OK) fail("graph upload");
    dev.graph_owner = ex.ann_index_->OwnerKey();
    dev.retired_owner = nullptr;   // (another segment's graph is in HBM now: nobody runs "on the graph that replaced mine" any more)
    dev.graph_n = ex.total_indexed_vector_;
  }
}

// dev.mu held.  The call's predicate: the compiled program (empty = none) over the segment's attribute rows, and the deleted bitset.
static void SyncPredicate(DeviceField& dev, vectordb::engine::TableSegmentMVP* table_segment, const std::vector<eps_filter_op>& program) {
  auto fail = [&](const char* what) { throw std::runtime_error(std::string("gfx950 executor: ") + what + ": " + eps_index_last_error(dev.h)); };
  ConcurrentBitset& deleted = *(table_segment->deleted_);
  if (eps_index_set_int_filter(dev.h, nullptr, 0, 0, EPS_OP_NONE, 0) != EPS_OK) fail("filter reset");
  if (!program.empty()) {
    // the attribute rows are handed over as they are: TableSegmentMVP::attribute_table_, primitive_offset_ bytes per row
    // (append-only: an update of the reference's table is delete + insert, table_segment_mvp.cpp:476-587; the device mirror is per
    // table segment, so a dropped-and-recreated table never meets a cached copy)
    if (eps_index_set_filter_program_ex(dev.h, program.data(), (int32_t)program.size(), table_segment->attribute_table_,
                                        table_segment->primitive_offset_, table_segment->record_number_, EPS_FILTER_ROWS_APPEND_ONLY) != EPS_OK)
      fail("filter program upload");
  } else if (eps_index_set_filter_program(dev.h, nullptr, 0, nullptr, 0, 0) != EPS_OK) {
    fail("filter reset");
  }
  if (eps_index_set_deleted(dev.h, deleted.data(), (int64_t)deleted.size()) != EPS_OK) fail("deleted upload");
}

VecSearchExecutor::VecSearchExecutor(const int64_t dimension, const int64_t start_search_point,
                                     std::shared_ptr<ANNGraphSegment> ann_index, int64_t* offset_table,
                                     int64_t* neighbor_list,
                                     std::variant<DenseVectorColumnDataContainer, VariableLenAttrColumnContainer*> vector_column,
                                     DistFunc fstdistfunc, void* dist_func_param, int num_threads, int64_t L_master,
                                     int64_t L_local, int64_t subsearch_iterations, bool prefilter_enabled)
    : ann_index_(ann_index),
      total_indexed_vector_(ann_index->record_number_),
      dimension_(dimension),
      start_search_point_(start_search_point),
      offset_table_(offset_table),
      neighbor_list_(neighbor_list),
      vector_column_(vector_column),
      fstdistfunc_(fstdistfunc),
      dist_func_param_(dist_func_param),
      num_threads_(num_threads),
      L_master_(L_master),
      L_local_(L_local),
      subsearch_iterations_(subsearch_iterations),
      prefilter_enabled_(prefilter_enabled),
      search_result_(L_master),
      distance_(L_master),
      brute_force_search_(ann_index->record_number_ < BruteforceThreshold) {
  if (std::holds_alternative<DenseVectorColumnDataContainer>(vector_column_) &&
      std::holds_alternative<DenseVecDistFunc<float>>(fstdistfunc_)) {
    metric_ = epsdrop::MetricOfDistFunc(reinterpret_cast<const void*>(std::get<DenseVecDistFunc<float>>(fstdistfunc_)));
    if (metric_ >= 0) dev_ = AcquireField(std::get<DenseVectorColumnDataContainer>(vector_column_), dimension_, metric_);
  }
}

VecSearchExecutor::~VecSearchExecutor() {}

Status VecSearchExecutor::Search(const VectorPtr query_data, vectordb::engine::TableSegmentMVP* table_segment,
                                 const size_t limit, std::vector<ExprNodePtr>& filter_nodes, int64_t& result_size) {
  result_size = 0;
  // TableMVP::Search discards the Status we return (table_mvp.cpp:372), so a failure must not look like "0 results":
  // throw, as the constructors of the reference's own classes do on I/O failure.
  if (!std::holds_alternative<DenseVectorPtr>(query_data) || !std::holds_alternative<DenseVectorColumnDataContainer>(vector_column_))
    throw std::runtime_error("gfx950 executor: sparse-vector fields are not served by the device executor");
  if (!dev_) throw std::runtime_error("no usable gfx950 device (libepsilla_gfx950 has no CPU fallback)");
  if (limit == 0) return Status::OK();
  DeviceField& dev = *dev_;
  {
    // unfiltered queries and queries whose filter compiles to a device program go through the micro-batcher: concurrent calls
    // with the same program (the same filter text) share one device batch
    static const bool batching = !(getenv("EPS_DROPIN_BATCH") && atoi(getenv("EPS_DROPIN_BATCH")) == 0);
    if (batching) {
      const int root0 = static_cast<int>(filter_nodes.size()) - 1;
      const bool unfiltered = root0 < 0 || (filter_nodes[root0]->node_type == NodeType::BoolConst && filter_nodes[root0]->bool_value);
      if (unfiltered) return SearchBatched(std::get<DenseVectorPtr>(query_data), table_segment, limit, result_size, nullptr);
      Compiler c{filter_nodes, table_segment};
      c.Logical((size_t)root0, true);
      if (!c.host_only && c.out.size() <= 64) return SearchBatched(std::get<DenseVectorPtr>(query_data), table_segment, limit, result_size, &c.out);
    }
  }
  std::lock_guard<std::mutex> lk(dev.mu);
  auto fail = [&](const char* what) -> Status {
    throw std::runtime_error(std::string("gfx950 executor: ") + what + ": " + eps_index_last_error(dev.h));
  };

  const int64_t total_vector = table_segment->record_number_;
  SyncRowsAndGraph(dev, *this, table_segment);

  // ---- filter lowering
  ConcurrentBitset& deleted = *(table_segment->deleted_);
  const int root = static_cast<int>(filter_nodes.size()) - 1;
  bool host_filter = false;
  std::vector<eps_filter_op> program;
  if (root >= 0 && !(filter_nodes[root]->node_type == NodeType::BoolConst && filter_nodes[root]->bool_value)) {
    Compiler c{filter_nodes, table_segment};
    c.Logical((size_t)root, true);
    if (c.host_only || c.out.size() > 64) host_filter = true; else program.swap(c.out);
  }
  SyncPredicate(dev, table_segment, program);

  eps_search_params p;
  eps_default_search_params(&p);
  // EPS_DROPIN_PREFER_EXACT=1 (opt-in, NOT the reference's semantics): answer graph-mode searches with the exact scan - recall 1.0
  // instead of the graph's, and on one MI355X also the lower latency up to tens of millions of rows; result counts
  // keep the reference's caps
  static const bool prefer_exact = getenv("EPS_DROPIN_PREFER_EXACT") && atoi(getenv("EPS_DROPIN_PREFER_EXACT")) != 0;
  p.mode = EPS_MODE_REFERENCE;
  p.prefilter = prefilter_enabled_ ? 1 : 0;
  p.intra_threads = num_threads_;
  p.master_queue = L_master_;
  p.local_queue = L_local_;
  p.sync_interval = subsearch_iterations_;
  const bool flat = prefilter_enabled_ || brute_force_search_ || dev.sharded || prefer_exact;
  if (prefer_exact && !prefilter_enabled_ && !brute_force_search_) p.mode = EPS_MODE_FLAT;
  if (dev.sharded) {
    // A sharded mirror walks graphs only if its shards hold the graphs of THIS executor's segment (BuildGraphOnMirror) - and never for
    // a host-evaluated filter: the brute-force branch below hands the shards a full visibility mask and expects an EXACT scan, a
    // per-shard walk would judge the mask on its top-L only and return too few rows (RunSearch has the same rule)
    const bool shard_graph = dev.shard_graph_owner == ann_index_->OwnerKey() && dev.shard_graph_n == total_indexed_vector_ && total_indexed_vector_ > 0;
    if (host_filter || !shard_graph) p.mode = EPS_MODE_FLAT;
  }
  auto publish = [&](const int64_t* ids, const float* dist, int64_t count) {
    if ((size_t)count > search_result_.size()) {
      search_result_.resize(count);
      distance_.resize(count);
    }
    for (int64_t i = 0; i < count; ++i) {
      search_result_[i] = ids[i];
      distance_[i] = dist[i];
    }
    result_size = count;
  };

  if (!host_filter) {
    // result counts of the reference: PreFilter -> min(|res|, limit) (:856-858); small table -> additionally <= L_local (:864);
    // graph -> min(n_indexed, limit, L_local) (:872)
    size_t want = limit;
    if (!prefilter_enabled_) want = std::min<size_t>(want, (size_t)std::max<int64_t>(L_local_, 1));
    want = std::min<size_t>(want, (size_t)std::max<int64_t>(total_vector, 1));   // (never more results than rows)
    if (want > ((size_t)1 << 20)) throw std::runtime_error("gfx950 executor: more than 1048576 results per query are not supported");
    const int32_t k = (int32_t)want;
    std::vector<int64_t> ids((size_t)k);
    std::vector<float> dist((size_t)k);
    int32_t count = 0;
    if (SearchOrExactScan(dev.h, std::get<DenseVectorPtr>(query_data), 1, k, &p, ids.data(), dist.data(), &count) != EPS_OK)
      return fail("search");
    publish(ids.data(), dist.data(), count);
    return Status::OK();
  }

  // ---- host-evaluated predicate on the candidates of the reference's own walk
  ExprEvaluator ev(filter_nodes, table_segment->field_name_mem_offset_map_, table_segment->primitive_offset_,
                   table_segment->var_len_attr_num_, table_segment->attribute_table_, table_segment->var_len_attr_table_);
  std::vector<int64_t> out_ids;
  std::vector<float> out_dist;
  if (!flat) {
    // graph: walk the <= L_master candidates in order, stop at searchLimit (:905-927)
    if (total_vector > total_indexed_vector_) {
      // the reference's BruteForceSearch over the un-indexed tail (:885-889) drops deleted rows and rows failing the filter
      // (evaluated with the row's distance) BEFORE the merge into the first K slots: the tail rows are judged here, on the
      // host as in the reference (O(tail)), and handed to the device as invisible
      bool uses_distance = false;
      for (auto& n : filter_nodes) uses_distance |= n && n->field_name == "@distance";
      const float* base = std::get<DenseVectorColumnDataContainer>(vector_column_);
      auto dfn = std::get<DenseVecDistFunc<float>>(fstdistfunc_);
      dev.mask.assign(deleted.data(), deleted.data() + deleted.size());
      if (dev.mask.size() < (size_t)(total_vector + 7) / 8) dev.mask.resize((size_t)(total_vector + 7) / 8, 0);
      for (int64_t id = total_indexed_vector_; id < total_vector; ++id) {
        if (deleted.test(id)) continue;
        const float d = uses_distance ? dfn(base + id * dimension_, std::get<DenseVectorPtr>(query_data), dist_func_param_) : 0.f;
        if (!ev.LogicalEvaluate(root, id, d)) dev.mask[id >> 3] |= uint8_t(1u << (id & 7));
      }
      if (eps_index_set_deleted(dev.h, dev.mask.data(), (int64_t)dev.mask.size()) != EPS_OK) return fail("mask upload");
    }
    const int64_t K = std::min<int64_t>({total_indexed_vector_, (int64_t)limit, L_local_});
    const int32_t cap = (int32_t)std::min<int64_t>(std::max<int64_t>(L_master_, K), (int64_t)1 << 20);
    std::vector<int64_t> ids((size_t)cap);
    std::vector<float> dist((size_t)cap);
    int32_t count = 0;
    if (eps_index_search_walk(dev.h, std::get<DenseVectorPtr>(query_data), 1, (int32_t)std::min<size_t>(limit, (size_t)1 << 20), cap, &p, ids.data(),
                              dist.data(), &count) != EPS_OK)
      return fail("search");
    for (int32_t i = 0; i < count && (int64_t)out_ids.size() < K; ++i)
      if (ev.LogicalEvaluate(root, ids[i], dist[i])) {
        out_ids.push_back(ids[i]);
        out_dist.push_back(dist[i]);
      }
    publish(out_ids.data(), out_dist.data(), (int64_t)out_ids.size());
    return Status::OK();
  }
  // brute force (:717-831): the answer is the first `want` passing rows in (dist,id) order.  Fetch the closest candidates
  // in growing portions and stop as soon as enough of them pass; a filter so selective that 1024 candidates do not
  // suffice falls back to evaluating it on every row, which is what the reference does for every query.
  size_t want = std::min<size_t>(limit, (size_t)total_vector);
  if (!prefilter_enabled_) want = std::min<size_t>(want, (size_t)std::max<int64_t>(L_local_, 1));
  for (int32_t cap = (int32_t)std::min<size_t>(1024, std::max<size_t>(64, 4 * want)); want <= 1024 && !dev.sharded; cap = std::min(1024, cap * 4)) {
    std::vector<int64_t> ids((size_t)cap);
    std::vector<float> dist((size_t)cap);
    int32_t count = 0;
    if (eps_index_search_walk(dev.h, std::get<DenseVectorPtr>(query_data), 1, (int32_t)want, cap, &p, ids.data(), dist.data(), &count) != EPS_OK)
      return fail("search");
    out_ids.clear();
    out_dist.clear();
    for (int32_t i = 0; i < count && out_ids.size() < want; ++i)
      if (prefilter_enabled_ ? ev.LogicalEvaluate(root, ids[i]) : ev.LogicalEvaluate(root, ids[i], dist[i])) {   // (:795 vs :751)
        out_ids.push_back(ids[i]);
        out_dist.push_back(dist[i]);
      }
    if (out_ids.size() >= want || count < cap) {   // enough passed, or the table has no more visible rows
      publish(out_ids.data(), out_dist.data(), (int64_t)out_ids.size());
      return Status::OK();
    }
    if (cap >= 1024) break;
  }
  if (want > ((size_t)1 << 20)) throw std::runtime_error("gfx950 executor: more than 1048576 results per query are not supported");
  // selective host-only filter: visibility of every row, evaluated on the host - the reference's own cost for every
  // brute-force query (:746-755); @distance, if the filter reads it, comes from the host distance function as there
  bool uses_distance = false;
  for (auto& n : filter_nodes) uses_distance |= n && n->field_name == "@distance";
  {
    const float* base = std::get<DenseVectorColumnDataContainer>(vector_column_);
    auto dfn = std::get<DenseVecDistFunc<float>>(fstdistfunc_);
    dev.mask.assign((size_t)(total_vector + 7) / 8, 0);
    for (int64_t id = 0; id < total_vector; ++id) {
      bool pass = !deleted.test(id);
      if (pass) {
        if (prefilter_enabled_ || !uses_distance) pass = ev.LogicalEvaluate(root, id);
        else pass = ev.LogicalEvaluate(root, id, dfn(base + id * dimension_, std::get<DenseVectorPtr>(query_data), dist_func_param_));
      }
      if (!pass) dev.mask[id >> 3] |= uint8_t(1u << (id & 7));
    }
  }
  if (eps_index_set_deleted(dev.h, dev.mask.data(), (int64_t)dev.mask.size()) != EPS_OK) return fail("mask upload");
  {
    const int32_t k = (int32_t)want;
    std::vector<int64_t> ids((size_t)k);
    std::vector<float> dist((size_t)k);
    int32_t count = 0;
    if (SearchOrExactScan(dev.h, std::get<DenseVectorPtr>(query_data), 1, k, &p, ids.data(), dist.data(), &count) != EPS_OK)
      return fail("search");
    publish(ids.data(), dist.data(), count);
  }
  return Status::OK();
}


// ---- micro-batched path for unfiltered queries -------------------------------------------------------------------
namespace {
bool SameKey(const Pending& a, const Pending& b) {
  return a.segment == b.segment && a.k == b.k && a.graph_owner == b.graph_owner && a.graph_n == b.graph_n && a.T == b.T &&
         a.L == b.L && a.Lq == b.Lq && a.I == b.I && a.prefilter == b.prefilter && a.program.size() == b.program.size() &&
         (a.program.empty() || std::memcmp(a.program.data(), b.program.data(), a.program.size() * sizeof(eps_filter_op)) == 0);
}

// One device batch: bring the mirror up to date for the batch's key (rows, graph, filter program, deleted bitset), then ONE
// eps_index_search over nq contiguous queries.  Returns the error text ("" = ok).
std::string RunSearch(DeviceField& dev, int64_t dim, const Pending& h, const float* q, int64_t nq, int64_t* ids, float* dist, int32_t* cnt) {
  std::lock_guard<std::mutex> lk(dev.mu);
  std::string err;
  auto fail = [&](const char* what) { err = std::string("gfx950 executor: ") + what + ": " + eps_index_last_error(dev.h); };
  const int64_t total_vector = h.segment->record_number_;
  if (total_vector > dev.attached) {
    const int32_t rc = dev.attached == 0 ? eps_index_attach_rows(dev.h, dev.column, total_vector)
                                         : eps_index_append_rows(dev.h, dev.column + dev.attached * dim, total_vector - dev.attached);
    if (rc != EPS_OK) fail("row upload"); else dev.attached = total_vector;
  }
  if (err.empty()) err = AdoptPendingBuild(dev, h.graph_owner, dim);
  if (err.empty() && !dev.sharded && h.graph_owner != dev.retired_owner && (dev.graph_owner != h.graph_owner || dev.graph_n != h.graph_n)) {
    if (eps_index_set_graph(dev.h, h.graph_n, h.off, h.nbr, h.start_point) != EPS_OK) fail("graph upload");
    else { dev.graph_owner = h.graph_owner; dev.graph_n = h.graph_n; dev.retired_owner = nullptr; }
  }
  ConcurrentBitset& deleted = *(h.segment->deleted_);
  if (err.empty() && eps_index_set_int_filter(dev.h, nullptr, 0, 0, EPS_OP_NONE, 0) != EPS_OK) fail("filter reset");
  if (err.empty()) {
    const int32_t rc = h.program.empty() ? eps_index_set_filter_program(dev.h, nullptr, 0, nullptr, 0, 0)
                                         : eps_index_set_filter_program_ex(dev.h, h.program.data(), (int32_t)h.program.size(), h.segment->attribute_table_,
                                                                           h.segment->primitive_offset_, total_vector, EPS_FILTER_ROWS_APPEND_ONLY);
    if (rc != EPS_OK) fail("filter program upload");
  }
  if (err.empty() && eps_index_set_deleted(dev.h, deleted.data(), (int64_t)deleted.size()) != EPS_OK) fail("deleted upload");
  if (err.empty()) {
    eps_search_params p;
    eps_default_search_params(&p);
    static const bool prefer_exact = getenv("EPS_DROPIN_PREFER_EXACT") && atoi(getenv("EPS_DROPIN_PREFER_EXACT")) != 0;
    p.mode = prefer_exact && !h.prefilter ? EPS_MODE_FLAT : EPS_MODE_REFERENCE;
    // a sharded mirror searches graphs only if its shards hold the graphs of THIS request's segment (built by BuildGraphOnMirror);
    // otherwise exact per-shard scans
    if (dev.sharded && !(dev.shard_graph_owner == h.graph_owner && dev.shard_graph_n == h.graph_n && h.graph_n > 0)) p.mode = EPS_MODE_FLAT;
    p.prefilter = h.prefilter ? 1 : 0;
    p.intra_threads = h.T;
    p.master_queue = h.L;
    p.local_queue = h.Lq;
    p.sync_interval = h.I;
    // EPS_DROPIN_FILTER_IN_TRAVERSAL=1 (opt-in, NOT the reference's semantics): graph searches with a device-compiled filter judge every
    // row they evaluate instead of the final top-L walk, so selective filters still return `limit` rows
    static const bool filter_in_traversal = getenv("EPS_DROPIN_FILTER_IN_TRAVERSAL") && atoi(getenv("EPS_DROPIN_FILTER_IN_TRAVERSAL")) != 0;
    p.filter_in_traversal = filter_in_traversal ? 1 : 0;
    // EPS_DROPIN_BATCH_T1=1 (opt-in, NOT the reference's knob setting): the reference's IntraQueryThreads spreads ONE query over cores to cut its
    // latency; a device batch of >= 64 queries fills the GPU with queries instead, and at equal recall one worker per query is the faster walk there
    // (10M x 768 manifold set, L = 100, batch 1024: 519.6 k q/s at T = 1 vs 431.5 k at T = 4, profiles/r4_graph_10Mx768_manifold_sweep.jsonl)
    static const bool batch_t1 = getenv("EPS_DROPIN_BATCH_T1") && atoi(getenv("EPS_DROPIN_BATCH_T1")) != 0;
    if (batch_t1 && nq >= 64) p.intra_threads = 1;
    if (SearchOrExactScan(dev.h, q, nq, h.k, &p, ids, dist, cnt) != EPS_OK) fail("search");
  }
  return err;
}

void RunBatch(DeviceField& dev, int64_t dim, std::vector<Pending*>& batch) {
  Pending& h = *batch[0];
  const int64_t nq = (int64_t)batch.size();
  const int32_t k = h.k;
  std::vector<float> q((size_t)nq * dim);
  std::vector<int64_t> ids((size_t)nq * k);
  std::vector<float> dist((size_t)nq * k);
  std::vector<int32_t> cnt((size_t)nq);
  for (int64_t i = 0; i < nq; ++i) std::memcpy(&q[(size_t)i * dim], batch[i]->query, sizeof(float) * dim);
  const std::string err = RunSearch(dev, dim, h, q.data(), nq, ids.data(), dist.data(), cnt.data());
  for (int64_t i = 0; i < nq; ++i) {
    Pending& r = *batch[i];
    r.error = err;
    if (err.empty()) {
      r.count = cnt[i];
      r.ids.assign(ids.begin() + i * k, ids.begin() + i * k + cnt[i]);
      r.dist.assign(dist.begin() + i * k, dist.begin() + i * k + cnt[i]);
    }
  }
}
}  // namespace

// the part of a request every member of a device batch must agree on (result count rules: see Search)
void VecSearchExecutor::FillKey(Pending& me, vectordb::engine::TableSegmentMVP* table_segment, size_t limit, const std::vector<eps_filter_op>* program) {
  if (program) me.program = *program;
  me.segment = table_segment;
  size_t want = limit;
  if (!prefilter_enabled_) want = std::min<size_t>(want, (size_t)std::max<int64_t>(L_local_, 1));
  want = std::min<size_t>(want, (size_t)std::max<int64_t>(table_segment->record_number_, 1));
  if (want > ((size_t)1 << 20)) throw std::runtime_error("gfx950 executor: more than 1048576 results per query are not supported");
  me.k = (int32_t)want;
  me.graph_owner = ann_index_->OwnerKey();
  me.graph_n = total_indexed_vector_;
  me.start_point = start_search_point_;
  me.off = offset_table_;
  me.nbr = neighbor_list_;
  me.T = num_threads_;
  me.L = L_master_;
  me.Lq = L_local_;
  me.I = subsearch_iterations_;
  me.prefilter = prefilter_enabled_;
}

// Additive batched entry (the reference is one vector per call: bindings/python/interface.cpp:260-331,
// db_server.cpp:458-510, executor_pool.hpp:10-31): nq queries, row-major, answered by ONE eps_index_search when the filter is
// empty or compiles to a device program - the same mirror synchronisation, the same mode selection and the same result caps
// as nq calls of Search().  Filters with host-only leaves run query by query through Search().  ids / dist: [nq][width]
// (-1 / +inf beyond counts[q]).
Status VecSearchExecutor::SearchBatch(const float* queries, int64_t nq, vectordb::engine::TableSegmentMVP* table_segment, const size_t limit,
                                      std::vector<ExprNodePtr>& filter_nodes, std::vector<int64_t>& ids, std::vector<float>& dist,
                                      std::vector<int32_t>& counts, int32_t& width) {
  width = 0;
  ids.clear();
  dist.clear();
  counts.assign((size_t)std::max<int64_t>(nq, 0), 0);
  if (!std::holds_alternative<DenseVectorColumnDataContainer>(vector_column_))
    throw std::runtime_error("gfx950 executor: sparse-vector fields are not served by the device executor");
  if (!dev_) throw std::runtime_error("no usable gfx950 device (libepsilla_gfx950 has no CPU fallback)");
  if (nq <= 0 || limit == 0) return Status::OK();
  const int root0 = static_cast<int>(filter_nodes.size()) - 1;
  const bool unfiltered = root0 < 0 || (filter_nodes[root0]->node_type == NodeType::BoolConst && filter_nodes[root0]->bool_value);
  std::vector<eps_filter_op> program;
  bool on_device = unfiltered;
  if (!unfiltered) {
    Compiler c{filter_nodes, table_segment};
    c.Logical((size_t)root0, true);
    if (!c.host_only && c.out.size() <= 64) {
      program.swap(c.out);
      on_device = true;
    }
  }
  if (on_device) {
    Pending key;
    FillKey(key, table_segment, limit, unfiltered ? nullptr : &program);
    width = key.k;
    ids.resize((size_t)nq * width);
    dist.resize((size_t)nq * width);
    const std::string err = RunSearch(*dev_, dimension_, key, queries, nq, ids.data(), dist.data(), counts.data());
    if (!err.empty()) throw std::runtime_error(err);
    return Status::OK();
  }
  // host-evaluated predicate: the reference's own walk per query
  size_t w = std::min<size_t>(limit, (size_t)std::max<int64_t>((int64_t)table_segment->record_number_, 1));
  if (!prefilter_enabled_) w = std::min<size_t>(w, (size_t)std::max<int64_t>(L_local_, 1));
  width = (int32_t)w;
  ids.assign((size_t)nq * width, -1);
  dist.assign((size_t)nq * width, std::numeric_limits<float>::infinity());
  for (int64_t q = 0; q < nq; ++q) {
    int64_t rs = 0;
    Search(const_cast<float*>(queries + q * dimension_), table_segment, limit, filter_nodes, rs);
    rs = std::min<int64_t>(rs, width);
    counts[(size_t)q] = (int32_t)rs;
    for (int64_t i = 0; i < rs; ++i) {
      ids[(size_t)q * width + i] = search_result_[i];
      dist[(size_t)q * width + i] = (float)distance_[i];
    }
  }
  return Status::OK();
}

Status VecSearchExecutor::SearchBatched(const float* query, vectordb::engine::TableSegmentMVP* table_segment, size_t limit,
                                        int64_t& result_size, const std::vector<eps_filter_op>* program) {
  DeviceField& dev = *dev_;
  Pending me;
  me.query = query;
  FillKey(me, table_segment, limit, program);
  std::unique_lock<std::mutex> lk(dev.qmu);
  dev.queue.push_back(&me);
  while (!me.done) {
    if (dev.busy) {  // somebody is driving the device: wait until served, or until the device is free again
      dev.qcv.wait(lk, [&] { return me.done || !dev.busy; });
      continue;
    }
    dev.busy = true;  // become the leader: serve the head of the queue and everything compatible with it
    std::vector<Pending*> batch;
    Pending* head = dev.queue.front();
    for (auto it = dev.queue.begin(); it != dev.queue.end() && batch.size() < 2048;) {   // (2048 = one filter slice of the matrix engine)
      if (SameKey(**it, *head)) {
        batch.push_back(*it);
        it = dev.queue.erase(it);
      } else {
        ++it;
      }
    }
    lk.unlock();
    try {
      RunBatch(dev, dimension_, batch);
    } catch (const std::exception& e) {   // (allocation failure while gathering the batch): the followers must still be released
      for (Pending* r : batch) r->error = std::string("gfx950 executor: ") + e.what();
    }
    lk.lock();
    for (Pending* r : batch) r->done = true;
    dev.busy = false;
    dev.qcv.notify_all();
  }
  lk.unlock();
  if (!me.error.empty()) throw std::runtime_error(me.error);
  if ((size_t)me.count > search_result_.size()) {
    search_result_.resize(me.count);
    distance_.resize(me.count);
  }
  for (int32_t i = 0; i < me.count; ++i) {
    search_result_[i] = me.ids[i];
    distance_[i] = me.dist[i];
  }
  result_size = me.count;
  return Status::OK();
}

// No vector arithmetic here: primary-key lookup / geo-index probe / full scan with the host filter engine.
Status VecSearchExecutor::SearchByAttribute(meta::TableSchema& table_schema, vectordb::engine::TableSegmentMVP* table_segment,
                                            const size_t skip, const size_t raw_limit, vectordb::Json& primary_keys,
                                            std::vector<ExprNodePtr>& filter_nodes, int64_t& result_size) {
  const int64_t total_vector = table_segment->record_number_;
  ConcurrentBitset& deleted = *(table_segment->deleted_);
  ExprEvaluator ev(filter_nodes, table_segment->field_name_mem_offset_map_, table_segment->primitive_offset_,
                   table_segment->var_len_attr_num_, table_segment->attribute_table_, table_segment->var_len_attr_table_);
  const int root = static_cast<int>(filter_nodes.size()) - 1;
  const int64_t limit = std::min<int64_t>((int64_t)raw_limit, total_vector);
  if (limit > (int64_t)search_result_.size()) search_result_.resize(limit);
  result_size = 0;
  int64_t seen = 0;  // rows that passed so far (before skip/limit windowing)
  // returns false once the window [skip, skip+limit) is full
  auto offer = [&](int64_t id) {
    if (deleted.test(id) || !ev.LogicalEvaluate(root, id)) return true;
    if (seen >= (int64_t)skip && seen < (int64_t)skip + limit) search_result_[result_size++] = id;
    ++seen;
    return seen < (int64_t)skip + limit;
  };
  const int64_t npk = primary_keys.GetSize();
  if (npk > 0) {
    for (int64_t i = 0; i < npk; ++i) {
      auto pk = primary_keys.GetArrayElement(i);
      size_t id = 0;
      if (table_segment->PK2ID(pk, id) && !offer((int64_t)id)) break;
    }
    return Status::OK();
  }
  bool used_geo = false;
  for (auto& field : table_schema.fields_) {
    if (field.field_type_ != meta::FieldType::GEO_POINT) continue;
    const int64_t node = ev.UpliftingGeoIndex(field.name_, root);
    if (node == -1) continue;
    used_geo = true;
    std::vector<vectordb::engine::index::GeospatialIndex::value_t> hits;
    const double lat = ev.NumEvaluate(filter_nodes[node]->arguments[1], -1, 0);
    const double lon = ev.NumEvaluate(filter_nodes[node]->arguments[2], -1, 0);
    const double rad = ev.NumEvaluate(filter_nodes[node]->arguments[3], -1, 0);
    table_segment->geospatial_indices_[field.name_]->searchWithinRadius(lat, lon, rad, hits);
    for (auto& h : hits)
      if (!offer(h.second)) break;
  }
  if (used_geo) return Status::OK();
  if (SelectOnDevice(table_segment, skip, limit, filter_nodes, result_size)) return Status::OK();
  for (int64_t id = 0; id < total_vector; ++id)
    if (!offer(id)) break;
  return Status::OK();
}

// Tables below this many rows keep the host loop of SearchByAttribute's full scan: see DESIGN.md ("Filter-only gets") for the measurement
// behind it.  EPS_DROPIN_SELECT_MIN_ROWS overrides it (read on every call).
constexpr int64_t kSelectMinRows = 2048;

// The full-scan branch (:1016-1029) on the device: eps_index_select over the field's mirror, when the table is large enough, the mirror is
// one device and the filter is empty / true or compiles to a device program.  false = not taken (nothing was touched): the host loop answers.
// A device error throws, as in Search(): the two paths never stand in for each other on failure.
bool VecSearchExecutor::SelectOnDevice(vectordb::engine::TableSegmentMVP* table_segment, size_t skip, int64_t limit,
                                       std::vector<ExprNodePtr>& filter_nodes, int64_t& result_size) {
  if (!dev_ || dev_->sharded) return false;
  const int64_t total_vector = table_segment->record_number_;
  int64_t min_rows = kSelectMinRows;
  if (const char* e = getenv("EPS_DROPIN_SELECT_MIN_ROWS"))
    if (*e) min_rows = atoll(e);
  if (total_vector < min_rows || total_vector <= 0) return false;
  const int root = static_cast<int>(filter_nodes.size()) - 1;
  std::vector<eps_filter_op> program;
  if (root >= 0 && !(filter_nodes[root]->node_type == NodeType::BoolConst && filter_nodes[root]->bool_value)) {
    Compiler c{filter_nodes, table_segment};
    c.Logical((size_t)root, false);   // (LogicalEvaluate(root, id): no distance, :1018)
    if (c.host_only || c.out.size() > 64) return false;
    program.swap(c.out);
  }
  DeviceField& dev = *dev_;
  std::lock_guard<std::mutex> lk(dev.mu);
  SyncRowsAndGraph(dev, *this, table_segment);
  SyncPredicate(dev, table_segment, program);
  int64_t count = 0;
  const int64_t dskip = (int64_t)std::min<size_t>(skip, (size_t)total_vector);   // (no rank reaches total_vector)
  if (eps_index_select(dev.h, dskip, limit, search_result_.data(), &count, nullptr) != EPS_OK)
    throw std::runtime_error(std::string("gfx950 executor: select: ") + eps_index_last_error(dev.h));
  result_size = count;
  return true;
}

}  // namespace execution
}  // namespace engine
}  // namespace vectordb

std::string epsdrop::BuildGraphOnMirror(const float* column, int64_t n, int64_t dim, int metric, const void* owner, int64_t** off, int64_t** nbr,
                                        int64_t* nav, std::shared_ptr<void>* keep) {
  using vectordb::engine::execution::DeviceField;
  std::shared_ptr<DeviceField> devp = vectordb::engine::execution::AcquireFieldForBuild(column, dim, metric);
  if (!devp) return "no usable gfx950 device (libepsilla_gfx950 has no CPU fallback)";
  DeviceField& dev = *devp;
  // The build must not hold the field's serving lock (at 10M rows eps_index_build is minutes, and every Search / RunSearch
  // of the field takes dev.mu): under the lock only the rows the mirror does not hold yet are uploaded and rows [0, n) are copied
  // device to device into a SIDE index (eps_index_clone_rows: 30 GB in ~10 ms); the build then runs on that copy while the old index
  // and the old graph keep serving - what the reference's Rebuild does with its snapshot of rows [0, n) (table_mvp.cpp:133-195).
  // The finished index is adopted by the first search of the new segment's executors (AdoptPendingBuild).  If the copy does not fit
  // (tables beyond half of the HBM) the build runs in place under the lock, as in r3.
  // the build IN PLACE, on the serving index, dev.mu held (r3 behaviour): when a second copy of the rows does not fit, and when the side build
  // itself runs out of HBM (copy + build scratch + 8-bit mirror next to the serving index)
  auto build_in_place_locked = [&]() -> std::string {
    auto fail = [&](const char* what) { return std::string(what) + ": " + eps_index_last_error(dev.h); };
    if (dev.pending_h) {   // (a side build of an older segment that nobody adopted: it only holds HBM, and must not be adopted over this graph)
      eps_index_destroy(dev.pending_h);
      dev.pending_h = nullptr;
      dev.pending_owner = nullptr;
      dev.pending_n = -1;
    }
    if (eps_index_build(dev.h, n, nullptr) != EPS_OK) return fail("build");   // defaults = NSGConfig(45,50,300,100)
    dev.retired_owner = nullptr;
    if (dev.sharded) {
      *off = new int64_t[n + 1]();
      *nbr = new int64_t[1]();
      *nav = 0;
      dev.shard_graph_owner = owner;
      dev.shard_graph_n = n;
    } else {
      int64_t gn = 0, edges = 0;
      eps_index_graph_info(dev.h, &gn, &edges, nav);
      *off = new int64_t[gn + 1];
      *nbr = new int64_t[edges > 0 ? edges : 1];
      if (eps_index_get_graph(dev.h, *off, *nbr) != EPS_OK) {
        delete[] *off;
        delete[] *nbr;
        *off = *nbr = nullptr;
        return fail("get_graph");
      }
      dev.graph_owner = owner;   // the device index already holds this graph: the segment's executors need not upload it again
      dev.graph_n = n;
    }
    *keep = devp;
    return "";
  };
  eps_index* side = nullptr;
  {
    std::lock_guard<std::mutex> lk(dev.mu);
    auto fail = [&](const char* what) { return std::string(what) + ": " + eps_index_last_error(dev.h); };
    if (n > dev.attached) {   // only the rows the mirror does not hold yet cross PCIe
      const int32_t rc = dev.attached == 0 ? eps_index_attach_rows(dev.h, column, n) : eps_index_append_rows(dev.h, column + dev.attached * dim, n - dev.attached);
      if (rc != EPS_OK) return fail("row upload");
      dev.attached = n;
    }
    static const bool in_place = getenv("EPS_DROPIN_BUILD_IN_PLACE") && atoi(getenv("EPS_DROPIN_BUILD_IN_PLACE")) != 0;
    if (!in_place) {
      const int32_t rc = dev.sharded ? eps_index_create_sharded(dim, metric, dev.devices.data(), (int32_t)dev.devices.size(), &side)
                                     : eps_index_create(dim, metric, dev.devices[0], &side);
      if (rc != EPS_OK) side = nullptr;
      if (side && eps_index_clone_rows(side, dev.h, n) != EPS_OK) {   // (no room for a second copy of the rows)
        eps_index_destroy(side);
        side = nullptr;
      }
    }
    if (!side) return build_in_place_locked();
  }
  // ---- the build itself: on the side index, nobody waits for it
  auto sfail = [&](const char* what) {
    const std::string e = std::string(what) + ": " + eps_index_last_error(side);
    eps_index_destroy(side);
    return e;
  };
  if (eps_index_build(side, n, nullptr) != EPS_OK) {
    // (most likely HBM: the side copy fitted, the build next to the serving index did not) - once more in place, as r3 built every table
    eps_index_destroy(side);
    side = nullptr;
    std::lock_guard<std::mutex> lk(dev.mu);
    return build_in_place_locked();
  }
  if (dev.sharded) {
    *off = new int64_t[n + 1]();
    *nbr = new int64_t[1]();
    *nav = 0;
  } else {
    int64_t gn = 0, edges = 0;
    eps_index_graph_info(side, &gn, &edges, nav);
    *off = new int64_t[gn + 1];
    *nbr = new int64_t[edges > 0 ? edges : 1];
    if (eps_index_get_graph(side, *off, *nbr) != EPS_OK) {
      delete[] *off;
      delete[] *nbr;
      *off = *nbr = nullptr;
      return sfail("get_graph");
    }
  }
  {
    std::lock_guard<std::mutex> lk(dev.mu);
    if (dev.pending_h) eps_index_destroy(dev.pending_h);   // (a build whose segment was never searched)
    dev.pending_h = side;
    dev.pending_owner = owner;
    dev.pending_n = n;
  }
  *keep = devp;
  return "";
}
