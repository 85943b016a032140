/* epsilla_gfx950.h — C ABI of libepsilla_gfx950.so, the MI355X (gfx950 / CDNA4) implementation of
 * Epsilla's ANN hot path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * What each entry point replaces in the reference (paths relative to /root/reference/engine):
 *
 *   eps_index_create / destroy      VecSearchExecutor ctor + ExecutorPool slot
 *                                   (db/execution/vec_search_executor.cpp:29-73, executor_pool.hpp:10-31);
 *                                   metric selection = GetDistFunc (db/index/index.cpp:10-35)
 *   eps_index_attach_rows           the executor borrowing TableSegmentMVP::vector_tables_[f]
 *                                   (db/table_segment_mvp.hpp:85, alloc .cpp:106-111): row-major float[n][dim]
 *   eps_index_set_deleted           ConcurrentBitset bytes of table_segment->deleted_
 *                                   (utils/concurrent_bitset.cpp:9-18), read per Search() call (:839)
 *   eps_index_set_int_filter        the `ID < N`-class post-filter ExprEvaluator::LogicalEvaluate applies to
 *                                   result candidates (vec_search_executor.cpp:905-927, query/expr/expr_evaluator.cpp:170-258)
 *   eps_index_build                 ANNGraphSegment::BuildFromVectorTable (db/ann_graph_segment.cpp:201-242)
 *   eps_index_set_graph / get_graph the public CSR members offset_table_/neighbor_list_/navigation_point_
 *                                   (db/ann_graph_segment.hpp:44-49) the executor is constructed from
 *   eps_index_save_graph/load_graph ANNGraphSegment::SaveANNGraph (.cpp:156-199) / file ctor (.cpp:39-98),
 *                                   byte-identical `ann_graph_<field>.bin`
 *   eps_index_search                VecSearchExecutor::Search (.cpp:833-935) for a BATCH of queries: mode
 *                                   selection, SearchImpl (:518-715), BruteForceSearch (:717-768),
 *                                   PreFilterBruteForceSearch (:770-831), tail merge, post-filter; results are
 *                                   what the caller reads from search_result_ / distance_ (hpp:51-52)
 *   eps_index_select                VecSearchExecutor::SearchByAttribute's full scan (.cpp:1016-1029): the visible rows in row
 *                                   order, windowed by skip / limit
 *   eps_index_search_range          (new) every row within a distance of the query - what a filter `@distance < r` asks of a Search - with
 *                                   the count of such rows: the radius query the reference answers by guessing a limit
 *   eps_index_search_among          the row-by-row loops in which SearchByAttribute judges a primary-key list or a geo index's id list
 *                                   (db/execution/vec_search_executor.cpp:966-1013), with a distance and a top-k on top: the k closest
 *                                   of the rows the CALLER names - the allow-list search, the second stage of a hybrid search
 *   eps_index_search_groups         (new) the k closest groups of rows, each by its closest row; the reference's relative is the host-side
 *                                   grouping of a finished answer (FacetExecutor, db/execution/aggregation.hpp) - it has no grouped search
 *   eps_index_search_group_rows     (new) ... and of each of those groups its m closest rows and the number of its visible rows: the
 *                                   `group_size` of a grouped search; the reference has no relative
 *   eps_index_search_multi          (new) the k closest groups for a query that is itself several vectors, by the sum over them of the distance
 *                                   to the group's closest row - the late-interaction score of a chunk table; the reference has no relative
 *   eps_index_search_diverse        (new) k rows of a flat search's fetch_k closest (or of the caller's lists) by maximal marginal relevance:
 *                                   close to the query, far from each other; the reference has no relative
 *   eps_sparse_index_*              BruteForceSearch over a SPARSE_VECTOR_FLOAT field: GetL2DistSqr / GetCosineDist / GetInnerProductDist
 *                                   (db/vector.cpp:7-96) row by row, as an exact scan of a CSR table; for dot and cosine also term at a
 *                                   time on inverted lists built on request (eps_sparse_index_build_inverted), the same bits
 *   eps_normalize_rows              Normalize (db/vector.cpp:60-69) and the insert-time normalisation
 *                                   (db/table_segment_mvp.cpp:574-587)
 *   eps_merge_topk                  (new) merges per-shard top-k lists after the RCCL all-gather
 *   eps_merge_range / _packed       (new) joins the answers G shards gave to one eps_index_search_range into the unsharded table's answer
 *   eps_merge_select                (new) the same for eps_index_select: a window over the shards' ordered ids, and the totals added up
 *   eps_exchange_allgather_merge_range  (new) the exchange step of a sharded radius search: one all-gather, one merge launch
 *                                   The reference has no counterpart of these: it does not shard a table
 *
 * Pointer arguments documented "host or device" are classified with hipPointerGetAttributes; device
 * pointers are used in place (no copy) on the index's stream.  WHEN an array is read:
 *   - a HOST array passed to any call has been read when the call returns, whatever kind its outputs are (page-locked memory included: the
 *     caller may refill it at once);
 *   - a DEVICE array is read at the call's place in the index's stream (eps_index_set_stream) and must stay valid, and unchanged, until the
 *     stream has reached that place; a device array a call installs (eps_index_attach_rows, _set_deleted, _set_int_filter,
 *     _set_filter_program) is borrowed and read, in place, by every later call at ITS place in the stream.
 * Every function returns a status code
 * from the reference's own table (utils/error.hpp:11-41): 0 = OK.  Calls on one handle must not overlap
 * (same contract as one VecSearchExecutor: one thread per executor instance); different handles are
 * independent.  The library never falls back to a CPU path: without a usable gfx950 device
 * eps_index_create fails with EPS_INFRA_UNEXPECTED_ERROR.
 */
#ifndef EPSILLA_GFX950_H_
#define EPSILLA_GFX950_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes: utils/error.hpp:11-41 */
#define EPS_OK 0
#define EPS_USER_ERROR 30000
#define EPS_INFRA_UNEXPECTED_ERROR 40001
#define EPS_DB_UNEXPECTED_ERROR 50001
#define EPS_DB_UNSUPPORTED_ERROR 50002
#define EPS_NOT_IMPLEMENTED_ERROR 50009
#define EPS_INVALID_PAYLOAD 50400

/* meta::MetricType (db/catalog/meta_types.hpp:44-50) as used by GetDistFunc; "smaller = closer" for all:
 * EUCLIDEAN -> squared L2, COSINE -> 1 - dot (rows/queries normalised by the caller or eps_normalize_rows),
 * DOT_PRODUCT -> -dot. */
#define EPS_METRIC_EUCLIDEAN 0
#define EPS_METRIC_COSINE 1
#define EPS_METRIC_DOT_PRODUCT 2

/* search modes */
#define EPS_MODE_REFERENCE 0 /* VecSearchExecutor::Search's own mode selection (:855-935)          */
#define EPS_MODE_FLAT 1      /* exact flat scan of [0,n_total) (the BruteForceSearch answer for any n) */
#define EPS_MODE_GRAPH 2     /* graph traversal + tail even when n_indexed < BruteforceThreshold       */

/* flat-scan engines (EPS_MODE_FLAT, and the flat branches of EPS_MODE_REFERENCE) */
#define EPS_FLAT_AUTO 0
#define EPS_FLAT_STREAM 1 /* fp32 streaming scan, HBM-bound; any batch size                            */
#define EPS_FLAT_MFMA 2   /* fp16-MFMA lower-bound filter over a device-side half mirror + exact fp32
                             re-rank; returns the same exact answer; for large batches                 */
#define EPS_FLAT_MFMA_I8 3 /* the same with an int8 mirror as the filter's operand (twice the matrix rate,
                             half the mirror; the bound is computed from the stored residuals, so the
                             answer is again the exact one); tables an 8-bit grid cannot serve and batches
                             whose candidate lists overflow run the fp16 pass.  EPS_FLAT_AUTO picks this
                             form when it picks the matrix engine.                                     */

/* filter comparison operators for eps_index_set_int_filter */
#define EPS_OP_NONE 0
#define EPS_OP_LT 1
#define EPS_OP_LE 2
#define EPS_OP_EQ 3
#define EPS_OP_GE 4
#define EPS_OP_GT 5
#define EPS_OP_NE 6

/* Compiled filter: a postfix program over the packed attribute row of a candidate
 * (TableSegmentMVP::attribute_table_, rows of primitive_offset_ bytes), evaluated on a stack of doubles exactly as
 * ExprEvaluator::NumEvaluate / LogicalEvaluate do (query/expr/expr_evaluator.cpp:127-258): every number is a double,
 * comparisons and AND / OR / NOT produce 0 / 1, the row passes iff the final value is non-zero.  PUSH_* take `arg` = byte
 * offset of the attribute inside the row; PUSH_CONST takes `dval`; PUSH_DIST is the candidate's distance (`@distance`). */
#define EPS_FOP_PUSH_CONST 1
#define EPS_FOP_PUSH_DIST 2
#define EPS_FOP_PUSH_I8 3
#define EPS_FOP_PUSH_I16 4
#define EPS_FOP_PUSH_I32 5
#define EPS_FOP_PUSH_I64 6
#define EPS_FOP_PUSH_F32 7
#define EPS_FOP_PUSH_F64 8
#define EPS_FOP_PUSH_BOOL 9   /* true iff the byte is non-zero (expr_evaluator.cpp:56-59) */
#define EPS_FOP_ADD 10
#define EPS_FOP_SUB 11
#define EPS_FOP_MUL 12
#define EPS_FOP_DIV 13
#define EPS_FOP_MOD 14        /* fmod */
#define EPS_FOP_LT 15
#define EPS_FOP_LE 16
#define EPS_FOP_EQ 17
#define EPS_FOP_NE 18
#define EPS_FOP_GE 19
#define EPS_FOP_GT 20
#define EPS_FOP_AND 21
#define EPS_FOP_OR 22
#define EPS_FOP_NOT 23
#define EPS_FOP_EQ_BOOL 24    /* EQ / NE between boolean operands (:206-209) */
#define EPS_FOP_NE_BOOL 25
typedef struct eps_filter_op {
  int32_t op;
  int32_t arg;
  int64_t ival; /* reserved */
  double dval;
} eps_filter_op;

typedef struct eps_index eps_index; /* opaque */

/* Search knobs; mirror vectordb::Config (config/config.hpp:17-25) and the executor ctor arguments. */
typedef struct eps_search_params {
  int32_t mode;            /* EPS_MODE_*                                                       */
  int32_t flat_engine;     /* EPS_FLAT_*                                                       */
  int32_t prefilter;       /* Config::PreFilter: flat scan with the filter applied first        */
  int32_t intra_threads;   /* Config::IntraQueryThreads (T); the device runs T candidate
                              expansions of a query concurrently per round (1 = the reference's
                              deterministic single-thread order)                               */
  int64_t master_queue;    /* Config::MasterQueueSize (L)                                      */
  int64_t local_queue;     /* Config::LocalQueueSize (result cap, :872)                        */
  int64_t sync_interval;   /* Config::GlobalSyncInterval (expansions per worker per round)     */
  int32_t filter_in_traversal; /* 0 (default): the reference's semantics - deleted rows and the filter are judged on the
                              final top-L walk only (vec_search_executor.cpp:905-927), so a selective filter returns fewer than
                              `limit` rows.  1 (NOT the reference's answer): graph searches judge every row
                              they EVALUATE and return the closest visible ones; invisible rows still steer the walk.          */
  int32_t reserved;
} eps_search_params;

/* Build knobs; defaults = NSGConfig(45,50,300,100) (db/ann_graph_segment.cpp:29). */
typedef struct eps_build_params {
  int64_t search_length;
  int64_t out_degree;
  int64_t candidate_pool_size;
  int64_t knng;
  uint32_t seed;      /* rand_r state the NSG stage starts from (nsg.cpp:19 uses 100) */
  int32_t reserved;
} eps_build_params;

/* counters of the last eps_index_search call (the reference's commented-out
 * count_distance_computation_, vec_search_executor.hpp:162, revived) */
typedef struct eps_search_stats {
  int64_t dist_evals;       /* distance evaluations, summed over the batch                 */
  int64_t expansions;       /* graph nodes expanded, summed over the batch                 */
  int64_t rerank_rows;      /* rows re-ranked in exact fp32 by the MFMA engine             */
  int64_t overflow_queries; /* queries that fell back from the MFMA filter to the fp32 scan */
  double kernel_ms;         /* device time of the call measured with hipEvents on its stream */
  double main_kernel_ms;    /* device time of the dominant kernel only                      */
  int64_t main_kernel_launches;
  int64_t main_kernel_rows; /* rows covered by the launch timed in main_kernel_ms              */
  int64_t main_kernel_queries; /* queries covered by that launch (large batches run in slices)  */
  int64_t main_kernel_bits; /* operand width of that launch: 32 (fp32 stream / traversal), 16 or 8 (matrix engine) */
  double filter_ms_all;     /* device time of ALL filter-stage launches of the call (the dominant kernel runs once per stage; r4) */
  int64_t filter_rows_all;  /* rows those launches covered, summed (x main_kernel_queries = the call's matrix work)              */
  int64_t i8_folded;        /* 1: the 8-bit pass of this call ran with per-row margins folded into the rows' start values (a table whose rows differ: clamped / forced outlier rows; r4) */
  int64_t i8_declined;      /* 1: this call probed the 8-bit pass on this table, found its bound too loose for the data and ran the fp16 pass (r4) */
  int64_t one_pass;         /* 1: a handful of queries (<= 32, k <= 64; a deleted bitset, an int-column test or a compiled filter program) answered by ONE streaming pass over the 8-bit mirror + one re-rank (stream8_kernel.hpp) instead of the staged filter chain (r4) */
  int64_t i8_rotated;       /* 1: the 8-bit pass of this call ran in the table's ROTATED frame: rows and queries quantised as R x, R a fixed orthogonal map (signs, a permutation, 256-point Walsh-Hadamard blocks) - distances do not change, the grid's step and with it the bound's margin shrink on tables whose energy sits in a few columns (unit-norm embedding rows); chosen per table when its mirror is built (r6) */
} eps_search_stats;

void eps_default_search_params(eps_search_params* p);
void eps_default_build_params(eps_build_params* p);

int32_t eps_index_create(int64_t dim, int32_t metric, int32_t device, eps_index** out);
/* Hash-sharded index over `shards` GPUs of THIS process: row i of the table lives on shard i mod shards (device
 * devices[i mod shards]) as local row i / shards; every shard answers the whole batch on its rows, the per-shard top-k lists
 * are pushed peer to peer (xGMI) to the device that holds the caller's result buffers (devices[0] for host results) and merged
 * there.  The handle works with every eps_index_* entry point below.  Rows: a HOST table (eps_index_attach_rows: each shard reads
 * its rows with one strided copy) or, shard by shard, rows that already live on the shard's device (eps_index_attach_shard_rows).
 * Queries and results: host buffers, or (r4) device buffers on any device of the group - a shard on another device gets the
 * queries with one peer copy, the merge writes straight into the caller's ids / dist / counts (which must live together), and as
 * with a plain index the caller synchronises (eps_index_synchronize).  Bitsets, filter columns and attribute rows are host
 * buffers.  eps_index_build builds one graph per shard, eps_index_save/load_graph use <path>.shard<s> files; eps_index_set_graph
 * (one graph over the whole table), eps_index_set_stream and eps_index_search_walk are not available.
 * devices may repeat an ordinal (several shards on one GPU). */
int32_t eps_index_create_sharded(int64_t dim, int32_t metric, const int32_t* devices, int32_t shards, eps_index** out);
int32_t eps_index_destroy(eps_index* h);
const char* eps_index_last_error(const eps_index* h);
/* What kind of failure the last error was (r6; callers branch on this, never on the text).  EPS_ERRCLASS_DEVICE_RANGE: the request is valid for
 * the reference (config/config.hpp:28-44 accepts SearchQueueSize / LocalQueueSize up to 10^7 and IntraQueryThreads up to 128 at any
 * out-degree; VecSearchExecutor::Search, vec_search_executor.cpp:833-935, has no result cap) but lies outside what the device traversal runs
 * (queues <= 2^20 keys, IntraQueryThreads x out-degree <= 2048, <= 1024 rows per query under filter_in_traversal or when a graph result is
 * merged with an un-indexed tail): the same request with mode = EPS_MODE_FLAT is answered exactly, which is what the drop-in adapter does. */
#define EPS_ERRCLASS_OTHER 0
#define EPS_ERRCLASS_DEVICE_RANGE 1
int32_t eps_index_last_error_class(const eps_index* h);

/* use an existing HIP stream (hipStream_t passed as void*); NULL = the index's own non-blocking stream,
 * hipStreamLegacy ((void*)1) = the legacy default stream.  Device buffers handed to the index (rows, queries,
 * outputs, bitsets, columns) must be ready on the index's stream: share the producer's stream or synchronise
 * the producer before the call. */
int32_t eps_index_set_stream(eps_index* h, void* hip_stream);
int32_t eps_index_synchronize(eps_index* h);

/* rows: host or device, row-major float[n][dim].  Host rows are copied to HBM; device rows are
 * borrowed (caller keeps them alive and immutable for [0,n)).  Replaces any previous attachment. */
int32_t eps_index_attach_rows(eps_index* h, const float* rows, int64_t n);
/* rows beyond the current count (the un-indexed tail, :885-900); only for host-attached (owned) stores */
int32_t eps_index_append_rows(eps_index* h, const float* rows, int64_t n_new);
/* rows of ONE shard of a hash-sharded index: local row l is global row l * shards + shard; host memory (copied) or memory of the
 * shard's own device (borrowed).  Once every shard holds its rows the table has sum(n_local) rows; the counts must be the hash
 * split of that sum (shard s holds ceil((n - s) / shards) rows) or searches and builds fail with EPS_USER_ERROR.  On a plain index
 * shard 0 is the index itself.  (r4; replaces what TableSegmentMVP::vector_tables_ is for one GPU, table_segment_mvp.hpp:85) */
int32_t eps_index_attach_shard_rows(eps_index* h, int32_t shard, const float* rows, int64_t n_local);
/* dst gets its OWN device copy of the first n rows of src - an index of the same kind on the same device(s): plain / plain, or two
 * shard groups over the same device list - with one device-to-device copy per shard; replaces dst's rows like eps_index_attach_rows.
 * What TableMVP::Rebuild's snapshot is for the reference (table_mvp.cpp:133-156: the build works on rows [0, n) while inserts and
 * searches go on): the drop-in builds the new graph on such a copy and swaps it in, so a rebuild never blocks queries (r4). */
int32_t eps_index_clone_rows(eps_index* dst, eps_index* src, int64_t n);
int64_t eps_index_row_count(const eps_index* h);

/* On-disk table segment of the reference (`<db>/<table_id>/data_mvp.bin`, TableSegmentMVP::SaveTableSegment,
 * db/table_segment_mvp.cpp:939-1010) read straight into HBM: header (record count, first id), deleted
 * bitset, packed attribute rows (record_count x primitive_offset bytes), variable-length attributes (skipped), then one
 * float[record_count][dim] table per dense vector field.  The caller describes the schema-dependent sizes; the index takes
 * the rows of dense field `field` (its dim must equal the index's), the deleted bitset, and keeps the attribute rows on the
 * device for eps_index_set_filter_program(ops, nops, NULL, 0, 0).  *n_out = record count. */
typedef struct eps_table_layout {
  int64_t primitive_offset;   /* bytes per packed attribute row (TableSegmentMVP::primitive_offset_)            */
  int32_t var_len_attrs;      /* strings / sparse vectors per record (var_len_attr_num_)                       */
  int32_t dense_fields;       /* dense vector fields, in schema order (dense_vector_num_)                      */
  const int64_t* dense_dims;  /* their dimensions (vector_dims_)                                                */
  int32_t field;              /* which of them to load                                                          */
  int32_t reserved;
} eps_table_layout;
int32_t eps_index_load_table(eps_index* h, const char* data_mvp_path, const eps_table_layout* layout, int64_t* n_out);

/* global id = local row index * stride + base (hash sharding by row index: stride = #shards, base = rank) */
int32_t eps_index_set_id_map(eps_index* h, int64_t base, int64_t stride);

/* deleted: host or device bitset, bit (i&7) of byte (i>>3); nbytes >= ceil(n/8); NULL clears */
int32_t eps_index_set_deleted(eps_index* h, const uint8_t* bits, int64_t nbytes);
/* integer attribute column: value of row i at column + i*stride_bytes, width_bytes in {1,2,4,8}, signed;
 * host or device; rows failing `value <op> constant` are filtered. EPS_OP_NONE clears. */
int32_t eps_index_set_int_filter(eps_index* h, const void* column, int64_t stride_bytes, int32_t width_bytes,
                                 int32_t op, int64_t constant);

/* compiled filter program (see eps_filter_op): `rows` = packed attribute rows (host or device), row i at rows + i*stride_bytes,
 * n_rows of them.  Replaces eps_index_set_int_filter's filter; nops = 0 clears.  A row is visible iff it is not deleted
 * and the program leaves a non-zero value.  Programs are limited to 64 instructions and a stack depth of 16.  Host rows
 * are copied to the device, all of them, on every call. */
int32_t eps_index_set_filter_program(eps_index* h, const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride_bytes,
                                     int64_t n_rows);
/* The same with flags.  EPS_FILTER_ROWS_APPEND_ONLY: the caller promises that the host rows it handed over before FROM THIS
 * POINTER (same stride, same table attached) have not changed since - TableSegmentMVP::attribute_table_ is such a table: an
 * update is delete + insert (db/table_segment_mvp.cpp:476-587) - so only the rows beyond those already on the device are
 * uploaded.  Re-attaching rows (eps_index_attach_rows) forgets the cached copy. */
#define EPS_FILTER_ROWS_APPEND_ONLY 1
int32_t eps_index_set_filter_program_ex(eps_index* h, const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride_bytes,
                                        int64_t n_rows, int32_t flags);

/* graph over rows [0,n): built on the device, or supplied / exported as the reference's CSR */
int32_t eps_index_build(eps_index* h, int64_t n, const eps_build_params* p);
/* One stage of the build on its own: NsgIndex::SyncPrune's sort + SelectEdge (db/index/nsg/nsg.cpp:557-567, 655-685) for
 * caller-supplied candidate lists.  Node nodes[i] with candidates cands[i][0..cands_per_node) (-1 = none; the node itself is
 * skipped): candidates sorted by (L2 distance to the node, id), the closest kept, every further one of the first `depth`
 * (candidate_pool_size; <= 0 = all) kept iff no kept neighbour is closer to it than the node is (MRNG rule), at most out_degree.
 * out_ids [m][out_degree] (-1 padded), out_deg [m]; host arrays. */
int32_t eps_index_select_edges(eps_index* h, const int64_t* nodes, int64_t m, const int64_t* cands, int32_t cands_per_node,
                               int32_t depth, int32_t out_degree, int64_t* out_ids, int32_t* out_deg);
/* Another stage on its own: NsgIndex::InterInsert (db/index/nsg/nsg.cpp:583-653) over all n = row-count nodes, on caller-supplied
 * edge lists ids [n][out_degree] with deg[v] valid entries each (what Link leaves).  Every edge v->u offers v to u; u keeps its
 * own edges plus the offers if they fit into out_degree, otherwise SelectEdge(limit = false) over all of them sorted by (L2
 * distance, id) - applied once per node to the whole candidate set (the reference applies it incrementally in node order, which
 * differs where a list overflows: see DESIGN.md 3.4).  Every offer is considered (kept in a CSR by receiving node), so the result
 * does not depend on the order in which the device produces them.  out_ids [n][out_degree] (-1 padded), out_deg [n]; host arrays. */
int32_t eps_index_inter_insert(eps_index* h, const int64_t* ids, const int32_t* deg, int64_t n, int32_t out_degree, int64_t* out_ids,
                               int32_t* out_deg);
/* The first stage on its own: the K-nearest-neighbour graph of rows [0,n) that the build links (the reference's KNNGraph /
 * NN-Descent stage, db/index/knn/knn.hpp:90-135; K = p->knng).  out_ids [n][min(K, n-1)] host, closest first, -1 padded, the node
 * itself excluded.  Exact below 65 536 rows; above, the 128 closest by approximate key re-ranked in exact fp32. */
int32_t eps_index_knn_graph(eps_index* h, int64_t n, const eps_build_params* p, int64_t* out_ids);
/* The Link stage on its own (NsgIndex::Link without InterInsert, db/index/nsg/nsg.cpp:488-516: per node GetNeighbors :158-268 on the
 * kNN graph from the navigation node's first search_length neighbours, then SyncPrune :540-580 = pool + the node's own kNN row,
 * sorted, SelectEdge over the first candidate_pool_size).  knn: [n][min(p->knng, n-1)] host (NULL: the device's own kNN stage);
 * navigation_point < 0: the closest row to the centroid (reported in *nav_out).  out_ids [n][out_degree] (-1 padded), out_deg [n]. */
int32_t eps_index_link(eps_index* h, int64_t n, const int64_t* knn, int64_t navigation_point, const eps_build_params* p, int64_t* out_ids,
                       int32_t* out_deg, int64_t* nav_out);
/* Two stages of the flat matrix engine on their own (r7), so that a test can hand the device and an fp64 reference identical inputs
 * (tests/mirror_ref.py, tests/test_gpu_mirror_pin.py).  Single-device indices only; host arrays; nothing a later search could see changes
 * (statistics, engine choices) - a mirror that a search would have built is built.
 *
 * A view of a mirror: builds or extends the mirror of width `bits` (8 | 16) exactly as a search would, prepares the nq <= 2048 queries exactly
 * as the staged chain would (8-bit: on the table's grid and in its frame, with the table's own fold decision), and copies what the kernels read
 * into the host buffers that are not NULL.  The scalars are always filled in: call once with every buffer NULL for the sizes.  Per-row buffers
 * hold n_pad rows (the padding rows included), x holds n_pad x d_pad elements (8-bit: int8 codes; 16: fp16), q holds nq x d_pad.
 *   8-bit: x, acc0, erow, hrow, mu [d_pad], sp [d_pad] (rotated frame only: source column, bit 31 = negative sign), scal [8], scalf [8] (scal
 *          with the two margin entries zeroed: what thresholds of folded launches read), q, qstat [nq][4]; when the table folds: acc0b (the start
 *          values with THIS batch's per-row margins) and qmax [2] (float bits of the batch's largest |q'| and |q' - qh'|).  usable = 0: the table
 *          does not fit one grid, nothing is copied.
 *   fp16:  x, xn (|x|^2), start (the accumulators' start values: -|x|^2 / 2 for L2, 0 otherwise, -inf on padding rows), scal [4], q, qstat. */
typedef struct eps_mirror_view {
  int64_t n, n_pad;          /* out: rows mirrored; rows of the padded mirror                                              */
  int64_t forced_rows;       /* out, 8-bit: rows whose constant leaves the accumulator's range (always passed)             */
  int64_t extended_rows;     /* out: rows converted by extensions after an append                                          */
  int32_t d_pad;             /* out: elements per mirror row                                                               */
  int32_t usable;            /* out: the table has a usable mirror of this width (8: one grid fits; 16: values in range)   */
  int32_t rot, rot_w, fold;  /* out, 8-bit: rotated frame, columns it covers, per-row margins folded per batch             */
  int32_t version;           /* out (nq > 0): filter kernel the chain launches for this shape, 3 | 7                       */
  float step;                /* out, 8-bit: the grid's step                                                                */
  float slack;               /* out: relative fp32 allowance of the thresholds (rerank_slack)                              */
  void* x;
  int32_t* acc0;
  int32_t* acc0b;
  float* erow;
  float* hrow;
  float* mu;
  int32_t* sp;
  float* scal;
  float* scalf;
  uint32_t* qmax;
  float* xn;
  float* start;
  void* q;
  float* qstat;
} eps_mirror_view;
int32_t eps_index_mirror_view(eps_index* h, int32_t bits, const float* queries, int64_t nq, eps_mirror_view* view);
/* One filter pass with imposed thresholds: plan_chain -> prepare_queries -> thresholds -> ONE launch of the filter kernel over rows
 * [row_lo, row_hi) (row_lo a multiple of 256, row_hi <= rows) with the arguments the chain itself would build (v3 / v7, 128- or 256-query tiles,
 * group counters, folded start values); no re-rank, no fall-back.  mode: EPS_PASS_IDS (exact mode's lists of row ids, uint32), EPS_PASS_KEYS
 * (approx mode's (approximate distance, row) keys, uint64: order-preserving image of the fp32 distance << 32 | row) or EPS_PASS_DENSE (the seed
 * pass: the key of EVERY row of the range in slot row - row_lo, no test; v7 shapes, cap >= row_hi - row_lo).  thr: one value per query -
 * EPS_THR_RAW: T in the kernel's own unit (int32 for 8-bit operands: a row passes iff its accumulator >= T; float for fp16: iff its approximate key
 * <= T), used as it is; EPS_THR_DISTANCE: a distance (float), turned into T by the device as a stage's k-th best key would be, with the table's own
 * choice of maxima.  T_out [nq] (may be NULL): the T used.  cnt_out [nq]: rows that passed (counted beyond cap); cand_out [nq][cap]: the first
 * min(cnt, cap) entries of every list are valid, in no particular order. */
#define EPS_PASS_IDS 0
#define EPS_PASS_KEYS 1
#define EPS_PASS_DENSE 2
#define EPS_THR_RAW 0
#define EPS_THR_DISTANCE 1
int32_t eps_index_filter_pass(eps_index* h, const float* queries, int64_t nq, int32_t bits, int64_t row_lo, int64_t row_hi, int64_t cap, int32_t mode,
                              int32_t thr_form, const void* thr, void* T_out, uint32_t* cnt_out, void* cand_out);
/* The pass of the one-pass search on its own, so that a test can hold what it leaves behind to an integer reference (tests/one_pass_ref.py,
 * tests/test_gpu_one_pass_pin.py).  Single-device indices only; host arrays.  Does what the next eps_index_search(queries, nq, k, EPS_MODE_FLAT,
 * EPS_FLAT_MFMA_I8) with default parameters would do up to and including the launch of the pass - the entry rule, the mirror's build or extension,
 * the mask launch under a filter program, the prep launch (or none: the "clean" second call of 1-2 queries quantises them in the pass), the fold
 * launch on a table that folds per-row margins, the pass in the form the shape selects - and NO re-rank launch, and copies out what the pass left:
 *   form     which instantiation ran (below)
 *   raw_cnt  [nq][waves]            entries every wavefront found for every query (counted beyond wave_cap)
 *   raw      [nq][waves][wave_cap]  every wavefront's private list as stored: (accumulator << 32) | row; the first min(count, wave_cap) are valid
 *   table    [nq][slots]            the final table of best accumulators (INT32_MIN: an empty slot)
 *   qstat    [nq][4]                the queries' constants as the pass used them (clean form: as workgroup 0 of the pass wrote them)
 *   kth, T_final [nq]               the k-th largest slot (INT32_MIN: fewer than k filled) and the threshold the re-rank's selection would apply,
 *                                   computed on the device from the final table by the function that selection calls
 * raw_cnt, raw and table are written densely for the `waves` and `slots` the form reports; the caller provides room for
 * EPS_ONE_PASS_MAX_WAVES wavefronts, EPS_ONE_PASS_WAVE_CAP entries and EPS_ONE_PASS_MAX_SLOTS slots.
 * EPS_DB_UNSUPPORTED_ERROR: that search would not take the one-pass form (the entry rule - fewer than 65 536 rows, dim > 1024, k > 64, nq > 32, more
 * than 16 queries on a folding or a large table -, a form the table has been declined for, filtered calls being sent to the staged chain, a filter
 * program that reads @distance, a table without a usable 8-bit mirror): a probe never runs anything else in its place.  Afterwards the next one-pass
 * search starts with its prep launch; nothing else a later search could see changes (statistics, declined forms, the count of filtered calls to skip). */
#define EPS_ONE_PASS_MAX_WAVES 8192
#define EPS_ONE_PASS_WAVE_CAP 32
#define EPS_ONE_PASS_MAX_SLOTS 128
typedef struct eps_one_pass_form {
  int32_t pieces;          /* 256-byte pieces of a mirror row: 2 | 3 | 4                                                   */
  int32_t matrix;          /* 0: the v_dot4 kernel (1-4 queries), 1: the matrix-core kernel                                */
  int32_t width;           /* v_dot4: queries the kernel is built for, 1 | 2 | 4; matrix: 16-query column blocks, 1 | 2    */
  int32_t wide;            /* v_dot4 with the 128-slot table (k = 17..64, 1-2 queries)                                     */
  int32_t prep_in_kernel;  /* the pass quantised its queries itself: no prep launch                                        */
  int32_t slots, waves;    /* table slots per query (64 | 128); wavefronts of the launch                                   */
  int32_t fold, rot;       /* per-row margins folded into the start values; the table's grid lies in the rotated frame     */
  int32_t masked;          /* a filter program was evaluated into a bitset by the mask launch                              */
  int32_t wave_cap;        /* entries a wavefront's list holds                                                             */
  int32_t chunk;           /* consecutive rows a wavefront takes per step: row r belongs to wavefront (r / chunk) % waves  */
} eps_one_pass_form;
int32_t eps_index_one_pass_probe(eps_index* h, const float* queries, int64_t nq, int32_t k, eps_one_pass_form* form, uint32_t* raw_cnt, uint64_t* raw,
                                 int32_t* table, float* qstat, int32_t* kth, int32_t* T_final);
int32_t eps_index_set_graph(eps_index* h, int64_t n, const int64_t* offsets, const int64_t* neighbors,
                            int64_t navigation_point);
int32_t eps_index_graph_info(const eps_index* h, int64_t* n, int64_t* edges, int64_t* navigation_point);
int32_t eps_index_get_graph(const eps_index* h, int64_t* offsets, int64_t* neighbors);
int32_t eps_index_save_graph(eps_index* h, const char* path);
int32_t eps_index_load_graph(eps_index* h, const char* path);

/* queries: host or device float[nq][dim]; ids_out int64[nq][k], dist_out float[nq][k], counts_out
 * int32[nq] (host or device, all three the same kind).  Unused slots are id -1 / +inf.
 * COSINE queries must already be normalised (TableMVP::Search does it, table_mvp.cpp:333-349). */
int32_t eps_index_search(eps_index* h, const float* queries, int64_t nq, int32_t k, const eps_search_params* p,
                         int64_t* ids_out, float* dist_out, int32_t* counts_out);
/* The candidates the reference's post-filter loop walks (vec_search_executor.cpp:905-927), for filters that only the host
 * DBMS can evaluate (strings, LIKE, IN, geo): same traversal / flat scan, same tail merge with searchLimit =
 * min(n_indexed, limit, L_local) (:872-900), deleted rows and device-side filters already removed, in walk order; at most
 * `cap` per query (cap >= limit).  ids_out [nq][cap], dist_out [nq][cap], counts_out [nq].  The caller applies its
 * predicate to these <= cap candidates and keeps the first `limit` that pass - O(L) host work as in the reference,
 * instead of O(N). */
int32_t eps_index_search_walk(eps_index* h, const float* queries, int64_t nq, int32_t limit, int32_t cap, const eps_search_params* p,
                              int64_t* ids_out, float* dist_out, int32_t* counts_out);
/* VecSearchExecutor::SearchByAttribute's full-scan branch (db/execution/vec_search_executor.cpp:1016-1029) - the path behind DBServer::Project,
 * the client's `get` without a primary-key list: the rows of [0, eps_index_row_count) that are not deleted and pass the filter (whatever
 * eps_index_set_deleted, eps_index_set_int_filter and eps_index_set_filter_program last installed; `@distance` reads as 0, as
 * LogicalEvaluate(root, id) evaluates it there), in ascending row order; those of rank [skip, skip + limit) among them are written as
 * ids_out[rank - skip] = row * stride + base (eps_index_set_id_map).  *count_out = clamp(total - skip, 0, limit) ids were written;
 * *total_out (may be NULL) = the visible rows of the whole table, a `count where` for free.  ids_out [limit], count_out [1], total_out [1]:
 * host or device, all the same kind - device: asynchronous on the index's stream; host: the call synchronises, as eps_index_search does.
 * limit = 0 or an empty table: count 0.  Negative skip / limit: EPS_USER_ERROR.  A sharded handle: EPS_DB_UNSUPPORTED_ERROR.  Nothing a later
 * search can observe changes (filters, statistics, engine choices).  Three launches (csrc/select.hip): verdict bitset + block counts, scan
 * of the counts, scatter of the window - the reference's loop is serial over all rows (`TODO: leverage multithread to accelerate`, :945). */
int32_t eps_index_select(eps_index* h, int64_t skip, int64_t limit, int64_t* ids_out, int64_t* count_out, int64_t* total_out);
/* Radius search: for every query j the rows that are visible - not deleted, passing the int-column test and the installed program, exactly as for
 * eps_index_search - and whose exact fp32 distance is <= radius[j].  The exact fp32 distance is the value eps_index_search in EPS_MODE_FLAT returns
 * for that (row, query), bit for bit; a program's `@distance` reads the same value, on every engine.  queries: host or device float[nq][dim]
 * (COSINE: already normalised); radius: HOST float[nq], NaN is EPS_USER_ERROR, +inf is allowed.  totals_out[j] (may be NULL) = the number of such
 * rows, whatever cap is; counts_out[j] = min(total, cap); ids_out[j][0 .. count) / dist_out[j][0 .. count) = the count smallest in ascending
 * (distance, id) order - the library's one key order, ids through eps_index_set_id_map - the unused slots -1 / +inf.  So total <= cap: the answer
 * is complete; total > cap: the cap closest, and the caller knows how many are missing.  ids_out [nq][cap], dist_out [nq][cap], counts_out [nq]
 * (may be NULL), totals_out [nq]: host or device, all the same kind - device: on the index's stream, the caller synchronises; host: the call
 * synchronises.  1 <= cap <= 8192 (one workgroup orders a query's keys in LDS); nq = 0: EPS_OK; an empty table: counts and totals 0.  p: only
 * flat_engine is read (NULL: defaults) - EPS_FLAT_STREAM scans the fp32 rows; EPS_FLAT_MFMA / EPS_FLAT_MFMA_I8 run ONE launch of the lower-bound
 * filter over the fp16 / 8-bit mirror with thresholds from the radii, then give the rows that passed their exact distance (csrc/range.hip); a
 * table the mirror cannot serve falls to the next form, as in a search; EPS_FLAT_AUTO chooses as a search does.  All forms return the same bits.
 * A query whose candidate list overflowed runs again on the stream form, one whose total exceeds cap takes its cap closest from the flat scan:
 * both are counted in eps_search_stats::overflow_queries; no list ever silently loses a row.  eps_index_last_stats reports the call like a search
 * (main_kernel_*, main_kernel_bits 8 / 16 / 32, rerank_rows = candidates given an exact distance; main_kernel_ms times the pass - the filter launch
 * of the last slice of 2048 queries, or the stream scan - never a fall-back's scan).  A sharded handle: EPS_DB_UNSUPPORTED_ERROR;
 * after an append, a stale bitset / column / attribute rows: EPS_USER_ERROR.  Nothing a later search can observe changes. */
int32_t eps_index_search_range(eps_index* h, const float* queries, int64_t nq, const float* radius, int32_t cap, const eps_search_params* p,
                               int64_t* ids_out, float* dist_out, int32_t* counts_out, int64_t* totals_out);
/* Search among given rows: for every query j the k smallest (distance, id) keys over the VISIBLE rows its candidate list names - the exact k-NN of
 * an allow list, without a scan of the table and without a bitset of n / 8 bytes.  cand_offsets == NULL: the ONE list cand_ids[0 .. n_cand) serves
 * every query; else cand_offsets is a HOST int64[nq + 1], non-decreasing, [0] = 0, [nq] = n_cand (anything else: EPS_USER_ERROR), and query j's
 * list is cand_ids[cand_offsets[j] .. cand_offsets[j + 1]) - two queries of one batch may have different candidate sets.  cand_ids: host (copied
 * on the index's stream) or device (used in place) int64[n_cand], 0 <= n_cand < 2^31.  Ids are global (eps_index_set_id_map): an id names row
 * (id - base) / stride; an id that names no row - negative, below base, (id - base) % stride != 0, a row >= eps_index_row_count - is ignored, as
 * PK2ID returning false is in the reference (:972); a row named several times is judged and returned once.  Visible means not deleted, passing
 * the int-column test and the installed program, exactly as for eps_index_search; `@distance` reads the row's exact distance.  The distance is,
 * bit for bit, the value eps_index_search in EPS_MODE_FLAT returns for that (row, query).  counts_out[j] (may be NULL) = min(k, distinct visible
 * rows of the list), the unused slots -1 / +inf, an empty list: count 0.  queries, ids_out [nq][k], dist_out [nq][k], counts_out [nq]: as for
 * eps_index_search - host or device, the outputs all of one kind; device: on the index's stream, the caller synchronises; host: the call
 * synchronises.  1 <= k <= 1024 (a caller who wants more from a list orders it itself); nq = 0: EPS_OK.  A sharded handle:
 * EPS_DB_UNSUPPORTED_ERROR; after an append, a stale bitset / column / attribute rows: EPS_USER_ERROR.  Two launches (csrc/among.hip): a gather
 * with the flat scan's blocking that takes its row pointers from the list - m * dim * 4 bytes of rows per 4 queries for a shared list of m
 * entries, the sum of m_j * dim * 4 for per-query lists, 8 bytes per id - and a merge of the wavefronts' lists that drops repeated keys.
 * eps_index_last_stats reports the call like a search: dist_evals = (row, query) pairs given a distance (the entries that name a row, times the
 * queries they serve), main_kernel_bits 32, main_kernel_rows = n_cand, main_kernel_queries = nq, main_kernel_ms = the gather.  Nothing a later
 * search can observe changes. */
int32_t eps_index_search_among(eps_index* h, const float* queries, int64_t nq, const int64_t* cand_ids, const int64_t* cand_offsets, int64_t n_cand,
                               int32_t k, int64_t* ids_out, float* dist_out, int32_t* counts_out);
/* Grouped search: the k closest GROUPS of rows per query, each represented by its closest row - the call behind "the k best documents" over a
 * table of chunks.  The reference has no such call: it groups answers by an attribute on the host after the search (FacetExecutor,
 * db/execution/aggregation.hpp), and a caller of eps_index_search has to over-fetch, drop repeats on the host and search again.
 * eps_index_set_groups gives every row one int64 key: keys is a host or device int64[n], n must equal eps_index_row_count (else EPS_USER_ERROR);
 * any value is a key (negative, INT64_MIN, INT64_MAX, non-contiguous); rows with equal keys form a group.  The library relabels the keys to dense
 * int32 labels on the host (sort, unique, binary search: a set-up step) and keeps label[n] and key_of_label[G] on the device.  keys == NULL
 * forgets the groups.  After eps_index_attach_rows / eps_index_append_rows the labels are stale: eps_index_search_groups returns EPS_USER_ERROR
 * until the keys are set again, the rule a stale bitset follows.
 * The rule, for query j.  V_j = the rows of [0, eps_index_row_count) that are visible exactly as for eps_index_search_among: not deleted, passing
 * the int-column test and the installed program, `@distance` reading the row's exact distance.  The distance of (row, query) is, bit for bit,
 * the value eps_index_search in EPS_MODE_FLAT returns for that pair.  Every group with a row in V_j is represented by its row of V_j with the
 * smallest (distance, row) key - ties to the smaller row, a NaN distance after +inf, a group whose only visible rows are NaN still a group - and
 * the answer is the k smallest representatives in ascending key order.  Equivalently: walk V_j in ascending key order, keep a row iff its group
 * has not been seen, stop at k.  ids_out [nq][k] (through eps_index_set_id_map), dist_out [nq][k], group_keys_out [nq][k] (the caller's key of
 * each kept row), counts_out [nq] (may be NULL) = min(k, groups with a row in V_j); the unused slots -1 / +inf / key 0 (the count says which
 * slots are used).  queries and the outputs: host or device, the outputs all of one kind - device: on the index's stream, the caller
 * synchronises; host: the call synchronises.  1 <= k <= 1024; nq = 0: EPS_OK; no groups set: EPS_USER_ERROR.  p: only flat_engine is read (NULL:
 * defaults).  engine: EPS_GROUPS_PAGES takes the keys in ascending order a page of page_rows at a time - the first page from the flat engine a
 * search of (nq, page_rows) would use, later pages from the stream scan's continuation, only for the queries still unfinished - and keeps the
 * first occurrence of every label (csrc/groups.hip); a query is finished when it holds k representatives or its page came back short; one host
 * sync per round.  EPS_GROUPS_SCAN streams the table once per 4 queries and takes the minimum key per (query, group) with 64-bit atomics into a
 * table of c x G x 8 bytes, c queries at a time (c a multiple of 4 derived from scratch_bytes, never below 4), then reads the k smallest slots
 * back.  EPS_GROUPS_AUTO runs one round of pages and gives exactly the queries still unfinished to the scan: a table whose close rows are
 * spread over many groups is answered by the page, one whose close rows belong to few groups costs one scan instead of n / page_rows pages.
 * All three return the same bits.  page_rows: 0 = min(1024, 4 k rounded up to 64), or 1..1024.  scratch_bytes: 0 = 256 MiB, or a cap on the
 * scan's table; a failed allocation: EPS_INFRA_UNEXPECTED_ERROR.  eps_index_last_stats reports the call like a search.
 * eps_index_groups_info: *n_groups = G, *largest_group = rows of the largest group (both 0 while no groups are set), *last_engines = a mask of
 * (1 << EPS_GROUPS_PAGES) | (1 << EPS_GROUPS_SCAN) over the engines the last eps_index_search_groups ran, *last_scan_queries = how many of its
 * queries the scan answered; any pointer may be NULL.  A sharded handle: EPS_DB_UNSUPPORTED_ERROR from all three.  Nothing a later search
 * can observe changes. */
#define EPS_GROUPS_AUTO 0
#define EPS_GROUPS_PAGES 1
#define EPS_GROUPS_SCAN 2
int32_t eps_index_set_groups(eps_index* h, const int64_t* keys, int64_t n);
int32_t eps_index_search_groups(eps_index* h, const float* queries, int64_t nq, int32_t k, const eps_search_params* p, int32_t engine, int32_t page_rows,
                                int64_t scratch_bytes, int64_t* ids_out, float* dist_out, int64_t* group_keys_out, int32_t* counts_out);
int32_t eps_index_groups_info(eps_index* h, int64_t* n_groups, int64_t* largest_group, int32_t* last_engines, int64_t* last_scan_queries);
/* Grouped search, m rows per group: the k closest groups of eps_index_search_groups and of each its m closest rows - "the m best chunks of each of
 * the k best documents", and how many chunks of each document matched at all.  Before, a caller ran eps_index_search_groups, copied the keys to
 * the host, built a candidate list per (query, group) pair from its own copy of the keys and called eps_index_search_among with nq x k
 * pseudo-queries.
 * The rule, for query j, with V_j, the distance bits and the (distance, row) key order - NaN after +inf, ties to the smaller row - exactly as
 * eps_index_search_groups defines them.  The groups, their order, group_keys_out [nq][k] and counts_out [nq] (may be NULL) are those of
 * eps_index_search_groups with the same k, p, engine, page_rows and scratch_bytes.  For the s-th group g of query j, ids_out[j][s][0 .. c) (through
 * eps_index_set_id_map) and dist_out[j][s][0 .. c) are the c = min(m, |V_j n g|) smallest keys of V_j n g in ascending order, so slot 0 is the
 * representative eps_index_search_groups returns; row_counts_out[j][s] = c; group_sizes_out[j][s] (may be NULL) = |V_j n g|, the visible rows of
 * the group for this query (under a program on `@distance` it depends on the query).  Unused row slots: -1 / +inf; unused group slots: key 0, row
 * count 0, size 0.  Equivalently: walk V_j in ascending key order, admit a group on its first row until k groups are admitted, keep a row iff
 * its group is admitted and holds fewer than m rows; every visible row of an admitted group counts towards its size.
 * ids_out, dist_out [nq][k][m]; group_keys_out, row_counts_out, group_sizes_out [nq][k].  1 <= k <= 1024, 1 <= m <= 1024, k * m <= 65536, else
 * EPS_USER_ERROR; nq = 0: EPS_OK.  queries and the outputs: host or device, the outputs all of one kind - device: on the index's stream, the
 * caller synchronises (with EPS_GROUPS_SCAN the call has no host sync at all); host: the call synchronises.  No groups set, stale labels, stale
 * filters, a null required buffer, an unknown engine, outputs of mixed kinds: the errors of eps_index_search_groups.
 * The first call after eps_index_set_groups builds the rows by group on the device (csrc/group_rows.hip: a histogram of the labels, a scan, a
 * scatter: a set-up step with one stream sync, 4 n + 8 (G + 1) bytes kept until the labels go - eps_index_set_groups, or the refusal of stale
 * labels; a failed allocation: EPS_INFRA_UNEXPECTED_ERROR).  After the first phase a kernel lists, per (query, group) pair, the chunks of 256 rows
 * of its group (more where a group is huge: csrc/group_rows_host.hpp); a fixed grid of wavefronts strides over that list, each chunk into a
 * sorted list of m keys and a count of its visible rows, and a merge per pair follows: a group of any size is spread over the chip.
 * eps_index_groups_info reports what the equivalent eps_index_search_groups call would have left; eps_index_last_stats reports the call like a
 * search: dist_evals includes the (row, query) pairs of the second phase, main_kernel_ms is its gather.  A sharded handle:
 * EPS_DB_UNSUPPORTED_ERROR.  Nothing a later call can observe changes. */
int32_t eps_index_search_group_rows(eps_index* h, const float* queries, int64_t nq, int32_t k, int32_t m, const eps_search_params* p, int32_t engine,
                                    int32_t page_rows, int64_t scratch_bytes, int64_t* ids_out, float* dist_out, int64_t* group_keys_out,
                                    int32_t* row_counts_out, int64_t* group_sizes_out, int32_t* counts_out);
/* Multi-vector queries: the k closest groups by summed closest rows - the late-interaction score (the negated MaxSim under DOT_PRODUCT, a one-sided
 * Chamfer distance under L2) of a query that is a bag of vectors against documents that are groups of rows.  Before, a caller ran
 * eps_index_search with k = n per vector and reduced on the host: eps_index_search_groups lists only k <= 1024 groups per vector.
 * The rule.  Query j is the bag vectors[q_offsets[j] .. q_offsets[j + 1]) of t_j vectors, 0 <= t_j <= 1024.  For a vector u of the bag: V_u = the
 * visible rows exactly as eps_index_search_groups defines them for a query u (not deleted, passing the int-column test and the installed program,
 * `@distance` reading the exact distance of (row, u)); the distance of (row, u) is, bit for bit, what eps_index_search in EPS_MODE_FLAT returns;
 * b(u, g) = the smallest (distance, row) key over V_u n g - ties to the smaller row, NaN after +inf: the representative eps_index_search_groups
 * would return for u if g made its list; d(u, g) = its distance.  A group g QUALIFIES for bag j iff V_u n g is non-empty for every u of the bag; a
 * bag of t_j = 0 has no qualifying group.  score(j, g): s = +0.0f, then s = s + d(u, g) in fp32 for u in bag order, one add after the other -
 * nothing is reassociated, a NaN or an infinite term propagates as IEEE 754 says.  The qualifying groups are ordered by (score, group key): every
 * NaN score takes the one place after +inf, ties go to the smaller int64 key.  The answer is the k smallest; counts_out[j] = min(k, qualifying).
 * Candidates.  cand_keys == NULL: every group of eps_index_set_groups is considered.  Else only the groups whose keys the caller names: one list
 * cand_keys[0 .. n_cand) for every bag (cand_offsets == NULL), or bag j's list cand_keys[cand_offsets[j] .. cand_offsets[j + 1]) - cand_offsets a
 * host int64[nq + 1] checked as eps_index_search_among checks its offsets.  A key that names no group is ignored, a key named several times counts
 * once.  Both forms return the same bits: the second stage of a pipeline whose first stage found candidate documents by any means.
 * vectors: host or device float[T][dim], T = q_offsets[nq] < 2^31 (COSINE: normalised already); q_offsets: host int64[nq + 1], [0] = 0,
 * non-decreasing; cand_keys: host (copied) or device (used in place) int64[n_cand], 0 <= n_cand < 2^31.  group_keys_out, score_out [nq][k];
 * counts_out [nq], may be NULL; match_ids_out / match_dist_out, both NULL or neither, k * T elements: the entry of bag j, slot s, vector u lies at
 * k * q_offsets[j] + s * t_j + u and holds the row of b(u, g_s) (through eps_index_set_id_map) and d(u, g_s) - the chunk that matched each query
 * vector.  Unused slots: key 0 / +inf / -1 / +inf.  The outputs are all host or all device.  Host arrays are read before the call returns, device
 * arrays at the call's place in the index's stream; with device outputs the call does not synchronise the host (the first candidate-form call
 * after eps_index_set_groups builds the rows by group, as eps_index_search_group_rows does: a set-up step with one sync).
 * 1 <= k <= 1024, t_j <= 1024, well-formed offsets, else EPS_USER_ERROR; nq = 0: EPS_OK.  No groups set, stale labels, stale filters, a null required
 * buffer, outputs of mixed kinds: the errors of eps_index_search_groups.  A sharded handle: EPS_DB_UNSUPPORTED_ERROR.
 * A bag is never cut: the vectors of as many whole bags as fit share one table of 8-byte keys - t_j x G of them per bag in the whole-table form,
 * t_j x its candidates in the candidate form.  scratch_bytes = 0: max(256 MiB, the largest bag's table); a positive value is a cap, and a bag
 * whose own table exceeds it is refused with EPS_DB_UNSUPPORTED_ERROR before any launch, the message naming the bytes needed.
 * Whole-table form (csrc/multi.hip): eps_index_search_groups' scan with the bag vectors as its queries, then a sum and top-k over the table's
 * columns; n * dim * 4 + n * 4 bytes of traffic per 4 vectors plus 8 * t_j * G per bag.  Candidate form: the rows of the named groups, through the
 * rows by group, once per 4 vectors per bag that names them.  eps_index_last_stats reports the call like a search: dist_evals = the (row, vector)
 * pairs given a distance, main_kernel_bits = 32, main_kernel_ms = the scan or the gather.  eps_index_groups_info and everything else a later call
 * can observe are unchanged. */
int32_t eps_index_search_multi(eps_index* h, const float* vectors, const int64_t* q_offsets, int64_t nq, const int64_t* cand_keys,
                               const int64_t* cand_offsets, int64_t n_cand, int32_t k, int64_t scratch_bytes, int64_t* group_keys_out, float* score_out,
                               int32_t* counts_out, int64_t* match_ids_out, float* match_dist_out);
/* Diverse search: k rows per query that are close to the query but not copies of each other - greedy maximal marginal relevance (MMR) over a pool
 * of the query's fetch_k closest rows.  Before, a caller ran eps_index_search with k = fetch_k, copied fetch_k x dim x 4 bytes of rows per query to
 * the host and ran the loop there: the distances between the pool rows themselves are what only the index can compute without moving the rows.
 * The rule, for query j.  Pool: P_j = the answer eps_index_search in EPS_MODE_FLAT gives for (j, k = fetch_k) - ascending (distance, id) order, the
 * same visibility (not deleted, passing the int-column test and the installed program, `@distance` reading the exact distance), the same distance
 * bits; p: only flat_engine is read (NULL: defaults), chosen as a search of (nq, fetch_k) would choose it, a program that reads `@distance` taking
 * the exact stream scan; all engines return the same bits.  With cand_ids != NULL the pool is instead the answer of eps_index_search_among for the
 * same cand_ids / cand_offsets / n_cand with k = fetch_k: one list for the batch or one per query, unknown ids ignored, a row named several times
 * judged once (cand_ids == NULL with cand_offsets != NULL or n_cand != 0: EPS_USER_ERROR).  Pool position i is the i-th entry, d_i its distance to
 * the query with those bits, np <= fetch_k the pool's size.
 * Distance between pool rows: D(c, s) is, bit for bit, what eps_index_search_among returns for row c when the QUERY is row s as the index holds it
 * (-0 as +0, any NaN as the one quiet NaN, like every distance the library returns).  The orientation is fixed: the selected row is the query
 * side.  Visibility plays no part in D.
 * Selection: lam = lambda, mu = 1.0f - lambda computed once in fp32.  Step 1 takes position 0; its score is lam * d_0, one rounded multiply.  After
 * a row s is selected every unselected c updates m(c): m(c) = D(c, s) if s is the first selected row, otherwise m(c) = D(c, s) if D(c, s) < m(c) by
 * IEEE less-than - a NaN never replaces a value and a NaN m is never replaced.  Step t >= 2 scores every unselected c as
 * score(c) = (lam * d_c) - (mu * m(c)): two rounded multiplies and one rounded subtract, never contracted; the step takes the smallest score, scores
 * ordered as distances are everywhere in the library (-0 equals +0, every NaN after +inf), ties to the smaller pool position.  Selection stops at
 * min(k, np) rows.  lambda = 1 returns exactly the first k of the pool (while every m is finite: 0 * inf is a NaN score); lambda = 0 still starts at position 0.
 * ids_out[j][t] (through eps_index_set_id_map), dist_out[j][t] = d of the row selected t-th, score_out[j][t] (may be NULL) = its score at selection
 * as its key holds it (-0 as +0, a NaN as the quiet NaN), counts_out[j] (may be NULL) = min(k, np); rows in SELECTION order, the unused slots
 * -1 / +inf / +inf.  queries and the outputs: host or device, the outputs all of one kind - device: on the index's stream, the caller synchronises,
 * the call has no host sync of its own (EPS_FLAT_MFMA / _I8 keep the ones a search has); host: the call synchronises.  Host arrays are read before
 * the call returns.  1 <= k <= fetch_k <= 1024, lambda in [0, 1] and not NaN, cand_offsets as eps_index_search_among checks it, else
 * EPS_USER_ERROR; nq = 0: EPS_OK.  A null required buffer, outputs of mixed kinds, stale filters after an append: the errors of
 * eps_index_search_among.  A sharded handle: EPS_DB_UNSUPPORTED_ERROR.
 * After the pool (one page of a flat engine, or eps_index_search_among's two launches) one launch of diverse_select_kernel (csrc/diverse.hip): one
 * workgroup of 256 threads per query holds the pool's keys, m and a mark per position in LDS, stages the row selected last in LDS as the query and
 * strides over the pool with the flat scan's blocking.  Row reads: (min(k, np) - 1) x np x dim x 4 bytes per query, re-read every step, from L2
 * where the pool fits - QUADRATIC in k when k follows fetch_k: k = fetch_k = 1024 at dim 768 reads 3.2 GB per query.
 * eps_index_last_stats reports the call like a search: dist_evals = the pool phase's count + the (row, selected row) pairs given a distance,
 * main_kernel_bits 32, main_kernel_rows = fetch_k, main_kernel_queries = nq, main_kernel_ms = the selection kernel.  Nothing a later call can
 * observe changes. */
int32_t eps_index_search_diverse(eps_index* h, const float* queries, int64_t nq, int32_t k, int32_t fetch_k, float lambda, const int64_t* cand_ids,
                                 const int64_t* cand_offsets, int64_t n_cand, const eps_search_params* p, int64_t* ids_out, float* dist_out,
                                 float* score_out, int32_t* counts_out);
int32_t eps_index_last_stats(const eps_index* h, eps_search_stats* out);
/* main-kernel milliseconds (hipEvent pairs recorded on the index's stream) of the most recent search calls, oldest
 * first, at most min(cap, 64); synchronises the stream.  Returns the number written.  Lets a caller time a run of
 * searches without a host sync inside it. */
int32_t eps_index_kernel_times(eps_index* h, double* ms_out, int32_t cap);

/* ---- Sparse-vector fields (SPARSE_VECTOR_FLOAT): the exact scan of a CSR table.  GetDistFunc returns GetL2DistSqr / GetCosineDist /
 * GetInnerProductDist for such a field (db/index/index.cpp:22-34, db/vector.cpp:7-96) and BruteForceSearch calls them row by row
 * (db/execution/vec_search_executor.cpp:742, :802).  A handle of its own kind: nothing of an eps_index applies to it.
 *
 * A table is n rows in CSR: offsets int64[n + 1] with offsets[0] = 0, non-decreasing, offsets[n] = nnz; indices int32[nnz], strictly increasing
 * inside a row, 0 <= index < dim; values float[nnz] - the row checks of the reference's insert path (db/table_segment_mvp.cpp:526-550), except
 * that an empty row is accepted.  A batch of queries has the same form.  For query j the search returns the k smallest (distance, id) keys over the
 * rows whose bit in the deleted bitset is clear.  distance(row, query) is, bit for bit, what the reference's function returns for (v1 = row,
 * v2 = query): EPS_METRIC_EUCLIDEAN -> GetL2DistSqr, COSINE -> GetCosineDist, DOT_PRODUCT -> GetInnerProductDist - one fp32 accumulator from 0.0f,
 * the two-pointer merge in ascending index order, every product rounded before it is added (no fused multiply-add), L2 adding the unmatched
 * squares of both sides in merged order; COSINE = 1 - dot / sqrtf(v1_prod * v2_prod) with both norms summed in stored order, so an empty row or
 * query gives NaN.  Keys order as everywhere in the library: -0 equals +0, every NaN comes after +inf, ties are broken by id; a NaN row still
 * counts as a row.
 *
 * create: 1 <= dim <= 2^31 - 1; status codes and the no-CPU-fallback rule (EPS_INFRA_UNEXPECTED_ERROR without a gfx950 device) as
 * eps_index_create.  A NULL handle: EPS_USER_ERROR from every call.
 * attach_csr: the three arrays all host (copied) or all device (borrowed: the caller keeps them alive and unchanged); a mixed set is
 * EPS_USER_ERROR; 0 <= n < 2^31.  offsets[n] defines nnz (a device offsets array is read back for that one value).  Replaces any previous
 * table and forgets the bitset.  The table is validated in one device pass over the resident arrays before a search can see it - a row's elements
 * are read only after its own offsets were found ordered and inside [0, nnz], so no input makes a kernel read outside the three arrays; the pass
 * also takes every row's sum of squares in stored order (COSINE's v1_prod, the bits a recomputation per pair would give).  A violation:
 * EPS_USER_ERROR naming the first offending row, and the handle keeps the table it had.  The call synchronises the handle's stream.
 * set_id_map / set_deleted: as eps_index_set_id_map / eps_index_set_deleted (host or device bits, nbytes >= ceil(n / 8) else EPS_USER_ERROR,
 * NULL clears).  Int-column tests and filter programs are not served here: a caller folds them into the bitset.
 * search: q_offsets is a HOST int64[nq + 1], checked on the host; q_indices / q_values both host (validated on the host, copied) or both device
 * (validated by one small launch whose verdict the call reads back - ONE stream synchronisation - before it launches the scan).  A malformed
 * query: EPS_USER_ERROR naming the query.  A query of more than 4096 non-zeros (its pairs are staged in LDS): EPS_DB_UNSUPPORTED_ERROR, before
 * any launch.  1 <= k <= 1024 else EPS_USER_ERROR; nq = 0: EPS_OK, nothing touched; n = 0: counts 0.  ids_out [nq][k], dist_out [nq][k],
 * counts_out [nq] (may be NULL): all host (the call synchronises) or all device (on the handle's stream, the caller synchronises); ids through
 * the id map, unused slots -1 / +inf, counts = min(k, visible rows).  The call first waits for earlier work on the handle's stream (its staging
 * buffers are reused).
 * last_stats: dist_evals = n * nq (every row gets a distance; visibility is judged only for keys that would enter a list), main_kernel_rows = n,
 * main_kernel_queries = nq, main_kernel_bits = 32, main_kernel_launches, kernel_ms / main_kernel_ms from events; everything else 0. */
typedef struct eps_sparse_index eps_sparse_index;
int32_t eps_sparse_index_create(int64_t dim, int32_t metric, int32_t device, eps_sparse_index** out);
int32_t eps_sparse_index_destroy(eps_sparse_index* h);
const char* eps_sparse_index_last_error(const eps_sparse_index* h);
int32_t eps_sparse_index_set_stream(eps_sparse_index* h, void* hip_stream);
int32_t eps_sparse_index_synchronize(eps_sparse_index* h);
int32_t eps_sparse_index_attach_csr(eps_sparse_index* h, const int64_t* offsets, const int32_t* indices, const float* values, int64_t n);
int64_t eps_sparse_index_row_count(const eps_sparse_index* h);
int32_t eps_sparse_index_set_id_map(eps_sparse_index* h, int64_t base, int64_t stride);
int32_t eps_sparse_index_set_deleted(eps_sparse_index* h, const uint8_t* bits, int64_t nbytes);
int32_t eps_sparse_index_search(eps_sparse_index* h, const int64_t* q_offsets, const int32_t* q_indices, const float* q_values, int64_t nq,
                                int32_t k, int64_t* ids_out, float* dist_out, int32_t* counts_out);
int32_t eps_sparse_index_last_stats(const eps_sparse_index* h, eps_search_stats* out);

/* Inverted lists (postings) of the attached table: the table stored by column, so that a DOT_PRODUCT or COSINE query touches only the postings of
 * its own terms.  GetInnerProduct and GetCosineDist (db/vector.cpp:11-47) add a product only on a matching index, into one fp32 accumulator that
 * starts at 0.0f, in ascending index order - so a per-row accumulator that receives acc = acc + (row_value * query_value), the query's terms applied
 * in ascending index order, the product rounded before it is added and nothing fused, holds the same bits.  GetL2DistSqr adds the unmatched squares
 * of both sides in merged order and has no such form: EUCLIDEAN stays on the scan.  Opt-in; no other call changes what it does.
 *
 * The layout: col_offsets int64[dim + 1], col_offsets[0] = 0, non-decreasing, col_offsets[dim] = nnz; the postings of column c are
 * rows[col_offsets[c] .. col_offsets[c + 1]) with their values; rows are strictly ascending inside a column and the value bits are the CSR's.  The
 * image is owned by the handle, also where the CSR arrays are borrowed device arrays, and costs 8 * nnz + 8 * (dim + 1) bytes of device memory on
 * top of the CSR (the build needs up to 16 * nnz more and frees them when it ends).
 * build_inverted: builds the image of the attached table on the device (a stable sort of the CSR's elements by column) and synchronises.  No
 * table: EPS_USER_ERROR.  An EUCLIDEAN handle: EPS_DB_UNSUPPORTED_ERROR.  dim > 2^24: EPS_DB_UNSUPPORTED_ERROR (the column directory is dense).
 * Out of device memory: EPS_INFRA_UNEXPECTED_ERROR, and the handle goes on answering by the scan.  Calling it twice rebuilds.  n = 0 or nnz = 0:
 * an empty image.
 * drop_inverted: frees the image; without one EPS_OK.  attach_csr forgets the image as it forgets the bitset; set_deleted and set_id_map do not
 * touch it.
 * search, while an image exists on a DOT_PRODUCT or COSINE handle, runs on it: every documented property of eps_sparse_index_search holds
 * unchanged - validation, limits, host and device buffers, k <= 1024, the 4096-term query limit, NaN ordering, counts, the id map, the deleted
 * bitset and last_stats (dist_evals = n * nq, main_kernel_bits = 32, main_kernel_ms = the inverted launches) - and so does every returned bit.
 * The two engines are compared on one handle by searching, drop_inverted, and searching again (a rebuild is one sort of the table); the
 * eps_set_tuning table has no entry for them.
 * inverted_info: any out pointer may be NULL.  *columns = dim while an image exists, else 0; *postings = nnz of the image; *longest_column = its
 * longest column; *last_engine: 0 = none yet, 1 = scan, 2 = inverted lists (the engine of the last search).
 * get_inverted: host copies of the layout, for tests and tools: col_offsets int64[dim + 1], rows int32[nnz], values float[nnz]; any may be NULL.
 * Without an image: EPS_USER_ERROR. */
int32_t eps_sparse_index_build_inverted(eps_sparse_index* h);
int32_t eps_sparse_index_drop_inverted(eps_sparse_index* h);
int32_t eps_sparse_index_inverted_info(const eps_sparse_index* h, int64_t* columns, int64_t* postings, int64_t* longest_column, int32_t* last_engine);
int32_t eps_sparse_index_get_inverted(eps_sparse_index* h, int64_t* col_offsets, int32_t* rows, float* values);

/* in-place L2 normalisation of float[n][dim] (host or device). only_if_nonzero = 1 reproduces the
 * insert path (sum > 1e-10), 0 the query path (unconditional). */
int32_t eps_normalize_rows(float* rows, int64_t n, int64_t dim, int32_t only_if_nonzero, int32_t device,
                           void* hip_stream);

/* merges `shards` sorted top-k lists per query by (dist,id): dist/ids are [shards][nq][k] device or host
 * arrays (e.g. the output of an all-gather); out_* are [nq][k]. */
int32_t eps_merge_topk(const float* dist, const int64_t* ids, int32_t shards, int64_t nq, int32_t k,
                       float* out_dist, int64_t* out_ids, int32_t device, void* hip_stream);

/* the same merge over ONE gathered device buffer ("one ncclAllGather over a packed buffer"): shard s
 * contributed shard_stride_bytes bytes holding int64 ids[nq][k] at offset 0 and float dist[nq][k] at dist_offset_bytes. */
int32_t eps_merge_topk_packed(const void* gathered, int64_t shard_stride_bytes, int64_t dist_offset_bytes, int32_t shards,
                              int64_t nq, int32_t k, float* out_dist, int64_t* out_ids, int32_t device, void* hip_stream);

/* ---- Radius search and ordered select across shards.  The reference has no counterpart (it does not shard a table): G single-device
 * indices, shard s holding the rows i with i mod G = s and eps_index_set_id_map(base = s, stride = G), each answer the whole call over their rows;
 * these calls join the G answers into exactly the answer of ONE index over the whole table.  One launch (csrc/merge_lists.hip): every list element
 * finds its own output slot - its position plus, from one binary search per other list, the number of keys before it (`<=` against the shards before
 * it, `<` against those after: equal keys are ordered by shard number) - no serial merge, no sort.
 *
 * eps_merge_range: ids / dist [shards][nq][cap], counts int32 [shards][nq], totals int64 [shards][nq] = what eps_index_search_range wrote on every
 * shard (global ids through each shard's id map).  A list's valid length is its counts entry; keys order as everywhere in the library, by (distance,
 * id), -0 = +0, every NaN after +inf.  out_totals[j] = the sum of totals[s][j]; out_counts[j] = min(that, cap); out_ids[j] / out_dist[j] = the count
 * smallest keys in ascending order, the unused slots -1 / +inf: the contract of eps_index_search_range - also where a shard's own total exceeded cap,
 * since the cap closest of the union lie among the per-shard cap closest.  out_counts and out_totals may be NULL.  1 <= cap <= 8192,
 * 1 <= shards <= 16 (else EPS_USER_ERROR), nq = 0: EPS_OK.  Lists and results are all host or all device buffers (a mixed set: EPS_USER_ERROR):
 * host buffers are staged and the call synchronises; device buffers are used in place, asynchronously on hip_stream.
 * eps_range_pack_bytes: the size of ONE shard's packed answer, ids i64[nq][cap] | totals i64[nq] | dist f32[nq][cap] | counts i32[nq], rounded up to
 * a multiple of 8 (-1: nq or cap out of range).  eps_merge_range_packed: the same merge over one gathered DEVICE buffer in which shard s's packed
 * answer starts at s * shard_stride_bytes (a multiple of 8, >= eps_range_pack_bytes) - what one all-gather of packed answers delivers.
 *
 * eps_merge_select: ids [shards][len], counts [shards], totals [shards] = what eps_index_select(skip = 0, limit = len) wrote on every shard.
 * out_ids[0 .. count) = ranks [skip, skip + limit) of the ascending merged ids, *count_out = clamp(sum of counts - skip, 0, limit), *total_out (may be
 * NULL) = the sum of totals.  A shard's list must reach as far as the window can: len < skip + limit is EPS_USER_ERROR, and so is a negative len,
 * skip or limit; limit = 0: count 0.  Host or device as above. */
int32_t eps_merge_range(const int64_t* ids, const float* dist, const int32_t* counts, const int64_t* totals, int32_t shards, int64_t nq, int32_t cap,
                        int64_t* out_ids, float* out_dist, int32_t* out_counts, int64_t* out_totals, int32_t device, void* hip_stream);
int64_t eps_range_pack_bytes(int64_t nq, int32_t cap);
int32_t eps_merge_range_packed(const void* gathered, int64_t shard_stride_bytes, int32_t shards, int64_t nq, int32_t cap, int64_t* out_ids, float* out_dist,
                               int32_t* out_counts, int64_t* out_totals, int32_t device, void* hip_stream);
int32_t eps_merge_select(const int64_t* ids, const int64_t* counts, const int64_t* totals, int32_t shards, int64_t len, int64_t skip, int64_t limit,
                         int64_t* out_ids, int64_t* count_out, int64_t* total_out, int32_t device, void* hip_stream);

/* ---- The exchange step of the sharded path, owned by the library (r6).  One process per GPU: every rank holds, for the whole
 * batch, the top-k lists over ITS shard (global ids); eps_exchange_allgather_merge packs them as [ids int64[nq][k] | dist f32[nq][k]]
 * (12 k nq bytes per rank), runs ONE ncclAllGather on the RCCL communicator the handle owns (xGMI inside a node) and merges the `world`
 * sorted lists of every query by (dist, id) - every rank ends with the same global top-k in out_ids / out_dist.  Lists, results and the
 * stream belong to the rank's device; the call is asynchronous on that stream.  RCCL is resolved at run time (dlopen; a copy the process
 * already holds - PyTorch ships one - is the one used).  Bootstrap, the caller's only part: rank 0 fills 128 bytes with
 * eps_exchange_unique_id and sends them to every rank (bench.py: a gloo broadcast), every rank calls eps_exchange_create (collective:
 * returns when all `world` ranks have joined).  *out is set even on failure (its message: eps_exchange_last_error).  world <= 16.
 * The reference has no counterpart (no sharding, SURVEY 8e "Semantics vs reference"): sharded exact top-k == unsharded exact top-k. */
#define EPS_EXCHANGE_ID_BYTES 128
typedef struct eps_exchange eps_exchange;
int32_t eps_exchange_unique_id(void* id128);
int32_t eps_exchange_create(int32_t rank, int32_t world, const void* id128, int32_t device, eps_exchange** out);
int32_t eps_exchange_allgather_merge(eps_exchange* x, const int64_t* ids, const float* dist, int64_t nq, int32_t k, int64_t* out_ids, float* out_dist,
                                     void* hip_stream);
/* The same step for a radius search: every rank holds its shard's answer of eps_index_search_range for the whole batch; the call packs it into the
 * rank's slot of the gathered buffer (eps_range_pack_bytes per rank), runs ONE ncclAllGather and the launch of eps_merge_range_packed - every rank
 * ends with the unsharded answer.  Device buffers only; out_counts / out_totals may be NULL; eps_exchange_times reports the call like a top-k
 * exchange.  The mailbox form does not serve it. */
int32_t eps_exchange_allgather_merge_range(eps_exchange* x, const int64_t* ids, const float* dist, const int32_t* counts, const int64_t* totals, int64_t nq,
                                           int32_t cap, int64_t* out_ids, float* out_dist, int32_t* out_counts, int64_t* out_totals, void* hip_stream);
/* device time of the two parts - all-gather, merge - of the last calls (hipEvents on their stream, kept for 64 calls; waits for them):
 * us_pairs[2 i], us_pairs[2 i + 1] for the oldest .. newest of min(calls, 64, max_calls) calls; returns how many (-1: failure) */
int32_t eps_exchange_times(eps_exchange* x, double* us_pairs, int32_t max_calls);
/* what the handle runs on: rank, world, RCCL's version number and the path of the library that answers */
int32_t eps_exchange_info(eps_exchange* x, int32_t* rank, int32_t* world, int32_t* rccl_version, char* rccl_path, int64_t cap);
/* The b = 1 form of the same step ("for b=1 prefer direct P2P stores into a peer-mapped buffer + flag"; r6): for a handful of queries -
 * nq * k * 12 <= 16 KB per rank - a collective costs more than the bytes it moves.  Every rank owns a MAILBOX in device memory that every peer maps
 * (hipIpc); a call stores this rank's packed lists into every peer's mailbox, raises a flag there (release at system scope), waits on the device until
 * all `world` flags of the OWN mailbox show the call's number, and merges - three small launches on the caller's stream, no collective, no host round
 * trip.  Setup: eps_exchange_create_direct (no communicator; or an exchange made by eps_exchange_create), eps_exchange_mailbox_export on every rank
 * (64 bytes), the host gathers the `world` handles by whatever it has, eps_exchange_mailbox_connect(x, handles[world][64]).  Ranks may share a device.
 * A peer that does not deliver within ~10 s is reported by a later call (EPS_INFRA_UNEXPECTED_ERROR) instead of hanging the stream. */
#define EPS_EXCHANGE_HANDLE_BYTES 64
int32_t eps_exchange_create_direct(int32_t rank, int32_t world, int32_t device, eps_exchange** out);
int32_t eps_exchange_mailbox_export(eps_exchange* x, void* handle64);
int32_t eps_exchange_mailbox_connect(eps_exchange* x, const void* handles);
int32_t eps_exchange_direct_merge(eps_exchange* x, const int64_t* ids, const float* dist, int64_t nq, int32_t k, int64_t* out_ids, float* out_dist,
                                  void* hip_stream);
const char* eps_exchange_last_error(eps_exchange* x);
void eps_exchange_destroy(eps_exchange* x);

/* Engine-selection switches.  The library reads NO environment variable: what used to be lab switches are entries of one
 * process-wide table that only this call writes (name, value as text; value == NULL removes the entry; name == NULL empties
 * the table).  No entry changes a result - they pick between engines that return the same bits (tests/ run every answer
 * through both sides of each) or turn diagnostics on.  A name not listed here is stored and ignored:
 *   EPS_DEBUG (stage log on stderr), EPS_DEBUG_ONE_PASS_OVERFLOW (the one-pass search's log on stderr after a call that overflowed),
 *   EPS_TRV_PROF (traversal phase profile on stderr),
 *   EPS_TRV_PREFILTER 0|1 (8-bit lower-bound test of the traversal), EPS_TRV_VISITED bitmap|stamps, EPS_TRV_STAMP_START, EPS_TRV_WAVES 4|8|16,
 *   EPS_FLAT_ONE_PASS 0|1, EPS_ONE_PASS_TIMED, EPS_S8_HOST_WORDS 0|1, EPS_S8_TWO_LAUNCHES 0|1, EPS_S8_MAX_K 1..64, EPS_S8_FILTER_PROGRAMS 0|1, EPS_S8_RERANK 0|1,
 *   EPS_HOST_STAGING 0|1, EPS_MFMA_MAX_BATCH, EPS_MFMA_PROBE, EPS_MFMA_SEED, EPS_MFMA_GROUPSYNC, EPS_MFMA_SYNC_SHIFT, EPS_BUILD_VISITED, EPS_BUILD_PREFILTER,
 *   EPS_MIRROR_ROTATE 0|1 (frame of the 8-bit grid: identity | rotated; unset = chosen per table when its mirror is first built; read at that moment only),
 *   EPS_MIRROR_CLIP e (the grid cuts 10^-e of the sampled values off each tail, 1 <= e <= 9, in either frame; unset = 10^-7, rotated frame 10^-6;
 *   read when the mirror is first built).
 * Returns EPS_OK. */
int32_t eps_set_tuning(const char* name, const char* value);

#ifdef __cplusplus
}
#endif
#endif /* EPSILLA_GFX950_H_ */
