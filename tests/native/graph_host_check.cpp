// Stand-alone host check of csrc/graph_host.hpp - the seed list of a search, the connectivity repair and CSR assembly of the build, the launch plan
// of the traversal with its refusals, the tail merge's arithmetic, the LDS bytes of the build's launches and their refusal, the LDS layouts of the three
// kernels and the rule that judges the 8-bit prefilter - for a CPU build under -fsanitize=address,undefined
// (tests/test_graph_host_cpu.py builds and runs it).  Every list lives in a heap block exactly as long as the library's, so an index beyond a
// list is a heap overflow the sanitizer reports.
//   graph_host_check                    all checks; prints "graph_host_check OK"
//   graph_host_check seeds <file> <L>   the seed list of the graph in <file> (int64: n, nav, off[n + 1], nbr[off[n]]), one line of ids
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../vectordb_amd/csrc/graph_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;
typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;
static const uint32_t PAD = 0xFFFFFFFFu;

// ------------------------------------------------------------------------------------------------ seed lists
// the rule once more, with a set and a loop: distinct neighbours that name a node, then nav + 1, nav + 2, ... modulo n
static std::vector<uint32_t> seeds_restated(const std::vector<int64_t>& adj, int64_t nav, int64_t n, int64_t L) {
  std::set<int64_t> seen;
  std::vector<uint32_t> out;
  for (int64_t v : adj)
    if ((int64_t)out.size() < L && v >= 0 && v < n && seen.insert(v).second) out.push_back((uint32_t)v);
  for (int64_t step = 1; (int64_t)out.size() < L; ++step)
    if (seen.insert((nav + step) % n).second) out.push_back((uint32_t)((nav + step) % n));
  return out;
}

static void seed_case(const std::vector<int64_t>& adj, int64_t nav, int64_t n, int64_t L) {
  const std::vector<uint32_t> want = seeds_restated(adj, nav, n, L);
  std::vector<uint32_t> got64, got32;
  std::vector<uint32_t> adj32;
  for (int64_t v : adj) adj32.push_back(v < 0 ? PAD : (uint32_t)v);
  seed_list(adj.data(), (int64_t)adj.size(), nav, n, L, got64);      // the CSR's int64 ids (-1: no node)
  seed_list(adj32.data(), (int64_t)adj32.size(), nav, n, L, got32);  // the build's u32 lists (0xFFFFFFFF: no node)
  CHECK(got64 == want && got32 == want);
  CHECK((int64_t)got64.size() == L);
  std::set<uint32_t> distinct(got64.begin(), got64.end());
  CHECK((int64_t)distinct.size() == L);
  for (uint32_t v : got64) CHECK((int64_t)v < n);
}

static void seeds() {
  seed_case({}, 0, 1, 1);                                   // n = 1: the node itself
  seed_case({0}, 0, 1, 1);
  seed_case({1}, 0, 2, 1);
  seed_case({1}, 0, 2, 2);                                  // L = n
  seed_case({0}, 1, 2, 2);                                  // nav is the last node: the fill wraps
  seed_case({3, 3, 5, 3, 5, 0}, 2, 7, 4);                   // duplicate neighbours
  seed_case({3, 3, 5, 3, 5, 0}, 2, 7, 7);
  seed_case({0, 1, 2, 3, 4, 5}, 6, 7, 3);                   // more than L neighbours; nav last
  seed_case({4, -1, 4, -1, -1}, 6, 7, 7);                   // padding inside a list; nav last: 0, 1, ... follow
  seed_case({6}, 6, 7, 7);                                  // the node names itself
  seed_case({}, 3, 7, 5);
  std::vector<int64_t> many;
  for (int i = 0; i < 50; ++i) many.push_back((i * 37) % 64);
  for (int i = 0; i < 14; ++i) many.push_back(-1);
  for (int64_t L : {1, 2, 49, 50, 51, 63, 64}) {
    seed_case(many, 63, 64, L);
    seed_case(many, 0, 64, L);
    seed_case(many, 37, 64, L);
  }
}

// ------------------------------------------------------------------------------------------------ repair and CSR
struct Lists {   // [n][R] lists in heap blocks of exactly that size
  int64_t n;
  int R;
  std::vector<uint32_t> ids, deg;
  Lists(int64_t n_, int R_, const Edges& edges) : n(n_), R(R_), ids((size_t)n_ * R_, PAD), deg((size_t)n_, 0) {
    for (auto& e : edges) ids[(size_t)e.first * R + deg[e.first]++] = e.second;
  }
};

// traces[x]: the nodes orphan x's search evaluated, closest first.  Returns the repair edges after every property has been checked.
static Edges repair_case(const Lists& g, uint32_t nav, const std::vector<std::vector<uint32_t>>& traces, uint32_t seed, size_t want_edges) {
  std::vector<uint8_t> reached((size_t)g.n, 0);
  std::vector<uint32_t> stack, orphans;
  mark_reached(nav, g.ids.data(), g.deg.data(), g.R, reached, stack);
  CHECK(stack.empty());
  for (int64_t i = 0; i < g.n; ++i)
    if (!reached[i]) orphans.push_back((uint32_t)i);
  std::vector<unsigned long long> top(orphans.size() * TRACE_K, TRACE_EMPTY);
  for (size_t i = 0; i < orphans.size(); ++i) {
    const std::vector<uint32_t>& t = traces[orphans[i]];
    for (size_t e = 0; e < t.size() && e < (size_t)TRACE_K; ++e) top[i * TRACE_K + e] = ((unsigned long long)(e + 1) << 32) | t[e];   // (ascending keys)
  }
  const uint32_t deg_cap = (uint32_t)std::max(64, g.R + 1);
  const Edges extra = repair_orphans(g.n, g.R, g.ids.data(), g.deg.data(), orphans, top.data(), reached, deg_cap, seed ? seed : 100);
  CHECK(extra.size() == want_edges);
  for (int64_t i = 0; i < g.n; ++i) CHECK(reached[i]);
  std::vector<int64_t> off, nbr;
  graph_csr(g.n, g.R, g.ids.data(), g.deg.data(), extra, off, nbr);
  CHECK((int64_t)off.size() == g.n + 1 && off[0] == 0 && off[g.n] == (int64_t)nbr.size());
  int64_t edges = 0;
  for (int64_t i = 0; i < g.n; ++i) edges += g.deg[i];
  CHECK((int64_t)nbr.size() == edges + (int64_t)extra.size());
  for (int64_t i = 0; i < g.n; ++i) {
    CHECK(off[i] <= off[i + 1] && off[i + 1] - off[i] <= (int64_t)deg_cap);
    for (uint32_t j = 0; j < g.deg[i]; ++j) CHECK(nbr[off[i] + j] == (int64_t)g.ids[(size_t)i * g.R + j]);   // the node's own edges, in order ...
    int64_t at = off[i] + g.deg[i];
    for (auto& pr : extra)                                                                                    // ... then its repair edges, in the order found
      if ((int64_t)pr.first == i) CHECK(at < off[i + 1] && nbr[at++] == (int64_t)pr.second);
    CHECK(at == off[i + 1]);
  }
  // the CSR reaches every node from nav
  std::vector<uint8_t> seen((size_t)g.n, 0);
  std::vector<int64_t> todo(1, nav);
  seen[nav] = 1;
  while (!todo.empty()) {
    const int64_t x = todo.back();
    todo.pop_back();
    for (int64_t e = off[x]; e < off[x + 1]; ++e)
      if (!seen[nbr[e]]) {
        seen[nbr[e]] = 1;
        todo.push_back(nbr[e]);
      }
  }
  for (int64_t i = 0; i < g.n; ++i) CHECK(seen[i]);
  return extra;
}

static void repair() {
  {   // two components
    const Lists g(6, 3, {{0, 1}, {1, 2}, {2, 0}, {3, 4}, {4, 5}, {5, 3}});
    const Edges x = repair_case(g, 0, {{}, {}, {}, {4, 1, 2}, {1}, {1}}, 0, 1);   // (4 is closer to 3 but not reached: 1 is taken)
    CHECK(x.size() == 1 && x[0] == std::make_pair(1u, 3u));
  }
  {   // nothing to repair: no edge, the CSR is the lists
    const Lists g(3, 2, {{0, 1}, {1, 2}});
    CHECK(repair_case(g, 0, {{}, {}, {}}, 0, 0).empty());
  }
  {   // three components in a chain: {0, 1} <- nav, {2, 3} -> {4, 5}.  Attaching 2 reaches 4 and 5, which get no edge
    const Lists g(6, 2, {{0, 1}, {1, 0}, {2, 3}, {3, 4}, {4, 5}, {5, 4}});
    const Edges x = repair_case(g, 0, {{}, {}, {0}, {0}, {1}, {1}}, 0, 1);
    CHECK(x.size() == 1 && x[0] == std::make_pair(0u, 2u));
  }
  {   // the same chain met from its far end: {2, 3} is reached from {4, 5} only, so both get an edge, and 4's may come from the freshly linked 2
    const Lists g(6, 2, {{0, 1}, {1, 0}, {2, 3}, {3, 2}, {4, 5}, {5, 2}});
    const Edges x = repair_case(g, 0, {{}, {}, {1}, {1}, {5, 2, 0}, {0}}, 0, 2);
    CHECK(x.size() == 2 && x[0] == std::make_pair(1u, 2u) && x[1] == std::make_pair(2u, 4u));
  }
  {   // a saturated node passes the orphan on: nav has 64 edges (deg_cap = 65), the first orphan fills it, the others go to the next of the trace
    Edges e;
    for (uint32_t j = 1; j <= 64; ++j) e.push_back({0, j});
    const Lists g(70, 64, e);
    std::vector<std::vector<uint32_t>> tr(70);
    for (uint32_t o = 65; o < 70; ++o) tr[o] = {0, 1, 2};
    const Edges x = repair_case(g, 0, tr, 0, 5);
    CHECK(x.size() == 5 && x[0] == std::make_pair(0u, 65u));
    for (size_t i = 1; i < x.size(); ++i) CHECK(x[i] == std::make_pair(1u, (uint32_t)(65 + i)));
  }
  for (uint32_t seed : {0u, 1u, 12345u}) {   // traces without a reached node (empty, or only unreached nodes): the LCG's first reached node
    const Lists g(9, 2, {{0, 1}, {1, 2}, {2, 0}, {3, 4}, {5, 6}, {7, 8}});
    const Edges x = repair_case(g, 0, {{}, {}, {}, {}, {}, {6, 7}, {}, {8}, {}}, seed, 3);
    std::vector<uint8_t> r(9, 0);
    r[0] = r[1] = r[2] = 1;
    uint64_t lcg = seed ? seed : 100;
    const uint32_t heads[3] = {3, 5, 7}, tails[3] = {4, 6, 8};
    CHECK(x.size() == 3);
    for (size_t i = 0; i < x.size() && i < 3; ++i) {
      uint32_t c;
      do {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        c = (uint32_t)((lcg >> 33) % 9);
      } while (!r[c]);
      CHECK(x[i] == std::make_pair(c, heads[i]));
      r[heads[i]] = r[tails[i]] = 1;
    }
  }
  {   // lists_to_abi: -1 behind every list's end
    const Lists g(3, 3, {{0, 2}, {0, 1}, {2, 0}});
    std::vector<int64_t> ids(9, 7);
    std::vector<int32_t> deg(3, 7);
    lists_to_abi(g.ids.data(), g.deg.data(), 3, 3, ids.data(), deg.data());
    CHECK((ids == std::vector<int64_t>{2, 1, -1, -1, -1, -1, 0, -1, -1}) && (deg == std::vector<int32_t>{2, 0, 1}));
  }
}

// ------------------------------------------------------------------------------------------------ plan
static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

static TrvIn plan_in(int64_t n, int64_t nq, int dim, int64_t L, int64_t Lq, int T, int64_t I, int degree, bool prefilter) {
  TrvIn in;
  in.n_indexed = n;
  in.nq = nq;
  in.dim = dim;
  in.master_queue = L;
  in.local_queue = Lq;
  in.intra_threads = T;
  in.sync_interval = I;
  in.fixed_deg = (degree + 3) / 4 * 4;   // (graph_upload's stride)
  in.max_degree = degree;
  in.prefilter = prefilter;
  in.cols8 = prefilter ? dim : 0;
  in.cus = 256;
  in.waves = 0;
  in.filter_in_traversal = false;
  in.filtered = false;
  in.ecap_min = 0;
  return in;
}

static void plan_sweep() {
  const int64_t MiB = 1 << 20;
  for (int T : {1, 2, 4, 8, 32, 128})
    for (int64_t Lc : {(int64_t)1, (int64_t)64, (int64_t)500, (int64_t)2000, (int64_t)4000, MiB})
      for (int64_t nq : {1, 256, 257, 1024})
        for (int dim : {7, 32, 768})
          for (int degree : {1, 32, 52, 64})
            for (int64_t n : {Lc, (int64_t)2000, (int64_t)10000000})
              for (int variant = 0; variant < 4; ++variant) {
                TrvIn in = plan_in(n, nq, dim, Lc, Lc, T, variant == 3 ? 1 : 15, degree, variant == 1);
                if (variant == 1) in.cols8 = (dim + 255) / 256 * 256;   // (the rotated frame's row)
                if (variant == 2) in.filter_in_traversal = in.filtered = true, in.ecap_min = 100000;
                TrvPlan p;
                Refusal r;
                const int32_t rc = trv_plan(in, &p, &r);
                const int dp = (in.fixed_deg + 7) / 8 * 8;
                if (T * dp > 2048) {   // the one refusal inside the sweep
                  CHECK(rc == EPS_DB_UNSUPPORTED_ERROR && r.code == rc && r.err_class == EPS_ERRCLASS_DEVICE_RANGE && r.msg.find(" > 2048 is not supported") != std::string::npos);
                  continue;
                }
                CHECK(rc == EPS_OK && r.code == EPS_OK);
                if (rc != EPS_OK) continue;
                const int64_t L = std::min(Lc, n);
                CHECK(p.L == L && p.dp == dp && p.I == in.sync_interval);
                CHECK(pow2(p.Lp2) && p.Lp2 >= L && (p.Lp2 == 1 || p.Lp2 / 2 < L));
                CHECK(T == 1 ? p.hslots == 0 : (pow2(p.hslots) && p.hslots >= 2 * T * dp));
                CHECK(p.qtot == (int64_t)(T - 1) * p.Lq + p.Lp2);
                CHECK(p.Lq <= L && p.Lq >= 1);
                if (T > 1) CHECK(p.Lq <= (L + T - 1) / T + (int64_t)p.I * dp);
                else CHECK(p.Lq == L);
                CHECK(p.shm <= (size_t)160 * 1024);
                CHECK(p.shm == traverse2_lds_bytes(dim, T, (int)p.Lq, p.qtot, dp, p.qglobal, in.prefilter, in.cols8));
                CHECK(1 <= p.slots && p.slots <= nq);
                CHECK(p.words * 32 >= n && p.slots <= (int64_t)in.cus * p.per_cu && p.per_cu >= 1 && p.per_cu * p.nw <= 16);
                CHECK(p.slots * p.words * 4 <= ((int64_t)4 << 30) || p.slots == 1);
                if (p.qglobal) CHECK(p.slots * p.qtot * 8 <= ((int64_t)8 << 30) || p.slots == 1);
                CHECK(p.ecap_plan <= n && (p.ecap_plan >= in.ecap_min || p.ecap_plan == n));
                const int64_t per_query = std::max<int64_t>(L, in.filter_in_traversal ? p.ecap_plan : 0);
                CHECK(1 <= p.slice && p.slice <= nq && (p.slice * per_query * 8 <= ((int64_t)2 << 30) || p.slice == 1));
                CHECK(p.nw == 4 || p.nw == 8 || p.nw == 16);
                CHECK(p.vcap >= 1024 && p.vcap <= (1 << 20));
              }
}

static int32_t refused(const TrvIn& in, const char* text) {
  TrvPlan p;
  Refusal r;
  const int32_t rc = trv_plan(in, &p, &r);
  if (rc == EPS_OK) {
    CHECK(r.code == EPS_OK && r.msg.empty() && text[0] == 0);
    return rc;
  }
  CHECK(rc == EPS_DB_UNSUPPORTED_ERROR && r.code == rc && r.err_class == EPS_ERRCLASS_DEVICE_RANGE);
  CHECK(r.msg == text);
  if (r.msg != text) printf("  got: %s\n", r.msg.c_str());
  return rc;
}

static void refusals() {
  const int64_t n = 10000000, M = 1 << 20;
  const char* tL = "search: SearchQueueSize > 1048576 is not supported (use the flat engines)";
  const char* tLq = "search: LocalQueueSize > 1048576 is not supported (use the flat engines)";
  const char* tT = "search: IntraQueryThreads > 128 is not supported (the reference's own limit, config/config.hpp:29)";
  CHECK(refused(plan_in(n, 4, 32, M, 500, 1, 15, 32, false), "") == EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, M + 1, 500, 1, 15, 32, false), tL) != EPS_OK);
  CHECK(refused(plan_in(M, 4, 32, 4 * M, 500, 1, 15, 32, false), "") == EPS_OK);        // clamped to n first
  CHECK(refused(plan_in(n, 4, 32, 500, M, 1, 15, 32, false), "") == EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, 500, M + 1, 1, 15, 32, false), tLq) != EPS_OK);
  CHECK(refused(plan_in(M, 4, 32, 500, 4 * M, 1, 15, 32, false), "") == EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, M + 1, M + 1, 129, 15, 32, false), tL) != EPS_OK);    // the order of the refusals: L, Lq, T, T x degree
  CHECK(refused(plan_in(n, 4, 32, 500, M + 1, 129, 15, 32, false), tLq) != EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, 500, 500, 128, 15, 16, false), "") == EPS_OK);        // 128 x 16 = 2048
  CHECK(refused(plan_in(n, 4, 32, 500, 500, 129, 15, 64, false), tT) != EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, 500, 500, 129, 15, 1, false), tT) != EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, 500, 500, 32, 15, 64, false), "") == EPS_OK);         // 32 x 64 = 2048
  CHECK(refused(plan_in(n, 4, 32, 500, 500, 33, 15, 64, false),
                "search: IntraQueryThreads x maximum out-degree (rounded up to 8) > 2048 is not supported: 33 x 64 (at the build's out-degree cap of 64: "
                "IntraQueryThreads <= 32)") != EPS_OK);
  CHECK(refused(plan_in(n, 4, 32, 500, 500, 128, 15, 17, false),
                "search: IntraQueryThreads x maximum out-degree (rounded up to 8) > 2048 is not supported: 128 x 24 (at the build's out-degree cap of 64: "
                "IntraQueryThreads <= 32)") != EPS_OK);
  TrvIn csr = plan_in(n, 4, 32, 500, 500, 4, 15, 513, false);   // a CSR graph (out-degree above 64): its longest list counts
  csr.fixed_deg = 0;
  CHECK(refused(csr, "search: IntraQueryThreads x maximum out-degree (rounded up to 8) > 2048 is not supported: 4 x 520 (at the build's out-degree cap of 64: "
                     "IntraQueryThreads <= 32)") != EPS_OK);
  csr.max_degree = 512;
  CHECK(refused(csr, "") == EPS_OK);
  // the forced wavefront count: 4, 8, 16 as given, anything else 4
  for (int w : {4, 8, 16, 5, -1, 64}) {
    TrvIn in = plan_in(n, 1024, 768, 500, 500, 4, 15, 52, true);
    in.waves = w;
    TrvPlan p;
    Refusal r;
    CHECK(trv_plan(in, &p, &r) == EPS_OK && p.nw == ((w == 8 || w == 16) ? w : 4));
  }
}

static void pinned() {   // dim 768, T = 4, I = 15, prefilter over 768 columns, n = 10^7, 256 CUs
  struct Row {
    int64_t L;
    int degree;
    int64_t nq, Lq, qtot;
    bool hbm;
    size_t lds;
    int nw, per_cu;
    int64_t slots;
  };
  const Row rows[] = {{500, 52, 1024, 500, 2012, false, 36064, 4, 4, 1024},
                      {500, 52, 1, 500, 2012, false, 36064, 16, 1, 1},
                      {2000, 64, 1024, 1460, 6428, false, 80096, 8, 2, 512},
                      {2000, 64, 64, 1460, 6428, false, 80096, 16, 1, 64},
                      {4000, 64, 1024, 1960, 9976, true, 49760, 8, 2, 512}};
  for (const Row& w : rows) {
    TrvPlan p;
    Refusal r;
    CHECK(trv_plan(plan_in(10000000, w.nq, 768, w.L, w.L, 4, 15, w.degree, true), &p, &r) == EPS_OK);
    CHECK(p.Lq == w.Lq && p.qtot == w.qtot && p.qglobal == w.hbm && p.shm == w.lds && p.nw == w.nw && p.per_cu == w.per_cu && p.slots == w.slots);
    if (!(p.Lq == w.Lq && p.qtot == w.qtot && p.qglobal == w.hbm && p.shm == w.lds && p.nw == w.nw && p.per_cu == w.per_cu && p.slots == w.slots))
      printf("  L=%lld nq=%lld: Lq %lld qtot %lld %s LDS %zu nw %d per CU %d slots %lld\n", (long long)w.L, (long long)w.nq, (long long)p.Lq, (long long)p.qtot,
             p.qglobal ? "HBM" : "LDS", p.shm, p.nw, p.per_cu, (long long)p.slots);
  }
}

// the filtered traversal's evaluation log, at the exact inputs of the repeat case of tests/filtered_walk_ref.py (REPEAT: 40000 x 16, 12 queries,
// out-degree 96, T = 4, L = 180, I = 15): the first attempt's log is the floor of 16384 slots; the oracle's longest walk there evaluates 17497
// rows, graph_search_impl asks the second attempt for min(n, 17497 + 17497 / 4 + 1024) = 22895 and the plan grants exactly that
static TrvIn log_in(int64_t n, int64_t nq, int64_t L, int64_t ecap_min) {
  TrvIn in = plan_in(n, nq, 16, L, L, 4, 15, 96, false);
  in.filter_in_traversal = in.filtered = true;
  in.ecap_min = ecap_min;
  return in;
}

static void repeat_log() {
  TrvPlan p;
  Refusal r;
  CHECK(trv_plan(log_in(40000, 12, 180, 0), &p, &r) == EPS_OK && p.ecap_plan == 16384 && p.slice == 12 && p.dp == 96);
  CHECK(trv_plan(log_in(40000, 12, 180, 22895), &p, &r) == EPS_OK && p.ecap_plan == 22895 && p.slice == 12);
  CHECK(trv_plan(log_in(40000, 12, 180, 50000), &p, &r) == EPS_OK && p.ecap_plan == 40000);                    // never beyond n: a walk evaluates a row once
  CHECK(trv_plan(log_in(40000, 12, 256, 0), &p, &r) == EPS_OK && p.ecap_plan == 16384);                        // 64 L = the floor
  CHECK(trv_plan(log_in(40000, 12, 257, 0), &p, &r) == EPS_OK && p.ecap_plan == 64 * 257);
  CHECK(trv_plan(log_in(12000, 6, 2500, 0), &p, &r) == EPS_OK && p.ecap_plan == 12000);                        // clamped to the table
  CHECK(trv_plan(log_in(2000, 24, 500, 0), &p, &r) == EPS_OK && p.ecap_plan == 2000);
}

// What two groups of tests/filtered_walk_ref.py rely on, on 256 CUs, at every out-degree a graph of theirs can have.
// Group h's tiled step (2000 x 16, T = 4, L = 500, H_TILED = 1100 queries): 4 wavefronts per query, 4 workgroups per CU, 1024 workgroups in one
// launch of 1100 queries - fewer than the queries, so workgroups walk a second query; the 300 queries of the unfiltered width case get one each.
// Group e (12000 x 24, (T, L) = (4, 2500), (1, 12000) and (1, 9000)): a call of 6 queries keeps these queues in LDS (the 150 KB limit of up to 256
// queries), the E_TILED = 264 queries of the tests send them to HBM (the 80 KB limit of a batch).
static void shared_slots_and_hbm() {
  TrvPlan p;
  Refusal r;
  for (int degree : {32, 50, 52, 60, 64})
    for (int filtered = 0; filtered < 2; ++filtered) {
      TrvIn in = plan_in(2000, 1100, 16, 500, 500, 4, 15, degree, false);
      in.filter_in_traversal = in.filtered = filtered != 0;
      CHECK(trv_plan(in, &p, &r) == EPS_OK && p.nw == 4 && p.per_cu == 4 && p.slots == 1024 && p.slots < in.nq && p.slice == 1100 && !p.qglobal);
      in.nq = 300;
      CHECK(trv_plan(in, &p, &r) == EPS_OK && p.slots == 300 && p.slice == 300);
      for (int which = 0; which < 3; ++which) {
        const int64_t eL = which == 0 ? 2500 : (which == 1 ? 12000 : 9000);
        TrvIn e = plan_in(12000, 264, 24, eL, eL, which ? 1 : 4, 15, std::max(degree, 50), false);
        e.filter_in_traversal = e.filtered = filtered != 0;
        CHECK(trv_plan(e, &p, &r) == EPS_OK && p.qglobal && p.nw == 8 && p.slots == 264 && p.slice == 264 && p.ecap_plan == 12000);
        e.nq = 6;
        CHECK(trv_plan(e, &p, &r) == EPS_OK && !p.qglobal && p.nw == 16 && p.slots == 6);
      }
    }
}

static int ecap_of(int64_t n, int64_t nq, int64_t L, int64_t ecap_min) {
  TrvPlan p;
  Refusal r;
  if (n < 1 || nq < 1 || L < 1 || ecap_min < 0 || trv_plan(log_in(n, nq, L, ecap_min), &p, &r) != EPS_OK) return printf("bad arguments\n"), 2;
  printf("%lld\n", (long long)p.ecap_plan);
  return 0;
}

static void tails() {
  TailPlan t;
  Refusal r;
  // no tail: nothing staged, K = min(n, limit, LocalQueueSize, L)
  CHECK(tail_plan(2000, 2000, 500, 300, 10, 0, &t, &r) == EPS_OK);
  CHECK(t.tail_k == 10 && t.K == 10 && t.Klds == 0 && t.Kout == 10 && t.cand_num == 500 && t.cand_num_tail == 500);
  CHECK(tail_plan(2000, 2100, 500, 7, 10, 0, &t, &r) == EPS_OK);
  CHECK(t.tail_k == 10 && t.K == 7 && t.Klds == 7 && t.Kout == 7 && t.cand_num == 500 && t.cand_num_tail == 500);
  CHECK(tail_plan(5, 9, 5, 300, 10, 0, &t, &r) == EPS_OK);
  CHECK(t.K == 5 && t.Klds == 5 && t.Kout == 5 && t.cand_num == 5 && t.cand_num_tail == 5);
  CHECK(tail_plan(5, 9, 8, 300, 10, 0, &t, &r) == EPS_OK && t.cand_num == 5 && t.cand_num_tail == 8);
  // the walk form: k = the caller's cap, the walk's limit decides K and the tail list
  CHECK(tail_plan(2000, 2100, 500, 300, 64, 20, &t, &r) == EPS_OK);
  CHECK(t.tail_k == 20 && t.K == 20 && t.Klds == 20 && t.Kout == 64);
  // limit beyond 8192: without a tail as it is, with a tail refused - unless a queue is shorter anyway
  CHECK(tail_plan(100000, 100000, 20000, 20000, 9000, 0, &t, &r) == EPS_OK && t.K == 9000 && t.Klds == 0 && t.tail_k == 8192);
  CHECK(tail_plan(100000, 100001, 20000, 20000, 8192, 0, &t, &r) == EPS_OK && t.K == 8192 && t.Klds == 8192);
  CHECK(tail_plan(100000, 100001, 20000, 8192, 9000, 0, &t, &r) == EPS_OK && t.K == 8192);
  CHECK(tail_plan(100000, 100001, 20000, 20000, 8193, 0, &t, &r) == EPS_DB_UNSUPPORTED_ERROR && r.code == EPS_DB_UNSUPPORTED_ERROR && r.err_class == 0);
  CHECK(r.msg == "search: limit > 8192 with an un-indexed tail is not supported (rebuild the graph over the new rows)");
}

// ------------------------------------------------------------------------------------------------ LDS of the build's launches
static void build_lds() {
  const size_t KB = 1024, dev = 160 * KB;   // a gfx950 workgroup's LDS
  // SelectEdge at out_degree 50: 20 bytes per (padded) dimension, the pool, kept lists, scalars
  CHECK(prune_lds_bytes(768, 50) == 48800 && prune_lds_bytes(4096, 50) == 115360 && prune_lds_bytes(6520, 50) == 163840 && prune_lds_bytes(8192, 50) == 197280);
  CHECK(prune_lds_bytes(765, 50) == prune_lds_bytes(768, 50) && prune_lds_bytes(769, 50) == prune_lds_bytes(772, 50));
  CHECK(prune_lds_bytes(768, 512) == 48800 + 8 * 462);
  // Link's search: 4 bytes per dimension, queue, chunk buffers, scalars; + the LDS visited hash, + the prefilter's block
  CHECK(traverse_lds_bytes(768, 512, false) == 3072 + 4096 + 4096 + 1024 + 256);
  CHECK(traverse_lds_bytes(768, 512, true) == traverse_lds_bytes(768, 512, false) + 32768);
  CHECK(traverse_lds_bytes(768, 2048, false, true, 768) == 3072 + 16384 + 4096 + 1024 + 256 + 32 + 768);
  CHECK(traverse_lds_bytes(770, 512, false, true, 1024) == 3088 + 4096 + 4096 + 1024 + 256 + 32 + 1024);
  CHECK(traverse_lds_bytes(8192, 2048, true, true, 8192) == 32768 + 16384 + 4096 + 1024 + 256 + 32768 + 32 + 8192);   // (95 KB: SelectEdge is the larger at every width)
  for (int dim : {1, 768, 4096, 6520, 8192})
    for (int R : {1, 50, 512})
      CHECK(build_lds_need(dim, R, 2048, true, true, dim) == std::max(prune_lds_bytes(dim, R), traverse_lds_bytes(dim, 2048, true, true, dim)));
  // the check: what fits passes untouched, what does not is refused with the width that would
  for (int dim : {768, 4096, 6520}) {
    Refusal r;
    CHECK(build_lds_check(dim, 50, 512, false, false, 0, dev, &r) == EPS_OK && r.code == EPS_OK && r.msg.empty());
  }
  for (int dim : {6521, 6524, 8192}) {
    Refusal r;
    CHECK(build_lds_check(dim, 50, 512, false, false, 0, dev, &r) == EPS_DB_UNSUPPORTED_ERROR && r.code == EPS_DB_UNSUPPORTED_ERROR && r.err_class == EPS_ERRCLASS_DEVICE_RANGE);
    CHECK(r.msg.find("width limit of the graph build at out_degree 50: 6520 dimensions") != std::string::npos);
    CHECK(r.msg.find("rows of " + std::to_string(dim) + " dimensions need " + std::to_string(prune_lds_bytes(dim, 50)) + " bytes of LDS per workgroup, the device has 163840") != std::string::npos);
  }
  {   // out_degree moves the limit; a device with 64 KB has its own
    Refusal r;
    CHECK(build_lds_check(6520, 512, 512, false, false, 0, dev, &r) == EPS_DB_UNSUPPORTED_ERROR && r.msg.find("out_degree 512: 6332 dimensions") != std::string::npos);
    Refusal r2;
    CHECK(build_lds_check(2048, 50, 512, false, false, 0, 64 * KB, &r2) == EPS_DB_UNSUPPORTED_ERROR && r2.msg.find(": 1604 dimensions") != std::string::npos);
    Refusal r3;
    CHECK(build_lds_check(1604, 50, 512, false, false, 0, 64 * KB, &r3) == EPS_OK);
  }
}

// ------------------------------------------------------------------------------------------------ LDS layouts
// the three byte totals as they stood before the layouts were structs, kept here as the reference
static size_t old_prune_bytes(int dim, int R) {
  return (size_t)((dim + 3) & ~3) * 4 + (size_t)PRUNE_POOL * 8 + (size_t)R * 8 + 64 * 4 + 16 + (size_t)4 * ((dim + 3) & ~3) * 4;
}
static size_t old_traverse_bytes(int dim, int Lp2, bool hashvis, bool prefilter, int cols8) {
  const int qstride = (dim + 3) & ~3;
  return (size_t)qstride * 4 + (size_t)Lp2 * 8 + TRV_CHUNK * 8 * 2 + TRV_CHUNK * 4 + 64 * 4 + (hashvis ? TRV_HASH * 4 : 0) +
         (prefilter ? (size_t)(16 + 16 + (((cols8 > dim ? cols8 : dim) + 15) & ~15)) : 0);
}
static size_t old_traverse2_bytes(int dim, int T, int Lq, int64_t qtot, int dp, bool qglobal, bool prefilter, int cols8) {
  const int qstride = (dim + 3) & ~3;
  const size_t ecap = (size_t)T * dp;
  const int wide = cols8 > dim ? cols8 : dim;
  return (size_t)qstride * 4 + (qglobal ? (size_t)TRV2_SB : (size_t)qtot) * 8 + ecap * (8 + 8 + 4 + 4 + 4 + 4) + (size_t)traverse2_hash_slots(T, dp) * 8 +
         ((qglobal || T == 1) ? 0 : (size_t)2 * Lq * 4) + (size_t)trv2_sh_ints(T) * 4 + (prefilter ? (size_t)(16 + 16 + ((wide + 15) & ~15)) : 0);
}

struct Field {
  const char* name;
  size_t at, bytes, align;
};
// the arrays of a layout in field order: ascending, disjoint, each aligned to its element type, the last one inside the total
static void fields_fit(const std::vector<Field>& f, size_t total) {
  size_t end = 0;
  for (const Field& x : f) {
    CHECK(x.at >= end);
    CHECK(x.at % x.align == 0);
    if (x.at < end || x.at % x.align) printf("  field %s at %zu (%zu bytes), previous end %zu\n", x.name, x.at, x.bytes, end);
    end = x.at + x.bytes;
  }
  CHECK(end <= total);
}
static void inside(size_t at, size_t bytes, size_t align, size_t host, size_t host_bytes) {   // an overlay lies wholly inside the array it names
  CHECK(at % align == 0 && at >= host && at + bytes <= host + host_bytes);
}

static void lds_layouts() {
  const int dims[] = {1, 19, 32, 130, 768, 772, 1552, 8192};
  for (int dim : dims) {
    const size_t qrow = (size_t)((dim + 3) / 4 * 4) * 4;
    const int cols_cases[] = {-1, dim, (dim + 255) / 256 * 256 + 256};   // prefilter off, on, on with cols8 > dim
    for (int R : {50, 512}) {
      const PruneLds l = prune_lds(dim, R);
      fields_fit({{"sq", l.sq, qrow, 16}, {"pool", l.pool, (size_t)PRUNE_POOL * 8, 8}, {"kept", l.kept, (size_t)R * 4, 4}, {"keptd", l.keptd, (size_t)R * 4, 4},
                  {"sh", l.sh, 64 * 4, 4}, {"sqb", l.sqb, PRUNE_PB * qrow, 16}},
                 l.total);
      CHECK(l.total == old_prune_bytes(dim, R) && prune_lds_bytes(dim, R) == l.total);
    }
    for (int cols8 : cols_cases) {
      const bool pf = cols8 >= 0;
      const size_t q8 = pf ? (size_t)((std::max(dim, cols8) + 15) / 16 * 16) : 0;
      for (int Lp2 : {512, 2048})
        for (int hash_in_lds = 0; hash_in_lds < 2; ++hash_in_lds) {
          const TrvLds l = traverse_lds(dim, Lp2, hash_in_lds != 0, pf, pf ? cols8 : 0);
          std::vector<Field> f = {{"sq", l.sq, qrow, 16},          {"queue", l.queue, (size_t)Lp2 * 8, 8},  {"newk", l.newk, TRV_CHUNK * 8, 8},
                                  {"sorted", l.sorted, TRV_CHUNK * 8, 8}, {"work", l.work, TRV_CHUNK * 4, 4}, {"sh", l.sh, 64 * 4, 4},
                                  {"hash", l.hash, hash_in_lds ? (size_t)TRV_HASH * 4 : 0, 4}};
          if (pf) {
            f.push_back({"qst", l.pf.qst, 16, 16});
            f.push_back({"sq8", l.pf.sq8, q8, 16});
            CHECK((size_t)q8_bytes(dim, cols8) == q8);
          }
          fields_fit(f, l.total);
          inside(l.surv, TRV_CHUNK * 4, 4, l.sorted, TRV_CHUNK * 8);
          CHECK(l.total == old_traverse_bytes(dim, Lp2, hash_in_lds != 0, pf, pf ? cols8 : 0) && traverse_lds_bytes(dim, Lp2, hash_in_lds != 0, pf, pf ? cols8 : 0) == l.total);
        }
      for (int T : {1, 2, 4, 17, 32, 128})
        for (int dp : {8, 56, 64, 2048})
          for (int qglobal = 0; qglobal < 2; ++qglobal) {
            if (T * dp > 2048) continue;   // (trv_queues refuses it)
            const int Lq = 137;
            const int64_t qtot = (int64_t)(T - 1) * Lq + 512;
            const size_t ecap = (size_t)T * dp, H = (size_t)traverse2_hash_slots(T, dp);
            const Trv2Lds l = traverse2_lds(dim, T, Lq, qtot, dp, qglobal != 0, pf, pf ? cols8 : 0);
            std::vector<Field> f = {{"sq", l.sq, qrow, 16},
                                    {"qlds", l.qlds, (qglobal ? (size_t)TRV2_SB : (size_t)qtot) * 8, 8},
                                    {"newk", l.newk, ecap * 8, 8},
                                    {"sorted", l.sorted, ecap * 8, 8},
                                    {"eid", l.eid, ecap * 4, 4},
                                    {"eraw", l.eraw, ecap * 4, 4},
                                    {"work", l.work, ecap * 4, 4},
                                    {"npos", l.npos, ecap * 4, 4},
                                    {"hid", l.hid, H * 4, 4},
                                    {"hmin", l.hmin, H * 4, 4},
                                    {"auxl", l.auxl, (qglobal || T == 1) ? 0 : (size_t)2 * Lq * 4, 4},
                                    {"sh", l.sh, (size_t)trv2_sh_ints(T) * 4, 4}};
            if (pf) {
              f.push_back({"qst", l.pf.qst, 16, 16});
              f.push_back({"sq8", l.pf.sq8, q8, 16});
            }
            fields_fit(f, l.total);
            CHECK((size_t)l.H == H);
            inside(l.eacc, ecap * 4, 4, l.newk, ecap * 8);
            inside(l.wacc, ecap * 4, 4, l.newk, ecap * 8);
            CHECK(l.wacc >= l.eacc + ecap * 4);
            inside(l.wwk, ecap * 4, 4, l.sorted, ecap * 4);             // the first half of `sorted` ...
            inside(l.surv, ecap * 4, 4, l.sorted + ecap * 4, ecap * 4);   // ... and its second half
            CHECK(l.total == old_traverse2_bytes(dim, T, Lq, qtot, dp, qglobal != 0, pf, pf ? cols8 : 0));
            CHECK(traverse2_lds_bytes(dim, T, Lq, qtot, dp, qglobal != 0, pf, pf ? cols8 : 0) == l.total);
          }
    }
  }
  // the scalar slots stay inside their arrays
  CHECK(TRV_NODE + TRV_MAXM <= TRV_EDGE0 && TRV_EDGE0 + TRV_MAXM + 1 <= TRV_TQ && TRV_FP32 < TRV_WAVE && TRV_WAVE + 4 <= 64);
  CHECK(PRN_WAVE + 4 <= PRN_POS && PRN_POS + PRUNE_PB <= PRN_KEPT_CLOSER && PRN_KEPT_CLOSER + PRUNE_PB <= PRN_PEER_CLOSER && PRN_PEER_CLOSER + PRUNE_PB * PRUNE_PB <= 64);
  CHECK(TRV2_NEVAL < 16);
  // the 60 % rule: more than 60 % of the neighbour evaluations still read the fp32 row -> the test does not pay; nothing evaluated: no verdict
  CHECK(prefilter_pays(1000, 600) && !prefilter_pays(1000, 601) && prefilter_pays(1000, 0) && !prefilter_pays(1000, 1000));
  CHECK(prefilter_pays(0, 0) && prefilter_pays(0, 5) && !prefilter_pays(5, 4) && prefilter_pays(5, 3));
}

// ------------------------------------------------------------------------------------------------ seeds of a graph in a file
static int seeds_of_file(const char* path, int64_t L) {
  FILE* f = fopen(path, "rb");
  if (!f) return printf("cannot open %s\n", path), 2;
  int64_t head[2] = {0, 0};
  if (fread(head, 8, 2, f) != 2 || head[0] < 1 || head[1] < 0 || head[1] >= head[0] || L < 1 || L > head[0]) return fclose(f), printf("bad header\n"), 2;
  const int64_t n = head[0], nav = head[1];
  std::vector<int64_t> off((size_t)n + 1);
  if (fread(off.data(), 8, off.size(), f) != off.size() || off[0] != 0 || off[n] < 0) return fclose(f), printf("bad offsets\n"), 2;
  std::vector<int64_t> nbr((size_t)off[n]);
  if (fread(nbr.data(), 8, nbr.size(), f) != nbr.size()) return fclose(f), printf("bad neighbours\n"), 2;
  fclose(f);
  std::vector<uint32_t> out;
  seed_list(nbr.data() + off[nav], off[nav + 1] - off[nav], nav, n, L, out);
  for (uint32_t v : out) printf("%u ", v);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "seeds") == 0) return seeds_of_file(argv[2], atoll(argv[3]));
  if (argc == 6 && strcmp(argv[1], "ecap") == 0) return ecap_of(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]));
  seeds();
  repair();
  plan_sweep();
  refusals();
  pinned();
  repeat_log();
  shared_slots_and_hbm();
  tails();
  build_lds();
  lds_layouts();
  if (failures) {
    printf("graph_host_check: %d check(s) failed\n", failures);
    return 1;
  }
  printf("graph_host_check OK\n");
  return 0;
}
