// Stand-alone check of vectordb_amd/csrc/filters_host.hpp (built with -fsanitize=address,undefined by tests/test_filters_ref_cpu.py): the programs'
// validation, planes of identical texts, the queries' sort and its inverse, chunking of 0 / 1 / chunk / chunk + 1 entries, the item table, AUTO.
#include <stdio.h>
#include <stdlib.h>

#include "../../vectordb_amd/csrc/filters_host.hpp"

using namespace eps;

#define CHECK(c) if (!(c)) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c), exit(1)

static eps_filter_op op(int32_t o, int32_t arg = 0, double v = 0.0) { return eps_filter_op{o, arg, 0, v}; }

static void check_programs() {
  const char* why;
  // program 0: i32@0 == 17; 1: empty; 2: the same text as 0; 3: f64@4 < 0.5
  std::vector<eps_filter_op> ops = {op(EPS_FOP_PUSH_I32, 0), op(EPS_FOP_PUSH_CONST, 0, 17), op(EPS_FOP_EQ), op(EPS_FOP_PUSH_I32, 0), op(EPS_FOP_PUSH_CONST, 0, 17),
                                    op(EPS_FOP_EQ),          op(EPS_FOP_PUSH_F64, 4),       op(EPS_FOP_PUSH_CONST, 0, 0.5), op(EPS_FOP_LT)};
  const int32_t off[] = {0, 3, 3, 6, 9};
  CHECK(filters_programs_check(ops.data(), off, 4, 12, &why) == EPS_OK);
  CHECK(filters_programs_check(ops.data(), off, 4, 11, &why) == EPS_USER_ERROR);   // the double ends at byte 12
  CHECK(filters_programs_check(ops.data(), off, 0, 12, &why) == EPS_USER_ERROR && filters_programs_check(ops.data(), off, 65, 12, &why) == EPS_USER_ERROR);
  const int32_t bad0[] = {1, 3}, bad1[] = {0, 3, 2}, one[] = {0, 1};
  CHECK(filters_programs_check(ops.data(), bad0, 1, 12, &why) == EPS_USER_ERROR && filters_programs_check(ops.data(), bad1, 2, 12, &why) == EPS_USER_ERROR);
  const eps_filter_op dist = op(EPS_FOP_PUSH_DIST), cmp = op(EPS_FOP_EQ);
  CHECK(filters_programs_check(&dist, one, 1, 12, &why) == EPS_USER_ERROR && filters_programs_check(&cmp, one, 1, 12, &why) == EPS_USER_ERROR);
  const int32_t empty[] = {0, 0};
  CHECK(filters_programs_check(nullptr, empty, 1, 0, &why) == EPS_OK);   // only the empty program: no rows, no instructions
  CHECK(filters_programs_check(ops.data(), one, 1, 0, &why) == EPS_USER_ERROR);
  std::vector<eps_filter_op> longp(65, op(EPS_FOP_PUSH_CONST));
  const int32_t l65[] = {0, 65};
  CHECK(filters_programs_check(longp.data(), l65, 1, 12, &why) == EPS_DB_UNSUPPORTED_ERROR);

  // planes, the sort and its inverse: queries of program 2 land on plane 0 after program 0's, in the caller's order
  const int32_t qp[] = {3, 0, 2, 1, 0, 3, 2};
  FiltersPlan p;
  CHECK(filters_plan_queries(ops.data(), off, 4, qp, 7, &p, &why) == EPS_OK);
  CHECK(p.planes == 3 && p.plane_of_prog == (std::vector<int32_t>{0, 1, 0, 2}) && p.prog_of_plane == (std::vector<int32_t>{0, 1, 3}));
  CHECK(p.op_off == (std::vector<int32_t>{0, 3, 3, 6}) && p.pass_begin == (std::vector<int32_t>{0, 3}));
  CHECK(p.plane_q0 == (std::vector<int32_t>{0, 4, 5, 7}) && p.order == (std::vector<int32_t>{1, 2, 4, 6, 3, 0, 5}));
  for (int32_t q = 0; q < 7; ++q) CHECK(p.order[(size_t)p.inverse[(size_t)q]] == q);
  const int32_t out_of_range[] = {0, 4}, negative[] = {-1};
  CHECK(filters_plan_queries(ops.data(), off, 4, out_of_range, 2, &p, &why) == EPS_USER_ERROR && filters_plan_queries(ops.data(), off, 4, negative, 1, &p, &why) == EPS_USER_ERROR);
  CHECK(filters_plan_queries(ops.data(), off, 4, qp, 0, &p, &why) == EPS_OK && p.order.empty() && p.plane_q0.back() == 0);
}

static void check_chunking() {
  int32_t chunk, waves;
  const int64_t lens[] = {0, 1, FILTERS_CHUNK, FILTERS_CHUNK + 1, 4 * FILTERS_CHUNK, 4 * FILTERS_CHUNK + 1, 1000000, ((int64_t)1 << 31) - 1};
  for (int32_t k : {1, 10, 100, 1024})
    for (int64_t len : lens) {
      filters_chunking(len, k, &chunk, &waves);
      CHECK(chunk >= FILTERS_CHUNK && waves % FILTERS_BLOCK_WAVES == 0 && (int64_t)waves * chunk >= len);
      CHECK((int64_t)waves * k <= FILTERS_MERGE_KEYS && waves <= FILTERS_MAX_WAVES);
      CHECK(len > 0 ? (int64_t)(waves - FILTERS_BLOCK_WAVES) * chunk < len : waves == 0);   // no workgroup wholly beyond the list
    }
}

static void check_engines() {
  const char* why;   // planes: 0 with 5 queries, 1 with none, 2 with 1 query, 3 with 4 queries
  std::vector<eps_filter_op> ops = {op(EPS_FOP_PUSH_CONST, 0, 1), op(EPS_FOP_PUSH_CONST, 0, 2), op(EPS_FOP_PUSH_CONST, 0, 3)};
  const int32_t off[] = {0, 0, 1, 2, 3};
  const int32_t qp[] = {0, 3, 0, 3, 2, 0, 3, 0, 3, 0};
  FiltersPlan p;
  CHECK(filters_plan_queries(ops.data(), off, 4, qp, 10, &p, &why) == EPS_OK && p.planes == 4);
  const int64_t counts[] = {3001, 7, 0, 513};
  filters_plan_engines(&p, counts, 3001, 10, 4, EPS_FILTERS_LISTS, nullptr, 0);
  CHECK(p.engine == (std::vector<int32_t>{1, 0, 1, 1}) && p.list_total == 3001 + 0 + 513 && p.list_queries == 10 && p.list_evals == 5 * 3001 + 4 * 513);
  CHECK(p.list_begin[3] == 3001 && p.blocks.size() == 4);   // 4 + 1 queries of plane 0, 1 of plane 2, 4 of plane 3
  CHECK(p.blocks[0].nq == 4 && p.blocks[1].nq == 1 && p.blocks[1].q0 == 4 && p.blocks[2].list_len == 0 && p.blocks[2].waves == 0 && p.blocks[3].waves == 4);
  CHECK(p.blocks[0].waves == 8 && p.blocks[1].wave0 == 8 && p.blocks[2].wave0 == 16 && p.blocks[3].wave0 == 16 && p.partial_waves == 20);
  CHECK(p.items.size() == 2 + 2 + 0 + 1 && p.items[4].block == 3 && p.items[4].group == 0 && p.items[3].block == 1 && p.items[3].group == 1);
  for (const FiltersItem& it : p.items) CHECK((int64_t)it.group * FILTERS_BLOCK_WAVES * p.blocks[(size_t)it.block].chunk < p.blocks[(size_t)it.block].list_len);
  for (size_t s = 0; s < 10; ++s) CHECK(p.block_of[s] >= 0 && (int32_t)s >= p.blocks[(size_t)p.block_of[s]].q0 && (int32_t)s < p.blocks[(size_t)p.block_of[s]].q0 + p.blocks[(size_t)p.block_of[s]].nq);
  // AUTO: a dense plane the matrix engine would serve goes to it (513 of 3001 rows, one block: 17 % < 40 %); the rest while the scratch lasts
  const bool matrix[] = {true, true, true, true};
  filters_plan_engines(&p, counts, 3001, 10, 4, EPS_FILTERS_AUTO, matrix, FILTERS_SCRATCH_BYTES);
  CHECK(p.engine == (std::vector<int32_t>{2, 0, 1, 1}) && filters_dense(100001, 1000000, 16) && !filters_dense(100000, 1000000, 16) && filters_dense(25001, 1000000, 256));
  const int64_t first = filters_list_bytes(3001, 5, 10, 4);
  filters_plan_engines(&p, counts, 3001, 10, 4, EPS_FILTERS_AUTO, nullptr, first);   // room for plane 0's lists and an empty one only
  CHECK(p.engine == (std::vector<int32_t>{1, 0, 1, 2}));
  filters_plan_engines(&p, counts, 3001, 10, 4, EPS_FILTERS_AUTO, nullptr, first - 1);
  CHECK(p.engine == (std::vector<int32_t>{2, 0, 1, 1}));
}

int main() { return check_programs(), check_chunking(), check_engines(), printf("filters_host_check OK\n"), 0; }
