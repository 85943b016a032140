// Stand-alone host check of csrc/diverse_host.hpp - the argument checks and the LDS layout of diverse_select_kernel - for a CPU build under
// -fsanitize=address,undefined (tests/test_diverse_ref_cpu.py builds and runs it).  The layout is walked over every (fetch_k, dim) corner:
// fetch_k 1, 63, 64, 65, 1024 by dim 1, 3, 4, 7, 768, 8192.  At every point the regions are disjoint, each starts at a multiple of its element
// size (the row at 16 bytes: it is read in 16-byte pieces), the total stays within the 64 KB a launch gets without an attribute, and every element
// the kernel indexes is written into a heap block of exactly the planned size: an element beyond the plan is a heap overflow the sanitizer reports.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../vectordb_amd/csrc/diverse_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

static void arguments() {
  const char* why = nullptr;
  CHECK(diverse_args_check(0, 1, 1, 0.5f, &why) == EPS_OK);
  CHECK(diverse_args_check(7, 1024, 1024, 0.0f, &why) == EPS_OK);
  CHECK(diverse_args_check(7, 10, 100, 1.0f, &why) == EPS_OK);
  CHECK(diverse_args_check(7, 10, 100, -0.0f, &why) == EPS_OK);
  CHECK(diverse_args_check(-1, 1, 1, 0.5f, &why) == EPS_USER_ERROR && strstr(why, "nq"));
  CHECK(diverse_args_check(1, 0, 10, 0.5f, &why) == EPS_USER_ERROR && strstr(why, "fetch_k"));
  CHECK(diverse_args_check(1, -3, 10, 0.5f, &why) == EPS_USER_ERROR && strstr(why, "fetch_k"));
  CHECK(diverse_args_check(1, 11, 10, 0.5f, &why) == EPS_USER_ERROR && strstr(why, "fetch_k"));
  CHECK(diverse_args_check(1, 1, 1025, 0.5f, &why) == EPS_USER_ERROR && strstr(why, "fetch_k"));
  CHECK(diverse_args_check(1, 1, 0, 0.5f, &why) == EPS_USER_ERROR && strstr(why, "fetch_k"));
  CHECK(diverse_args_check(1, 1, 10, -0.1f, &why) == EPS_USER_ERROR && strstr(why, "lambda"));
  CHECK(diverse_args_check(1, 1, 10, 1.5f, &why) == EPS_USER_ERROR && strstr(why, "lambda"));
  CHECK(diverse_args_check(1, 1, 10, nanf(""), &why) == EPS_USER_ERROR && strstr(why, "lambda"));
  CHECK(diverse_args_check(1, 1, 10, INFINITY, &why) == EPS_USER_ERROR && strstr(why, "lambda"));
}

struct Region {
  int off, bytes, align;
};

static void layout() {
  const int fetch[] = {1, 63, 64, 65, 1024}, dims[] = {1, 3, 4, 7, 768, 8192};
  for (int fetch_k : fetch)
    for (int dim : dims) {
      const DiverseLds L = diverse_lds(fetch_k, dim);
      const int qstride = (dim + 3) & ~3;
      std::vector<Region> r = {{L.row, qstride * 4, 16}, {L.keys, fetch_k * 8, 8}, {L.red, DIVERSE_WAVES * 8, 8}, {L.m, fetch_k * 4, 4}, {L.taken, fetch_k, 1}};
      for (const Region& a : r) {
        CHECK(a.off >= 0 && a.off % a.align == 0);
        CHECK(a.off + a.bytes <= L.bytes);
      }
      std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
      for (size_t i = 0; i + 1 < r.size(); ++i) CHECK(r[i].off + r[i].bytes <= r[i + 1].off);   // disjoint
      CHECK(L.bytes % 16 == 0 && (int64_t)L.bytes <= DIVERSE_LDS_BUDGET);
      // the kernel's own indexing, into a block of exactly L.bytes
      unsigned char* lds = static_cast<unsigned char*>(aligned_alloc(16, (size_t)L.bytes));
      CHECK(lds != nullptr);
      if (!lds) continue;
      memset(lds, 0xAB, (size_t)L.bytes);
      float* srow = reinterpret_cast<float*>(lds + L.row);
      unsigned long long* keys = reinterpret_cast<unsigned long long*>(lds + L.keys);
      unsigned long long* red = reinterpret_cast<unsigned long long*>(lds + L.red);
      float* m = reinterpret_cast<float*>(lds + L.m);
      unsigned char* taken = lds + L.taken;
      for (int i = 0; i < qstride; ++i) srow[i] = 1.f;
      for (int i = 0; i < fetch_k; ++i) {
        keys[i] = ~0ull;
        m[i] = 2.f;
        taken[i] = 1;
      }
      for (int w = 0; w < DIVERSE_WAVES; ++w) red[w] = 3ull;
      // nothing written through one region shows in another
      bool clean = true;
      for (int i = 0; i < qstride; ++i) clean &= srow[i] == 1.f;
      for (int i = 0; i < fetch_k; ++i) clean &= keys[i] == ~0ull && m[i] == 2.f && taken[i] == 1;
      for (int w = 0; w < DIVERSE_WAVES; ++w) clean &= red[w] == 3ull;
      CHECK(clean);
      free(lds);
    }
  CHECK(diverse_lds(1024, 8192).bytes == 32768 + 8192 + 32 + 4096 + 1024);   // the largest launch: 46 112 bytes
}

int main() {
  arguments();
  layout();
  if (failures) {
    printf("diverse_host_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("diverse_host_check OK\n");
  return 0;
}
