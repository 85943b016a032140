// Stand-alone host check of csrc/result_block.hpp - the layout of a serving call's result block - for a CPU build under
// -fsanitize=address,undefined (tests/test_result_block_cpu.py builds and runs it).  Every call's part list (csrc/index_calls.cpp) over small nq, k,
// m and cap, odd products among them: the parts do not overlap, each starts at a multiple of its element size, the block ends where the last part
// ends, and split() fills exactly the arrays asked for - each a heap block of exactly its size, the block itself too, so a part that reaches past
// either is a heap overflow the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../vectordb_amd/csrc/result_block.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

using namespace eps;

struct FakeBuf {   // what place() asks of a device buffer
  void* p = nullptr;
  size_t cap = 0;
  bool fail = false;
  bool reserve(size_t bytes) {
    if (fail) return false;
    if (bytes <= cap) return true;
    free(p);
    p = malloc(bytes);   // exactly: one byte further is caught
    cap = bytes;
    return p != nullptr;
  }
  ~FakeBuf() { free(p); }
};

struct Spec {   // one output of a call: element size, element count, and whether the caller asked for it
  size_t elem, count;
  bool wanted;
};

static unsigned char pattern(int part, size_t byte) { return (unsigned char)(part * 37 + byte * 11 + 1); }

template <class T>
static ResultBlock::Ref<T> add_as(ResultBlock& rb, void* dst, size_t count) {
  return rb.add(static_cast<T*>(dst), count);
}

// the block of `specs` as a host call lays it out, checked; then as a device call sees it
static void check_call(const char* who, const std::vector<Spec>& specs) {
  std::vector<void*> dst;
  for (const Spec& s : specs) dst.push_back(s.wanted ? malloc(s.elem * s.count + (s.count == 0)) : nullptr);
  ResultBlock rb;
  std::vector<void*> dev;
  std::vector<int> ref;
  for (size_t i = 0; i < specs.size(); ++i)
    ref.push_back(specs[i].elem == 8 ? add_as<int64_t>(rb, dst[i], specs[i].count).i : add_as<int32_t>(rb, dst[i], specs[i].count).i);
  CHECK(rb.size() == (int)specs.size());
  CHECK(rb.one_kind([](const void*) { return false; }) && !rb.device());
  FakeBuf buf;
  CHECK(rb.place(buf));
  // layout: ascending, disjoint, aligned to the element, the block ends with the last part, no more than 7 bytes lost per part
  size_t end = 0, payload = 0;
  for (int i = 0; i < rb.size(); ++i) {
    const ResultBlock::Part& p = rb.part(i);
    CHECK(ref[i] == i && p.dst == dst[i] && p.bytes == specs[i].elem * specs[i].count);
    CHECK(p.off >= end && p.off - end < RESULT_ALIGN && p.off % specs[i].elem == 0 && p.off % RESULT_ALIGN == 0);
    end = p.off + p.bytes;
    payload += p.bytes;
  }
  CHECK(rb.bytes() == end && buf.cap == end && rb.block() == buf.p);
  CHECK(end < payload + RESULT_ALIGN * specs.size());
  if (failures) printf("  (%s)\n", who);
  // a kernel's view: every part has its slot, a null one too; writing each slot in full stays inside the block (the sanitizer watches)
  unsigned char* block = static_cast<unsigned char*>(buf.p);
  for (size_t b = 0; b < end; ++b) block[b] = 0xEE;
  for (int i = 0; i < rb.size(); ++i) {
    unsigned char* slot = specs[i].elem == 8 ? reinterpret_cast<unsigned char*>(rb.dev(ResultBlock::Ref<int64_t>{i}))
                                             : reinterpret_cast<unsigned char*>(rb.dev(ResultBlock::Ref<int32_t>{i}));
    CHECK(slot == block + rb.part(i).off);
    for (size_t b = 0; b < rb.part(i).bytes; ++b) {
      CHECK(slot[b] == 0xEE);   // nobody else's bytes
      slot[b] = pattern(i, b);
    }
  }
  // the way home: a host copy of the block, split into the arrays asked for - all of each, nothing of a null part
  unsigned char* h_block = static_cast<unsigned char*>(malloc(end + (end == 0)));
  for (size_t b = 0; b < end; ++b) h_block[b] = block[b];
  rb.split(h_block);
  for (size_t i = 0; i < specs.size(); ++i) {
    if (!dst[i]) continue;
    const unsigned char* got = static_cast<const unsigned char*>(dst[i]);
    for (size_t b = 0; b < specs[i].elem * specs[i].count; ++b) CHECK(got[b] == pattern((int)i, b));
  }
  free(h_block);

  // device results: no block, every part is the caller's own pointer - null where the caller passed null
  ResultBlock rd;
  for (size_t i = 0; i < specs.size(); ++i) {
    if (specs[i].elem == 8) add_as<int64_t>(rd, dst[i], specs[i].count);
    else add_as<int32_t>(rd, dst[i], specs[i].count);
  }
  CHECK(rd.one_kind([](const void*) { return true; }) && rd.device());
  FakeBuf none;
  none.fail = true;   // (never asked)
  CHECK(rd.place(none) && none.p == nullptr && rd.block() == nullptr);
  for (int i = 0; i < rd.size(); ++i)
    CHECK((specs[i].elem == 8 ? static_cast<void*>(rd.dev(ResultBlock::Ref<int64_t>{i})) : static_cast<void*>(rd.dev(ResultBlock::Ref<int32_t>{i}))) == dst[i]);
  for (void* p : dst) free(p);
}

static void layouts() {
  const size_t nqs[] = {1, 2, 3, 5, 8}, ks[] = {1, 3, 7, 10}, ms[] = {1, 3, 4}, caps[] = {1, 9, 64}, limits[] = {0, 1, 11};
  for (int optional = 0; optional < 2; ++optional) {
    const bool opt = optional != 0;
    for (size_t nq : nqs) {
      for (size_t k : ks) {
        // search, search_among: [ids i64 | dist f32 | counts i32?]
        check_call("search", {{8, nq * k, true}, {4, nq * k, true}, {4, nq, opt}});
        // search_groups: [ids | group keys | dist | counts?]
        check_call("search_groups", {{8, nq * k, true}, {8, nq * k, true}, {4, nq * k, true}, {4, nq, opt}});
        // search_group_rows: [ids | group keys | group sizes? | dist | row counts | counts?]
        for (size_t m : ms)
          check_call("search_group_rows", {{8, nq * k * m, true}, {8, nq * k, true}, {8, nq * k, opt}, {4, nq * k * m, true}, {4, nq * k, true}, {4, nq, opt}});
      }
      // search_range: [ids | totals? | dist | counts?]
      for (size_t cap : caps) check_call("search_range", {{8, nq * cap, true}, {8, nq, opt}, {4, nq * cap, true}, {4, nq, opt}});
    }
    // select: [count | total? | ids] - the head the call reads first is the block's first 16 bytes; no ids asked for where none can be written
    for (size_t limit : limits) check_call("select", {{8, 1, true}, {8, 1, opt}, {8, limit, limit > 0}});
  }
  // a 4-byte part of odd length ahead of an 8-byte one - the order no call uses today: the rule holds wherever a part stands
  check_call("4 before 8", {{4, 35, true}, {8, 5, true}, {4, 1, false}, {8, 3, true}});
  ResultBlock rb;
  rb.add(static_cast<int32_t*>(nullptr), 35);
  rb.add(static_cast<int64_t*>(nullptr), 5);
  CHECK(rb.part(1).off == 144 && rb.bytes() == 184);
}

static void kinds() {
  int64_t a[2];
  float b[2];
  int32_t c[2];
  const void* device_side = b;
  auto is_dev = [&](const void* p) { return p == device_side; };
  ResultBlock mixed;
  mixed.add(a, 2);
  mixed.add(b, 2);
  mixed.add(c, 2);
  CHECK(!mixed.one_kind(is_dev));
  ResultBlock with_null;   // a null part has no say
  with_null.add(b, 2);
  with_null.add(static_cast<int32_t*>(nullptr), 2);
  CHECK(with_null.one_kind(is_dev) && with_null.device());
  ResultBlock host;
  host.add(a, 2);
  host.add(static_cast<int64_t*>(nullptr), 2);
  host.add(c, 2);
  CHECK(host.one_kind(is_dev) && !host.device());
  FakeBuf full;
  full.fail = true;
  CHECK(!host.place(full));   // out of device memory: the call refuses
}

int main() {
  layouts();
  kinds();
  if (failures) {
    printf("result_block_host_check: %d check(s) failed\n", failures);
    return 1;
  }
  printf("result_block_host_check OK\n");
  return 0;
}
