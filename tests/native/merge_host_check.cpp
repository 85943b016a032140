// Stand-alone host check of csrc/merge_host.hpp - the argument checks, the packed layout of eps_range_pack_bytes and the staging of host buffers
// behind eps_merge_range / eps_merge_select - for a CPU build under -fsanitize=address,undefined (tests/test_merge_ref_cpu.py builds and runs it).
// The "device" is the host's heap, every staged block exactly as large as the library asks for, so a wrong offset or length is a heap overflow the
// sanitizer reports; the kernel launch is replaced by a serial merge that reads the lists through the same MergeRankArgs the kernel gets.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../vectordb_amd/csrc/merge_host.hpp"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                             \
    }                                                         \
  } while (0)

struct Key {
  uint32_t ord;
  int64_t id;
  bool operator<(const Key& o) const { return ord < o.ord || (ord == o.ord && id < o.id); }
};
static uint32_t ordinal(float f) {   // make_key's high word
  f += 0.0f;
  if (f != f) return 0xFFC00000u;
  uint32_t u;
  memcpy(&u, &f, 4);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
static float ord2f(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct CpuDev {
  int launches = 0;
  std::vector<void*> live;
  bool is_device(const void* p) { return std::find(live.begin(), live.end(), p) != live.end(); }
  void* alloc(size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    live.push_back(p);
    return p;
  }
  void free(void* p) {
    live.erase(std::find(live.begin(), live.end(), p));
    ::free(p);
  }
  bool h2d(void* dst, const void* src, size_t bytes) { return memcpy(dst, src, bytes), true; }
  bool d2h(void* dst, const void* src, size_t bytes) { return memcpy(dst, src, bytes), true; }
  bool sync() { return true; }
  void launch(const eps::MergeRankArgs& a) {   // the kernel's contract, serially
    ++launches;
    const bool dist = a.dist != nullptr;
    for (int64_t j = 0; j < a.nq; ++j) {
      std::vector<Key> all;
      int64_t total = 0;
      for (int s = 0; s < a.shards; ++s) {
        const char* cp = a.counts + s * a.counts_stride;
        int64_t len = dist ? (int64_t) reinterpret_cast<const int32_t*>(cp)[j] : reinterpret_cast<const int64_t*>(cp)[j];
        len = std::min(std::max<int64_t>(len, 0), a.L);
        total += reinterpret_cast<const int64_t*>(a.totals + s * a.totals_stride)[j];
        for (int64_t p = 0; p < len; ++p) {
          Key k;
          k.id = reinterpret_cast<const int64_t*>(a.ids + s * a.ids_stride)[j * a.L + p];
          k.ord = dist ? ordinal(reinterpret_cast<const float*>(a.dist + s * a.dist_stride)[j * a.L + p]) : 0u;
          all.push_back(k);
        }
      }
      std::stable_sort(all.begin(), all.end());
      const int64_t count = std::min(std::max<int64_t>((int64_t)all.size() - a.skip, 0), a.cap);
      for (int64_t e = 0; e < a.cap; ++e) {
        a.out_ids[j * a.cap + e] = e < count ? all[a.skip + e].id : -1;
        if (dist) a.out_dist[j * a.cap + e] = e < count ? ord2f(all[a.skip + e].ord) : INFINITY;
      }
      if (a.out_counts) {
        if (dist) static_cast<int32_t*>(a.out_counts)[j] = (int32_t)count;
        else static_cast<int64_t*>(a.out_counts)[j] = count;
      }
      if (a.out_totals) a.out_totals[j] = total;
    }
  }
};

static void layout() {
  for (int64_t nq : {0, 1, 3, 70})
    for (int64_t cap : {1, 2, 5, 8192}) {
      const eps::RangePack p = eps::range_pack(nq, cap);
      CHECK(p.totals_off == nq * cap * 8 && p.dist_off == p.totals_off + nq * 8 && p.counts_off == p.dist_off + nq * cap * 4);
      CHECK(p.bytes % 8 == 0 && p.bytes >= p.counts_off + nq * 4 && p.bytes < p.counts_off + nq * 4 + 8);
    }
  CHECK(eps::range_pack(3, 5).bytes == 216);
}

static void checks() {
  const char* why;
  CHECK(eps::merge_range_check(16, 0, 8192, &why) == EPS_OK);
  CHECK(eps::merge_range_check(17, 1, 8, &why) == EPS_USER_ERROR && strstr(why, "shards"));
  CHECK(eps::merge_range_check(0, 1, 8, &why) == EPS_USER_ERROR && strstr(why, "shards"));
  CHECK(eps::merge_range_check(2, 1, 8193, &why) == EPS_USER_ERROR && strstr(why, "cap"));
  CHECK(eps::merge_range_check(2, 1, 0, &why) == EPS_USER_ERROR && strstr(why, "cap"));
  CHECK(eps::merge_range_check(2, -1, 8, &why) == EPS_USER_ERROR && strstr(why, "nq"));
  CHECK(eps::merge_range_check(2, INT64_MAX / 2, 8192, &why) == EPS_USER_ERROR && strstr(why, "nq"));
  CHECK(eps::merge_select_check(true, 3, 10, 4, 6, &why) == EPS_OK);
  CHECK(eps::merge_select_check(true, 3, 0, 0, 0, &why) == EPS_OK);
  CHECK(eps::merge_select_check(true, 3, 10, 5, 6, &why) == EPS_USER_ERROR && strstr(why, "len < skip + limit"));
  CHECK(eps::merge_select_check(true, 3, 10, INT64_MAX, INT64_MAX, &why) == EPS_USER_ERROR && strstr(why, "len < skip + limit"));
  CHECK(eps::merge_select_check(true, 3, -1, 0, 0, &why) == EPS_USER_ERROR && strstr(why, "negative"));
  CHECK(eps::merge_select_check(true, 3, 10, -1, 1, &why) == EPS_USER_ERROR && strstr(why, "negative"));
  CHECK(eps::merge_select_check(true, 3, 10, 1, -1, &why) == EPS_USER_ERROR && strstr(why, "negative"));
  CHECK(eps::merge_select_check(true, 17, 10, 0, 1, &why) == EPS_USER_ERROR && strstr(why, "shards"));
  CpuDev dev;
  void* d = dev.alloc(8);
  int h = 0;
  const void* host[] = {&h, nullptr, &h}, *devs[] = {d, nullptr, d}, *mixed[] = {&h, d}, *none[] = {nullptr};
  CHECK(eps::merge_side(dev, host, 3) == 0 && eps::merge_side(dev, devs, 3) == 1 && eps::merge_side(dev, mixed, 2) == -1 && eps::merge_side(dev, none, 1) == -1);
  dev.free(d);
}

// host arrays of EXACTLY the documented sizes (heap: the sanitizer guards their ends)
static void range_staging(int shards, int64_t nq, int cap, bool with_counts, bool with_totals) {
  const size_t nk = (size_t)nq * cap;
  std::vector<int64_t> ids(shards * nk), totals((size_t)shards * nq), out_ids(nk, -7), out_totals(nq, -7);
  std::vector<float> dist(shards * nk), out_dist(nk, -7.f);
  std::vector<int32_t> counts((size_t)shards * nq), out_counts(nq, -7);
  srand(shards * 1000 + cap);
  for (int s = 0; s < shards; ++s)
    for (int64_t j = 0; j < nq; ++j) {
      const int len = rand() % (cap + 1);
      counts[s * nq + j] = len;
      totals[s * nq + j] = len + (len == cap ? rand() % 5 : 0);
      std::vector<Key> l(len);
      for (auto& k : l) k = Key{(uint32_t)(rand() % 4), (int64_t)(rand() % 6) * ((int64_t)1 << 33)};
      std::sort(l.begin(), l.end());
      for (int p = 0; p < cap; ++p) {
        ids[(s * nq + j) * cap + p] = p < len ? l[p].id : -1;
        dist[(s * nq + j) * cap + p] = p < len ? (float)l[p].ord * 0.5f : INFINITY;
      }
    }
  CpuDev dev;
  CHECK(eps::merge_range_host(dev, ids.data(), dist.data(), counts.data(), totals.data(), shards, nq, cap, out_ids.data(), out_dist.data(),
                              with_counts ? out_counts.data() : nullptr, with_totals ? out_totals.data() : nullptr) == EPS_OK);
  CHECK(dev.launches == 1 && dev.live.empty());
  for (int64_t j = 0; j < nq; ++j) {
    int64_t sum = 0, total = 0;
    for (int s = 0; s < shards; ++s) sum += counts[s * nq + j], total += totals[s * nq + j];
    const int64_t count = std::min<int64_t>(sum, cap);
    CHECK(!with_counts || out_counts[j] == count);
    CHECK(with_counts || out_counts[j] == -7);
    CHECK(with_totals ? out_totals[j] == total : out_totals[j] == -7);
    for (int64_t e = 0; e < cap; ++e) {
      const float dd = out_dist[j * cap + e];
      CHECK(e < count ? (out_ids[j * cap + e] >= 0 && dd >= 0.f && dd <= 1.5f) : (out_ids[j * cap + e] == -1 && isinf(dd)));
      if (e > 0 && e < count) CHECK(dd > out_dist[j * cap + e - 1] || (dd == out_dist[j * cap + e - 1] && out_ids[j * cap + e] >= out_ids[j * cap + e - 1]));
    }
  }
}

static void select_staging(int shards, int64_t len, int64_t skip, int64_t limit, bool with_total) {
  std::vector<int64_t> ids((size_t)shards * len), counts(shards), totals(shards), out(limit, -7), all;
  for (int s = 0; s < shards; ++s) {
    counts[s] = len ? (s * 7 + 3) % (len + 1) : 0;
    totals[s] = counts[s] + (counts[s] == len ? s : 0);
    for (int64_t p = 0; p < len; ++p) ids[s * len + p] = p < counts[s] ? p * shards + s : -1;
    for (int64_t p = 0; p < counts[s]; ++p) all.push_back(p * shards + s);
  }
  std::sort(all.begin(), all.end());
  int64_t count = -7, total = -7;
  CpuDev dev;
  CHECK(eps::merge_select_host(dev, ids.data(), counts.data(), totals.data(), shards, len, skip, limit, out.data(), &count, with_total ? &total : nullptr) == EPS_OK);
  CHECK(dev.launches == 1 && dev.live.empty());
  CHECK(count == std::min(std::max<int64_t>((int64_t)all.size() - skip, 0), limit));
  int64_t want_total = 0;
  for (int s = 0; s < shards; ++s) want_total += totals[s];
  CHECK(with_total ? total == want_total : total == -7);
  for (int64_t e = 0; e < limit; ++e) CHECK(out[e] == (e < count ? all[skip + e] : -1));
}

int main() {
  layout();
  checks();
  for (int shards : {1, 2, 3, 16})
    for (int cap : {1, 2, 5, 33}) {
      range_staging(shards, 1, cap, true, true);
      range_staging(shards, 7, cap, false, true);   // (nq odd: the counts part of a pack ends off a multiple of 8)
      range_staging(shards, 7, cap, true, false);
    }
  for (int shards : {1, 3, 16}) {
    select_staging(shards, 0, 0, 0, true);
    select_staging(shards, 9, 0, 9, true);
    select_staging(shards, 9, 4, 5, false);
    select_staging(shards, 9, 9, 0, true);
    select_staging(shards, 40, 30, 10, true);
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("merge_host_check OK\n");
  return 0;
}
