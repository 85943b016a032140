// The result arrays of one serving call (host code only: index_calls.cpp, and tests/native/result_block_host_check.cpp under the sanitizers).
// A call names each of its outputs once, in the order it wants them in the block; everything else follows from that list:
//   device results  every part's device pointer is the caller's own pointer (null where the caller passed null), and there is no block;
//   host results    the parts lie in ONE device block - kernels write there, fetch_to_host brings the block over and splits it.  A null
//                   optional output keeps its slot, so that a kernel may write it; it is not copied out.
// Layout rule: every part starts at a multiple of RESULT_ALIGN = 8 bytes, the largest element a part may have - so each part starts at a multiple
// of its own element size wherever it stands in the list; the block ends where its last part ends.
#pragma once
#include <assert.h>
#include <stddef.h>
#include <string.h>

namespace eps {

constexpr size_t RESULT_ALIGN = 8;

class ResultBlock {
 public:
  static constexpr int MAX_PARTS = 6;
  struct Part {
    void* dst;          // the caller's array (null: not asked for)
    size_t off, bytes;  // where it lies in a host call's block
  };
  template <class T>
  struct Ref {   // what add returns: names the part to dev()
    int i;
  };

  // the next part: `count` elements for the caller's array `dst`
  template <class T>
  Ref<T> add(T* dst, size_t count) {
    static_assert(RESULT_ALIGN % sizeof(T) == 0, "a part's element size must divide RESULT_ALIGN");
    assert(n_ < MAX_PARTS);
    Part& p = part_[n_];
    p.dst = dst;
    p.off = (bytes_ + RESULT_ALIGN - 1) / RESULT_ALIGN * RESULT_ALIGN;
    p.bytes = count * sizeof(T);
    bytes_ = p.off + p.bytes;
    return Ref<T>{n_++};
  }

  // false: the arrays the caller passed are not all host or all device memory (null parts have no say).  Otherwise device() is their kind
  template <class IsDevice>
  bool one_kind(IsDevice is_device) {
    bool first = true;
    for (int i = 0; i < n_; ++i) {
      if (!part_[i].dst) continue;
      const bool d = is_device(part_[i].dst);
      if (!first && d != dev_) return false;
      dev_ = d;
      first = false;
    }
    return true;
  }
  bool device() const { return dev_; }

  // after the last add and one_kind: host results get their block - `buf` (anything with reserve(bytes) and p) grows to hold it; device results
  // need none.  False: out of device memory
  template <class Buf>
  bool place(Buf& buf) {
    if (dev_) return true;
    if (!buf.reserve(bytes_)) return false;
    block_ = static_cast<char*>(buf.p);
    return true;
  }

  // where the kernels write part r (after place)
  template <class T>
  T* dev(Ref<T> r) const {
    return dev_ ? static_cast<T*>(part_[r.i].dst) : reinterpret_cast<T*>(block_ + part_[r.i].off);
  }

  const void* block() const { return block_; }
  size_t bytes() const { return bytes_; }
  int size() const { return n_; }
  const Part& part(int i) const { return part_[i]; }

  // a host copy of the block into the arrays the caller asked for
  void split(const void* h_block) const {
    for (int i = 0; i < n_; ++i)
      if (part_[i].dst) memcpy(part_[i].dst, static_cast<const char*>(h_block) + part_[i].off, part_[i].bytes);
  }

 private:
  Part part_[MAX_PARTS] = {};
  int n_ = 0;
  size_t bytes_ = 0;
  bool dev_ = false;
  char* block_ = nullptr;
};

}  // namespace eps
