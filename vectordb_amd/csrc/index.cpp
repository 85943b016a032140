// Host side of libepsilla_gfx950 — see index.hpp.  Compiled with hipcc (host code only here).
#include "index.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>

namespace eps {

// ------------------------------------------------------------------------------------------------ engine-selection switches
// (eps_set_tuning).  Values are interned and never freed, so a pointer handed out stays valid while another thread replaces the entry.
namespace {
std::mutex g_tune_mu;
std::unordered_map<std::string, const char*> g_tune;
std::unordered_set<std::string> g_tune_values;   // (interned: a value set a million times is stored once; element addresses are stable)
}  // namespace
const char* tune_env(const char* name) {
  {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (!g_tune.empty()) {
      auto it = g_tune.find(name);
      if (it != g_tune.end()) return it->second;
    }
  }
  return nullptr;
}
int tune_int(const char* name, int dflt) {
  const char* e = tune_env(name);
  return e ? atoi(e) : dflt;
}
void tune_set(const char* name, const char* value) {
  std::lock_guard<std::mutex> lk(g_tune_mu);
  if (!name) {
    g_tune.clear();
  } else if (!value) {
    g_tune.erase(name);
  } else {
    g_tune[name] = g_tune_values.emplace(value).first->c_str();
  }
}

// ------------------------------------------------------------------------------------------------ utils
DevBuf::~DevBuf() { release(); }
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
}
Index::HostBuf::~HostBuf() {
  if (p) (void)hipHostFree(p);
}
bool Index::HostBuf::reserve(size_t bytes) {
  if (bytes <= cap) return true;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    p = nullptr;
    return false;
  }
  cap = want;
  return true;
}
namespace {
std::mutex g_scratch_mu;
std::vector<ScratchClaim*> g_scratch;
}  // namespace
ScratchClaim::ScratchClaim() {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  g_scratch.push_back(this);
}
ScratchClaim::~ScratchClaim() {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  g_scratch.erase(std::remove(g_scratch.begin(), g_scratch.end(), this), g_scratch.end());
}
size_t scratch_reclaim() {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  size_t freed = 0;
  for (ScratchClaim* c : g_scratch) {
    if (!c->buf || !c->buf->p) continue;
    if (!c->try_enter()) continue;   // its owner is between "the table is there" and the launch that uses it (possibly this very thread)
    freed += c->buf->cap;
    c->buf->release();
    c->leave();
  }
  return freed;
}
bool DevBuf::reserve(size_t bytes) {
  if (bytes <= cap) return true;
  release();
  for (int attempt = 0; attempt < 2; ++attempt) {
    size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&p, want) == hipSuccess) {
      cap = want;
      return true;
    }
    (void)hipGetLastError();
    p = nullptr;
    if (hipMalloc(&p, bytes) == hipSuccess) {
      cap = bytes;
      return true;
    }
    (void)hipGetLastError();
    p = nullptr;
    if (attempt == 0 && scratch_reclaim() == 0) break;   // nothing to give back: fail; else once more
  }
  return false;
}
hipError_t DevBuf::grow_keeping(size_t want, size_t keep, hipStream_t s) {
  DevBuf bigger;
  if (!bigger.reserve(want)) return hipErrorOutOfMemory;
  hipError_t e = keep ? hipMemcpyAsync(bigger.p, p, keep, hipMemcpyDeviceToDevice, s) : hipSuccess;
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  std::swap(p, bigger.p);   // (bigger's destructor frees the old allocation)
  std::swap(cap, bigger.cap);
  return hipSuccess;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

bool is_page_locked_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {   // (memory the runtime has never seen: pageable)
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

Index::Index(int64_t dim, int metric, int device) : dim_(dim), metric_(metric), device_(device) {}

Index::~Index() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  if (graph_) graph_free(graph_);
  if (mirror_) half_mirror_free(mirror_);
  if (ev0_) (void)hipEventDestroy(ev0_);
  if (ev1_) (void)hipEventDestroy(ev1_);
  for (auto& pr : kring_)
    for (auto& e : pr)
      if (e) (void)hipEventDestroy(e);
  for (auto& pr : stage_ev_)
    for (auto& e : pr)
      if (e) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int32_t Index::hip_fail(hipError_t e, const char* what) {
  (void)hipGetLastError();
  return fail(EPS_INFRA_UNEXPECTED_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

int32_t Index::init() {
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
  for (auto& pr : kring_)
    for (auto& e : pr) HIP_TRY(hipEventCreate(&e));
  evk0_ = kring_[0][0];
  evk1_ = kring_[0][1];
  for (auto& pr : stage_ev_)
    for (auto& e : pr) HIP_TRY(hipEventCreate(&e));
  return EPS_OK;
}

int32_t Index::set_stream(void* s) {
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

int32_t Index::synchronize() {
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  return EPS_OK;
}

int32_t Index::attach_rows(const float* rows, int64_t n) { return attach_rows_strided(rows, n, dim_); }
int32_t Index::append_rows(const float* rows, int64_t n_new) { return append_rows_strided(rows, n_new, dim_); }

int32_t Index::clone_rows(IndexBase& src_base, int64_t n) {
  Index* src = dynamic_cast<Index*>(&src_base);
  if (!src || src == this) return fail(EPS_USER_ERROR, "clone_rows: the source must be another plain index");
  if (src->dim_ != dim_ || src->device_ != device_) return fail(EPS_USER_ERROR, "clone_rows: source and destination differ in dimension or device");
  if (n < 0 || n > src->n_rows_) return fail(EPS_USER_ERROR, "clone_rows: n exceeds the source's rows");
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(src->stream_));   // (the source's rows are complete)
  return attach_rows_strided(src->d_rows_, n, dim_, true);
}

int32_t Index::attach_rows_strided(const float* rows, int64_t n, int64_t pitch, bool copy_device_rows) {
  if (n < 0 || (n > 0 && !rows) || pitch < dim_) return fail(EPS_USER_ERROR, "attach_rows: bad arguments");
  if (n >= (int64_t)1 << 31) return fail(EPS_DB_UNSUPPORTED_ERROR, "attach_rows: more than 2^31-1 rows per index (shard first)");
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  if (is_device_ptr(rows) && pitch == dim_ && !copy_device_rows) {
    rows_buf_.release();
    d_rows_ = rows;
    rows_owned_ = false;
  } else {
    const size_t bytes = (size_t)n * dim_ * sizeof(float);
    if (!rows_buf_.reserve(bytes ? bytes : 16)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "attach_rows: out of device memory");
    if (bytes && pitch == dim_) HIP_TRY(hipMemcpyAsync(rows_buf_.p, rows, bytes, hipMemcpyDefault, stream_));
    else if (bytes) HIP_TRY(hipMemcpy2DAsync(rows_buf_.p, (size_t)dim_ * 4, rows, (size_t)pitch * 4, (size_t)dim_ * 4, (size_t)n, hipMemcpyDefault, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    d_rows_ = rows_buf_.as<float>();
    rows_owned_ = true;
  }
  n_rows_ = n;
  ++rows_version_;
  prog_rows_host_ = nullptr;   // a new table: attribute rows cached from the previous one are not its rows, whatever their address
  prog_rows_uploaded_ = 0;
  loaded_attr_rows_ = 0;       // ... nor are the rows a previous eps_index_load_table kept (load_table sets them again after attaching)
  // state that was sized for the previous table does not carry over: a graph over more rows than are attached now, a
  // deleted bitset or an attribute column of the old length
  if (n_indexed_ > n) {
    n_indexed_ = 0;
    nav_ = 0;
    h_off_.assign(1, 0);
    h_nbr_.clear();
    (void)graph_upload(*this);
  }
  if (deleted_bytes_ < (n + 7) / 8) {
    d_deleted_ = nullptr;
    deleted_bytes_ = 0;
  }
  if (fcol_rows_ < n) {
    f_op_ = 0;
    d_fcol_ = nullptr;
    fcol_rows_ = 0;
  }
  return EPS_OK;
}

int32_t Index::append_rows_strided(const float* rows, int64_t n_new, int64_t pitch) {
  if (n_new < 0 || (n_new > 0 && !rows) || pitch < dim_) return fail(EPS_USER_ERROR, "append_rows: bad arguments");
  if (n_new == 0) return EPS_OK;
  if (n_rows_ > 0 && !rows_owned_) return fail(EPS_USER_ERROR, "append_rows: the row store is borrowed device memory; re-attach instead");
  HIP_TRY(hipSetDevice(device_));
  HIP_TRY(hipStreamSynchronize(stream_));
  const size_t old_bytes = (size_t)n_rows_ * dim_ * sizeof(float);
  const size_t add_bytes = (size_t)n_new * dim_ * sizeof(float);
  if (old_bytes + add_bytes > rows_buf_.cap) {
    const hipError_t e = rows_buf_.grow_keeping((old_bytes + add_bytes) * 3 / 2, old_bytes, stream_);
    if (e == hipErrorOutOfMemory) return fail(EPS_INFRA_UNEXPECTED_ERROR, "append_rows: out of device memory");
    if (e != hipSuccess) return hip_fail(e, "append_rows: moving the rows");
  }
  if (pitch == dim_) HIP_TRY(hipMemcpyAsync(static_cast<char*>(rows_buf_.p) + old_bytes, rows, add_bytes, hipMemcpyDefault, stream_));
  else HIP_TRY(hipMemcpy2DAsync(static_cast<char*>(rows_buf_.p) + old_bytes, (size_t)dim_ * 4, rows, (size_t)pitch * 4, (size_t)dim_ * 4, (size_t)n_new,
                                hipMemcpyDefault, stream_));
  HIP_TRY(hipStreamSynchronize(stream_));
  d_rows_ = rows_buf_.as<float>();
  rows_owned_ = true;
  n_rows_ += n_new;   // rows_version_ stays: the fp16 mirror is extended by the new rows on the next MFMA search
  return EPS_OK;   // (a bitset / attribute column that is now too short is rejected by search(), see there)
}

// data_mvp.bin -> HBM (layout: db/table_segment_mvp.cpp:939-1010; the reference's own loader is its constructor, :133-295)
int32_t Index::load_table(const char* path, const eps_table_layout* lay, int64_t* n_out) {
  if (!path || !lay || lay->primitive_offset < 0 || lay->var_len_attrs < 0 || lay->dense_fields <= 0 || !lay->dense_dims || lay->field < 0 ||
      lay->field >= lay->dense_fields)
    return fail(EPS_USER_ERROR, "load_table: bad arguments");
  if (lay->dense_dims[lay->field] != dim_) return fail(EPS_USER_ERROR, "load_table: the field's dimension differs from the index's");
  const int fd = ::open(path, O_RDONLY);
  if (fd < 0) return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Cannot open file: ") + path);
  struct stat st;
  if (fstat(fd, &st) != 0 || st.st_size < 32) {
    ::close(fd);
    return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Corrupt table segment file: ") + path);
  }
  const size_t fsize = (size_t)st.st_size;
  void* map = mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
  ::close(fd);
  if (map == MAP_FAILED) return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Cannot map file: ") + path);
  struct Unmap {
    void* p;
    size_t n;
    ~Unmap() { munmap(p, n); }
  } unmap{map, fsize};
  const char* base = static_cast<const char*>(map);
  size_t pos = 0;
  auto need = [&](size_t bytes) { return bytes <= fsize && pos <= fsize - bytes; };
  auto corrupt = [&]() { return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Corrupt table segment file: ") + path); };
  if (!need(24)) return corrupt();
  uint64_t n64;
  int64_t first_id, bitset_size;
  std::memcpy(&n64, base + pos, 8);
  std::memcpy(&first_id, base + pos + 8, 8);
  std::memcpy(&bitset_size, base + pos + 16, 8);
  pos += 24;
  (void)first_id;
  if (n64 >= ((uint64_t)1 << 31) || bitset_size < 0 || !need((size_t)bitset_size)) return corrupt();
  const int64_t n = (int64_t)n64;
  if (bitset_size < (n + 7) / 8) return corrupt();   // the reference writes the whole ConcurrentBitset (capacity bits >= record count)
  const uint8_t* bits = reinterpret_cast<const uint8_t*>(base + pos);
  pos += (size_t)bitset_size;
  if ((uint64_t)lay->primitive_offset > fsize || (n > 0 && (uint64_t)lay->primitive_offset > (uint64_t)fsize / (uint64_t)n)) return corrupt();   // (n * offset cannot wrap)
  const size_t attr_bytes = (size_t)n * (size_t)lay->primitive_offset;
  if (!need(attr_bytes)) return corrupt();
  const char* attrs = base + pos;
  pos += attr_bytes;
  for (int64_t r = 0; r < n; ++r)            // variable-length attributes: int64 length + payload each
    for (int a = 0; a < lay->var_len_attrs; ++a) {
      if (!need(8)) return corrupt();
      int64_t len;
      std::memcpy(&len, base + pos, 8);
      pos += 8;
      if (len < 0 || !need((size_t)len)) return corrupt();
      pos += (size_t)len;
    }
  const float* field_rows = nullptr;
  for (int f = 0; f < lay->dense_fields; ++f) {
    if (lay->dense_dims[f] <= 0) return fail(EPS_USER_ERROR, "load_table: bad dimension");
    const size_t bytes = (size_t)n * (size_t)lay->dense_dims[f] * sizeof(float);
    if (!need(bytes)) return corrupt();
    if (f == lay->field) field_rows = reinterpret_cast<const float*>(base + pos);
    pos += bytes;
  }
  if (!need(8)) return corrupt();            // trailing WAL id
  int32_t rc = attach_rows(field_rows, n);   // the mapped pages go to HBM directly; no host copy of the table is made
  if (rc != EPS_OK) return rc;
  rc = n > 0 ? set_deleted(bits, bitset_size) : set_deleted(nullptr, 0);   // (never a bitset left over from a previous table)
  if (rc != EPS_OK) return rc;
  if (attr_bytes > 0) {   // keep the attribute rows on the device for a later filter program
    HIP_TRY(hipStreamSynchronize(stream_));
    if (!prog_rows_buf_.reserve(attr_bytes)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "load_table: out of device memory (attribute rows)");
    HIP_TRY(hipMemcpyAsync(prog_rows_buf_.p, attrs, attr_bytes, hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    d_prog_rows_ = prog_rows_buf_.as<uint8_t>();
    prog_rows_host_ = nullptr;
    prog_rows_stride_ = lay->primitive_offset;
    prog_rows_uploaded_ = n;
    loaded_attr_rows_ = n;
    loaded_attr_stride_ = lay->primitive_offset;
    prog_len_ = 0;
  }
  if (n_out) *n_out = n;
  return EPS_OK;
}

int32_t Index::set_id_map(int64_t base, int64_t stride) {
  if (stride <= 0) return fail(EPS_USER_ERROR, "set_id_map: stride must be positive");
  id_base_ = base;
  id_stride_ = stride;
  return EPS_OK;
}

int32_t Index::set_deleted(const uint8_t* bits, int64_t nbytes) {
  HIP_TRY(hipSetDevice(device_));
  if (!bits || nbytes <= 0) {
    d_deleted_ = nullptr;
    deleted_bytes_ = 0;
    return EPS_OK;
  }
  if (nbytes < (n_rows_ + 7) / 8) return fail(EPS_USER_ERROR, "set_deleted: bitset shorter than ceil(rows/8) bytes");
  deleted_bytes_ = nbytes;
  if (is_device_ptr(bits)) {
    d_deleted_ = bits;
  } else {
    // the DBMS hands over its bitset on every call; a table without deletions (the common case) is recognised here, which
    // skips the upload and keeps the unfiltered fast paths (MFMA-seeded staging) available
    const int64_t live = (n_rows_ + 7) / 8;
    bool any = false;
    int64_t i = 0;
    for (; i + 8 <= live && !any; i += 8) {
      uint64_t w;
      std::memcpy(&w, bits + i, 8);
      any = w != 0;
    }
    for (; i < live && !any; ++i) any = bits[i] != 0;
    if (!any && n_rows_ > 0) {   // (before any rows are attached nothing can be concluded from the live prefix)
      d_deleted_ = nullptr;
      return EPS_OK;
    }
    if (!deleted_buf_.reserve((size_t)nbytes)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "set_deleted: out of device memory");
    HIP_TRY(hipMemcpyAsync(deleted_buf_.p, bits, (size_t)nbytes, hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));  // the host bitset may change right after we return
    d_deleted_ = deleted_buf_.as<uint8_t>();
  }
  return EPS_OK;
}

int32_t Index::set_int_filter(const void* column, int64_t stride, int32_t width, int32_t op, int64_t constant) {
  HIP_TRY(hipSetDevice(device_));
  if (op == EPS_OP_NONE || !column) {
    f_op_ = 0;
    d_fcol_ = nullptr;
    fcol_rows_ = 0;
    return EPS_OK;
  }
  if (op < 0 || op > EPS_OP_NE) return fail(EPS_USER_ERROR, "set_int_filter: unknown operator");
  if (width != 1 && width != 2 && width != 4 && width != 8) return fail(EPS_USER_ERROR, "set_int_filter: width must be 1, 2, 4 or 8 bytes");
  if (stride < width) return fail(EPS_USER_ERROR, "set_int_filter: stride smaller than the value width");
  if (is_device_ptr(column)) {
    d_fcol_ = static_cast<const uint8_t*>(column);
  } else {
    const size_t bytes = (size_t)(n_rows_ > 0 ? (n_rows_ - 1) * stride + width : 0);
    if (!fcol_buf_.reserve(bytes ? bytes : 16)) return fail(EPS_INFRA_UNEXPECTED_ERROR, "set_int_filter: out of device memory");
    if (bytes) HIP_TRY(hipMemcpyAsync(fcol_buf_.p, column, bytes, hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    d_fcol_ = fcol_buf_.as<uint8_t>();
  }
  f_stride_ = stride;
  f_width_ = width;
  f_op_ = op;
  f_value_ = constant;
  fcol_rows_ = n_rows_;
  return EPS_OK;
}

int32_t Index::set_filter_program(const eps_filter_op* ops, int32_t nops, const void* rows, int64_t stride, int64_t n_rows, int32_t flags) {
  return set_filter_program_pitched(ops, nops, rows, stride, stride, n_rows, flags);
}

// rows: row i at rows + i * src_pitch, row_bytes (<= src_pitch) of it are the attribute row.  A hash-sharded table hands every
// shard the same memory with src_pitch = shards * row_bytes: only the shard's own rows are uploaded, packed at row_bytes.
int32_t Index::set_filter_program_pitched(const eps_filter_op* ops, int32_t nops, const void* rows, int64_t src_pitch, int64_t row_bytes, int64_t n_rows,
                                          int32_t flags) {
  HIP_TRY(hipSetDevice(device_));
  if (nops <= 0 || !ops) {
    prog_len_ = 0;
    d_prog_rows_ = nullptr;
    prog_uses_dist_ = false;
    return EPS_OK;
  }
  if (nops > 64) return fail(EPS_DB_UNSUPPORTED_ERROR, "set_filter_program: more than 64 instructions");
  const bool use_loaded = !rows && loaded_attr_rows_ > 0 && loaded_attr_rows_ >= n_rows_;   // the rows eps_index_load_table kept
  int64_t stride = row_bytes;   // of the device copy
  if (use_loaded) {
    stride = loaded_attr_stride_;
    n_rows = loaded_attr_rows_;
  }
  if ((!rows && !use_loaded) || stride <= 0 || n_rows < n_rows_ || (!use_loaded && src_pitch < row_bytes))
    return fail(EPS_USER_ERROR, "set_filter_program: attribute rows missing or shorter than the table");
  // validate: known opcodes, attribute loads inside a row, stack discipline
  int sp = 0, maxsp = 0;
  bool uses_dist = false;
  for (int i = 0; i < nops; ++i) {
    const int op = ops[i].op;
    if (op < EPS_FOP_PUSH_CONST || op > EPS_FOP_NE_BOOL) return fail(EPS_USER_ERROR, "set_filter_program: unknown opcode");
    if (op <= EPS_FOP_PUSH_BOOL) {
      static const int width[] = {0, 0, 0, 1, 2, 4, 8, 4, 8, 1};
      if (op >= EPS_FOP_PUSH_I8 && (ops[i].arg < 0 || (int64_t)ops[i].arg + width[op] > stride))   // (in 64 bits: arg = INT32_MAX must not wrap)
        return fail(EPS_USER_ERROR, "set_filter_program: attribute offset outside the row");
      uses_dist |= op == EPS_FOP_PUSH_DIST;
      ++sp;
    } else if (op == EPS_FOP_NOT) {
      if (sp < 1) return fail(EPS_USER_ERROR, "set_filter_program: stack underflow");
    } else {
      if (sp < 2) return fail(EPS_USER_ERROR, "set_filter_program: stack underflow");
      --sp;
    }
    maxsp = std::max(maxsp, sp);
  }
  if (sp != 1 || maxsp > 16) return fail(EPS_USER_ERROR, "set_filter_program: the program must leave exactly one value (stack depth <= 16)");
  HIP_TRY(hipStreamSynchronize(stream_));
  if (!prog_buf_.reserve((size_t)nops * sizeof(FilterOp))) return fail(EPS_INFRA_UNEXPECTED_ERROR, "set_filter_program: out of device memory");
  static_assert(sizeof(FilterOp) == sizeof(eps_filter_op), "FilterOp mirrors eps_filter_op");
  HIP_TRY(hipMemcpyAsync(prog_buf_.p, ops, (size_t)nops * sizeof(FilterOp), hipMemcpyHostToDevice, stream_));
  if (use_loaded) {
    d_prog_rows_ = prog_rows_buf_.as<uint8_t>();
  } else if (is_device_ptr(rows)) {
    d_prog_rows_ = static_cast<const uint8_t*>(rows);
    stride = src_pitch;   // used in place
    prog_rows_host_ = nullptr;
    loaded_attr_rows_ = 0;
  } else {
    loaded_attr_rows_ = 0;
    // Default: the whole table is uploaded (the caller may have edited it in place, or another table may live at the same address).
    // EPS_FILTER_ROWS_APPEND_ONLY is the caller's promise that rows handed over earlier FROM THIS POINTER are unchanged - true for
    // the reference's attribute table, where an update is delete + insert (table_segment_mvp.cpp:476-587) - then only the new
    // tail crosses PCIe.
    const size_t bytes = (size_t)n_rows * (size_t)stride;
    const bool same = (flags & EPS_FILTER_ROWS_APPEND_ONLY) && prog_rows_host_ == rows && prog_rows_stride_ == stride && prog_rows_pitch_ == src_pitch &&
                      prog_rows_uploaded_ <= n_rows && prog_rows_buf_.p;
    const int64_t have_rows = same ? prog_rows_uploaded_ : 0;
    const size_t have = (size_t)have_rows * (size_t)stride;
    if (bytes > prog_rows_buf_.cap) {
      const hipError_t e = prog_rows_buf_.grow_keeping(bytes + bytes / 2 + 16, have, stream_);
      if (e == hipErrorOutOfMemory) return fail(EPS_INFRA_UNEXPECTED_ERROR, "set_filter_program: out of device memory");
      if (e != hipSuccess) return hip_fail(e, "set_filter_program: moving the attribute rows");
    }
    if (n_rows > have_rows) {
      const char* src = static_cast<const char*>(rows) + (size_t)have_rows * (size_t)src_pitch;
      char* dst = static_cast<char*>(prog_rows_buf_.p) + have;
      if (src_pitch == stride) HIP_TRY(hipMemcpyAsync(dst, src, bytes - have, hipMemcpyHostToDevice, stream_));
      else HIP_TRY(hipMemcpy2DAsync(dst, (size_t)stride, src, (size_t)src_pitch, (size_t)stride, (size_t)(n_rows - have_rows), hipMemcpyHostToDevice, stream_));
    }
    d_prog_rows_ = prog_rows_buf_.as<uint8_t>();
    prog_rows_host_ = rows;
    prog_rows_stride_ = stride;
    prog_rows_pitch_ = src_pitch;
    prog_rows_uploaded_ = n_rows;
  }
  HIP_TRY(hipStreamSynchronize(stream_));
  prog_stride_ = stride;
  prog_rows_n_ = n_rows;
  prog_len_ = nops;
  prog_uses_dist_ = uses_dist;
  f_op_ = 0;   // replaces the single-comparison filter
  d_fcol_ = nullptr;
  fcol_rows_ = 0;
  return EPS_OK;
}

FilterSpec Index::filter_spec() const {
  FilterSpec f = no_filter();
  f.deleted = d_deleted_;
  f.column = f_op_ ? d_fcol_ : nullptr;
  f.stride = f_stride_;
  f.width = f_width_;
  f.op = f_op_;
  f.value = f_value_;
  if (prog_len_ > 0 && d_prog_rows_) {
    f.prog = prog_buf_.as<FilterOp>();
    f.prog_rows = d_prog_rows_;
    f.prog_stride = prog_stride_;
    f.prog_len = prog_len_;
    f.prog_use_dist = prefilter_call_ ? 0 : 1;   // PreFilterBruteForceSearch evaluates the filter without a distance (:795)
  }
  return f;
}

// ------------------------------------------------------------------------------------------------ graph
int32_t Index::set_graph(int64_t n, const int64_t* off, const int64_t* nbr, int64_t nav) {
  if (n < 0 || (n > 0 && (!off || (!nbr && off[n] > 0)))) return fail(EPS_USER_ERROR, "set_graph: bad arguments");
  if (n > n_rows_) return fail(EPS_USER_ERROR, "set_graph: graph has more nodes than attached rows");
  if (n > 0 && (nav < 0 || nav >= n)) return fail(EPS_USER_ERROR, "set_graph: navigation point out of range");
  if (n > 0) {
    if (off[0] != 0) return fail(EPS_USER_ERROR, "set_graph: offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
      if (off[i + 1] < off[i]) return fail(EPS_USER_ERROR, "set_graph: offsets must be non-decreasing");
    const int64_t e = off[n];
    for (int64_t i = 0; i < e; ++i)
      if (nbr[i] < 0 || nbr[i] >= n) return fail(EPS_USER_ERROR, "set_graph: neighbor id out of range");
    h_off_.assign(off, off + n + 1);
    h_nbr_.assign(nbr, nbr + e);
  } else {
    h_off_.assign(1, 0);
    h_nbr_.clear();
  }
  n_indexed_ = n;
  nav_ = nav;
  return graph_upload(*this);
}

int32_t Index::graph_info(int64_t* n, int64_t* edges, int64_t* nav) const {
  if (n) *n = n_indexed_;
  if (edges) *edges = n_indexed_ > 0 ? h_off_[n_indexed_] : 0;
  if (nav) *nav = nav_;
  return EPS_OK;
}

int32_t Index::get_graph(int64_t* off, int64_t* nbr) const {
  if (!off || !nbr) return EPS_USER_ERROR;
  if (h_off_.empty()) {
    off[0] = 0;
    return EPS_OK;
  }
  std::memcpy(off, h_off_.data(), sizeof(int64_t) * h_off_.size());
  if (!h_nbr_.empty()) std::memcpy(nbr, h_nbr_.data(), sizeof(int64_t) * h_nbr_.size());
  return EPS_OK;
}

// ann_graph_<field>.bin, byte-compatible with ANNGraphSegment::SaveANNGraph (db/ann_graph_segment.cpp:156-199):
// i64 n, i64 first_record_id, i64 offsets[n+1], i64 neighbors[E], i64 navigation_point; tmp + fsync + rename.
int32_t Index::save_graph(const char* path) {
  if (!path) return fail(EPS_USER_ERROR, "save_graph: null path");
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Cannot open file: ") + path);
  const int64_t n = n_indexed_, first = 0;
  std::vector<int64_t> zero(1, 0);
  const int64_t* off = h_off_.empty() ? zero.data() : h_off_.data();
  const int64_t e = off[n];
  bool ok = std::fwrite(&n, 8, 1, f) == 1 && std::fwrite(&first, 8, 1, f) == 1 &&
            std::fwrite(off, 8, (size_t)n + 1, f) == (size_t)n + 1 &&
            (e == 0 || std::fwrite(h_nbr_.data(), 8, (size_t)e, f) == (size_t)e) && std::fwrite(&nav_, 8, 1, f) == 1;
  std::fflush(f);
  fsync(fileno(f));
  std::fclose(f);
  if (!ok) return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Failed to write to file: ") + path);
  if (std::rename(tmp.c_str(), path) != 0)
    return fail(EPS_INFRA_UNEXPECTED_ERROR, "Failed to rename temp file: " + tmp + " to " + path);
  return EPS_OK;
}

int32_t Index::load_graph(const char* path) {
  if (!path) return fail(EPS_USER_ERROR, "load_graph: null path");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Cannot open file: ") + path);
  int64_t hdr[2];
  std::vector<int64_t> off, nbr;
  int64_t nav = 0;
  std::fseek(f, 0, SEEK_END);
  const int64_t fsize = (int64_t)std::ftell(f);   // header values are untrusted: bound them by the file size
  std::fseek(f, 0, SEEK_SET);
  bool ok = std::fread(hdr, 8, 2, f) == 2 && hdr[0] >= 0 && hdr[0] <= (fsize - 32) / 8;
  if (ok) {
    off.resize((size_t)hdr[0] + 1);
    ok = std::fread(off.data(), 8, off.size(), f) == off.size() && off[hdr[0]] >= 0 && off[hdr[0]] <= (fsize - 24 - 8 * (hdr[0] + 1)) / 8;
  }
  if (ok) {
    nbr.resize((size_t)off[hdr[0]]);
    ok = (nbr.empty() || std::fread(nbr.data(), 8, nbr.size(), f) == nbr.size()) && std::fread(&nav, 8, 1, f) == 1;
  }
  std::fclose(f);
  if (!ok) return fail(EPS_DB_UNEXPECTED_ERROR, std::string("Corrupt ANN graph file: ") + path);
  return set_graph(hdr[0], off.data(), nbr.data(), nav);
}

int32_t Index::build(int64_t n, const eps_build_params* p) {
  if (n < 0 || n > n_rows_) return fail(EPS_USER_ERROR, "build: n exceeds the attached rows");
  HIP_TRY(hipSetDevice(device_));
  return graph_build(*this, n, build_params_or_default(p));
}

}  // namespace eps
