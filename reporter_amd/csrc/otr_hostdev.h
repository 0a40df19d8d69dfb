// otr_hostdev.h — the host side every device stage shares (host code only): the HIP error
// check, the two launch-grid helpers, the growable device buffer pool with its one
// out-of-memory exception and message, and the guard that turns that exception into a return
// code at an entry point.  The hipcub scan / sort helpers are in otr_devscan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/otr.h"

// (uses the `std::string* err` of the enclosing function)
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      if (err) *err = std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x;    \
      return OTR_DEVICE_ERROR;                                                           \
    }                                                                                    \
  } while (0)

namespace otr {

// blocks of `block` threads that cover n items: none for n == 0
static inline unsigned grid_ceil(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }
// the same, but at least one block (a launch of zero blocks is an error)
static inline unsigned grid_ceil1(int64_t n, int block) {
  return (unsigned)std::max<int64_t>(1, (n + block - 1) / block);
}

// A device buffer that cannot be allocated ends the call: the pool throws, the entry point
// (guarded) catches after draining the stream and returns OTR_DEVICE_ERROR naming the buffer
// — no kernel ever runs on a missing buffer.  One type for every pool, so a guard catches
// the failure of any of them: store code that calls into the matcher stays behind its guard.
enum class PoolOwner { matcher, sessions, tile_store };
struct DeviceOom {
  PoolOwner owner;
  const char* name;  // the stores' buffers
  int slot;          // the matcher's
  size_t bytes;      // the size of the last attempt
};

// drains the stream, clears the sticky allocation error, names the buffer
inline int oom_error(hipStream_t stream, const DeviceOom& o, std::string* err) {
  if (stream) (void)hipStreamSynchronize(stream);  // nothing of this call still running
  (void)hipGetLastError();
  if (!err) return OTR_DEVICE_ERROR;
  if (o.owner == PoolOwner::matcher) {
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    *err = "out of device memory: buffer " + std::to_string(o.slot) + " needs " + std::to_string(o.bytes >> 20) +
           " MiB (" + std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) + " MiB free): split the batch";
  } else {
    *err = std::string("out of device memory: ") + (o.owner == PoolOwner::sessions ? "session" : "tile store") +
           " buffer '" + o.name + "' needs " + std::to_string((o.bytes >> 20) + 1) + " MiB";
  }
  return OTR_DEVICE_ERROR;
}

// Runs an entry point's body and turns a pool's exception into the return code (no C++
// exception crosses the C ABI).  The stream is read when the exception arrives: the body may
// be what creates it.
template <class F>
int guarded(const hipStream_t& stream, std::string* err, F&& f) {
  try {
    return f();
  } catch (const DeviceOom& o) {
    return oom_error(stream, o, err);
  }
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// Growable device buffers by slot number.  A slot that is too small is freed and allocated
// again a quarter larger than asked, so sizes that creep up do not allocate every call.
struct DevPool {
  PoolOwner owner;
  const char* const* names;  // per slot, or nullptr (the matcher's slots go by number)
  std::vector<DevBuf> b;

  DevPool(PoolOwner o, const char* const* slot_names, size_t n_slots) : owner(o), names(slot_names), b(n_slots) {}

  struct NoRoom {
    bool operator()(int) const { return false; }
  };
  // n elements of T in `slot` (one at least), or DeviceOom.  The stores take the defaults:
  // one attempt.  The matcher's policy: second_exact tries again at the exact size, and
  // make_room(slot), when it could free something, buys one more attempt at that size.
  template <class T, class Room = NoRoom>
  T* get(int slot, size_t n, bool second_exact = false, Room&& make_room = Room()) {
    DevBuf& s = b[slot];
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if (s.bytes >= bytes) return (T*)s.p;
    drop(slot);
    size_t tried = bytes + bytes / 4;
    bool ok = hipMalloc(&s.p, tried) == hipSuccess;
    if (!ok && second_exact) {
      tried = bytes;
      ok = hipMalloc(&s.p, tried) == hipSuccess;
      if (!ok && make_room(slot)) {
        (void)hipGetLastError();  // what could be freed is gone: once more
        ok = hipMalloc(&s.p, tried) == hipSuccess;
      }
    }
    if (!ok) {
      (void)hipGetLastError();  // clear the sticky allocation error
      s.p = nullptr;
      throw DeviceOom{owner, names ? names[slot] : nullptr, slot, tried};
    }
    s.bytes = tried;
    return (T*)s.p;
  }

  // what the slot holds if that is at least `bytes`, else nullptr
  void* held(int slot, size_t bytes) const { return b[slot].bytes >= bytes ? b[slot].p : nullptr; }
  void drop(int slot) {
    if (b[slot].p) (void)hipFree(b[slot].p);
    b[slot] = DevBuf{};
  }
  // an empty slot at exactly `bytes`, or nullptr and no exception (optional workspace)
  void* try_exact(int slot, size_t bytes) {
    DevBuf& s = b[slot];
    if (hipMalloc(&s.p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      s.p = nullptr;
      return nullptr;
    }
    s.bytes = bytes;
    return s.p;
  }
  void release() {
    for (int s = 0; s < (int)b.size(); ++s) drop(s);
  }
};

}  // namespace otr
