// One growable buffer with one owner: device memory (or, with pinned = true, page-locked host memory) that is grown on
// demand, reported to a byte counter and freed by its destructor.  Host-only.  Everything the plan allocates goes through it.
//
// The four primitives -- allocate, free, drain the stream, copy between host and device (for gpa_hoststage.h) -- are the
// inline functions below.  With GPA_DEVBUF_HOST_SEAM defined they are malloc / free / nothing / memcpy and count their calls,
// and the n-th allocation can be made to fail: that is how tests/host/devbuf_check.cpp and hoststage_check.cpp check the types
// without a GPU.
#pragma once
#include <stddef.h>

#ifdef GPA_DEVBUF_HOST_SEAM
#include <stdlib.h>
#include <string.h>
typedef int hipError_t;
typedef void* hipStream_t;
constexpr hipError_t hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2;
namespace gpa {
struct DevBufSeam { long allocs = 0, frees = 0, syncs = 0, fail_at = 0, copies = 0; };   // fail_at = n > 0: the n-th allocation from now fails
inline DevBufSeam g_devbuf_seam;
inline hipError_t devbuf_alloc(void** p, size_t bytes, bool) {
  if (g_devbuf_seam.fail_at > 0 && --g_devbuf_seam.fail_at == 0) return hipErrorOutOfMemory;
  *p = malloc(bytes);
  if (!*p) return hipErrorOutOfMemory;
  ++g_devbuf_seam.allocs;
  return hipSuccess;
}
inline void devbuf_free(void* p, bool) { free(p); ++g_devbuf_seam.frees; }
inline hipError_t devbuf_sync(hipStream_t) { ++g_devbuf_seam.syncs; return hipSuccess; }
inline hipError_t devbuf_copy(void* dst, const void* src, size_t bytes, bool, hipStream_t) {
  memcpy(dst, src, bytes);
  ++g_devbuf_seam.copies;
  return hipSuccess;
}
}  // namespace gpa
#else
#include <hip/hip_runtime.h>
namespace gpa {
inline hipError_t devbuf_alloc(void** p, size_t bytes, bool pinned) { return pinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes); }
inline void devbuf_free(void* p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
inline hipError_t devbuf_sync(hipStream_t s) { return hipStreamSynchronize(s); }
// enqueued on s; the host side must stay as it is until s has drained
inline hipError_t devbuf_copy(void* dst, const void* src, size_t bytes, bool to_device, hipStream_t s) {
  return hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, s);
}
}  // namespace gpa
#endif

namespace gpa {

struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;              // bytes behind ptr
  size_t* counted = nullptr;   // where the owner accounts the bytes (gpa_plan::ws_bytes); null: a temporary nobody counts
  bool pinned = false;         // page-locked host memory instead of device memory

  DevBuf() = default;
  explicit DevBuf(size_t* counter, bool pinned_ = false) : counted(counter), pinned(pinned_) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap), counted(o.counted), pinned(o.pinned) { o.ptr = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      ptr = o.ptr; cap = o.cap; counted = o.counted; pinned = o.pinned;
      o.ptr = nullptr; o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  template <class T> T* as() const { return static_cast<T*>(ptr); }

  // at least `bytes` (0 asks for 16).  Grow-only: nothing happens while the capacity suffices.  Growing a live buffer drains
  // `stream` first (work enqueued there may still use the old one) and frees it.  A failed allocation leaves the buffer empty.
  hipError_t reserve(size_t bytes, hipStream_t stream) {
    if (bytes == 0) bytes = 16;
    if (ptr && cap >= bytes) return hipSuccess;
    if (ptr) {
      const hipError_t e = devbuf_sync(stream);
      if (e != hipSuccess) return e;
      release();
    }
    const hipError_t e = devbuf_alloc(&ptr, bytes, pinned);
    if (e != hipSuccess) { ptr = nullptr; return e; }
    cap = bytes;
    if (counted) *counted += bytes;
    return hipSuccess;
  }

  void release() {
    if (!ptr) return;
    devbuf_free(ptr, pinned);
    if (counted) *counted -= cap;
    ptr = nullptr;
    cap = 0;
  }
};

}  // namespace gpa
