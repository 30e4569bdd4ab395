// Staging of one host-pointer call: its operands side by side in ONE DevBuf.  Host-only, no heap.  Declare every operand once,
// in the order the slots shall have (a slot starts on a multiple of `align`, the last one ends with its last byte); then
//   upload()    reserves the buffer and enqueues the uploads.  The buffer may move when it grows: device pointers exist only
//               from here on.
//   dev(i)      the device pointer of operand i -- null for an absent one (declared with a null host pointer: no bytes, no copy)
//   download()  enqueues the downloads and drains the stream (not needed before a tail call of a _dev form that drains it)
// Both return hipError_t for HIP_TRY.  The primitives are those of gpa_devbuf.h: with GPA_DEVBUF_HOST_SEAM the type runs on the
// CPU (tests/host/hoststage_check.cpp).
#pragma once
#include "gpa_devbuf.h"

namespace gpa {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

class HostStage {
 public:
  static constexpr int MAX_OPERANDS = 8;
  // align: a power of two; 256 unless the slots must sit exactly as a caller laid them out before
  HostStage(DevBuf& buf, hipStream_t stream, size_t align = 256) : buf_(buf), stream_(stream), align_(align) {}

  // Each returns the operand's index (-1: more than MAX_OPERANDS, which upload() then refuses).  `at`: a device address of the
  // caller's -- the operand takes part in the copies, not in the buffer.
  int in(const void* src, size_t bytes, void* at = nullptr) { return add(src, nullptr, bytes, at); }
  int out(void* dst, size_t bytes, void* at = nullptr) { return add(nullptr, dst, bytes, at); }
  int inout(void* host, size_t bytes, bool upload_it = true) { return add(upload_it ? host : nullptr, host, bytes, nullptr); }

  hipError_t upload() {
    hipError_t e = overflow_ ? hipErrorInvalidValue : buf_.reserve(end_, stream_);
    for (int i = 0; i < n_ && e == hipSuccess; ++i) {
      Operand& o = op_[i];
      if (!o.src && !o.dst) continue;
      o.dev = o.at ? o.at : buf_.as<unsigned char>() + o.off;
      if (o.src) e = devbuf_copy(o.dev, o.src, o.bytes, true, stream_);
    }
    return e;
  }
  void* dev(int i) const { return i >= 0 && i < n_ ? op_[i].dev : nullptr; }
  template <class T> T* as(int i) const { return static_cast<T*>(dev(i)); }
  hipError_t download() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_ && e == hipSuccess; ++i)
      if (op_[i].dst && op_[i].dev) e = devbuf_copy(op_[i].dst, op_[i].dev, op_[i].bytes, false, stream_);
    return e == hipSuccess ? devbuf_sync(stream_) : e;
  }

 private:
  struct Operand {
    const void* src;   // uploaded from here (null: not uploaded)
    void* dst;         // downloaded to here (null: not downloaded); both null: absent
    size_t bytes, off;
    void *at, *dev;    // dev stays null until upload()
  };
  int add(const void* src, void* dst, size_t bytes, void* at) {
    if (n_ == MAX_OPERANDS) { overflow_ = true; return -1; }
    size_t off = 0;
    if (!at && (src || dst)) { off = (end_ + align_ - 1) & ~(align_ - 1); end_ = off + bytes; }
    op_[n_] = Operand{src, dst, bytes, off, at, nullptr};
    return n_++;
  }
  DevBuf& buf_;
  hipStream_t stream_;
  size_t align_, end_ = 0;
  Operand op_[MAX_OPERANDS];
  int n_ = 0;
  bool overflow_ = false;
};

}  // namespace gpa
