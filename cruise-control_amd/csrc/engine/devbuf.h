// How the host side of the query kernels owns and lays out device memory (DESIGN.md "Query workspaces"): DevBuf and
// PinBuf own one block each, Carver cuts a block into typed pieces. No HIP here: device.h includes this, and the test
// emulation builds device.h with a plain host compiler. The four allocation functions are defined once per build: by
// the product in device.cpp (hipMalloc / hipFree / hipHostMalloc / hipHostFree), by the test emulation in
// tests/emu/device_emu.cpp (it has none of these buffers: its alloc throws).
#pragma once
#include <cstddef>
#include <stdexcept>
#include <utility>

namespace ccmi {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Weak: a build that defines none of them still links and loads, and has no buffers (ensure throws).
#define CCMI_WEAK __attribute__((weak))
CCMI_WEAK void* deviceAlloc(size_t bytes);  // throws; never null
CCMI_WEAK void deviceFree(void* p) noexcept;
CCMI_WEAK void* pinnedAlloc(size_t bytes);  // throws; never null
CCMI_WEAK void pinnedFree(void* p) noexcept;
#undef CCMI_WEAK

// An owning, move-only block that only grows. One growth rule for everyone (a decision, not a measurement): a first
// allocation is align256(bytes), at least 256, so a fixed-size workspace pays nothing extra; a regrowth is
// align256(bytes + bytes / 4), so a growing output amortises. ensure never keeps the old contents: the old block is
// freed before the new one is allocated, and a failed allocation leaves the buffer empty and reusable. The frees run on
// whatever device is current: ~Device and the aggregator's destroy make theirs current first.
template <void* (*Alloc)(size_t), void (*Free)(void*) noexcept>
class GrowBuf {
 public:
  GrowBuf() = default;
  GrowBuf(GrowBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  GrowBuf& operator=(GrowBuf&& o) noexcept {
    GrowBuf t(std::move(o));  // this block goes with t
    std::swap(p_, t.p_);
    std::swap(cap_, t.cap_);
    return *this;
  }
  ~GrowBuf() { release(); }
  void* ensure(size_t bytes) {
    if (bytes > cap_) {
      const size_t want = p_ ? align256(bytes + bytes / 4) : align256(bytes ? bytes : 1);
      release();
      if (!Alloc) throw std::logic_error("this build has no allocation functions for devbuf.h");
      p_ = Alloc(want);
      cap_ = want;
    }
    return p_;
  }
  void* get() const { return p_; }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void release() {
    if (p_) Free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  void* p_ = nullptr;
  size_t cap_ = 0;
};
using DevBuf = GrowBuf<deviceAlloc, deviceFree>;
using PinBuf = GrowBuf<pinnedAlloc, pinnedFree>;  // pinned host memory: the staging of one copy in or out

// Cuts one block into typed pieces. take(p, count) gives p room for `count` elements of P. The guarantee of the type:
// every piece starts on a 256-byte boundary of the block and owns align256(sizeof(P) * count) bytes, at least 256, so a
// zero-count piece is still a valid pointer of its own, and a kernel that finishes a list with whole 16-byte stores
// (records in pairs, int32 lists in fours) stays inside its own piece. A pass over a null base places nothing and leaves
// the size in `off`; a pass over the block places the pieces.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <class P>
  void take(P*& p, size_t count) {
    p = (P*)(base ? base + off : nullptr);
    off += align256(count ? sizeof(P) * count : 1);
  }
};

// The two passes of one layout(Carver&): sized over a null base, room made in `buf`, placed there. Returns the size.
template <class Buf, class Layout>
size_t carve(Buf& buf, Layout layout) {
  Carver sizing(nullptr);
  layout(sizing);
  Carver placing(buf.ensure(sizing.off));
  layout(placing);
  return placing.off;
}

}  // namespace ccmi
