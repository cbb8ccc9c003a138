// rpc_amd/csrc/workspace.h -- carving several arrays out of one leased device
// block.  A workspace's layout is written once, as a function over a WsLayout:
// a measuring pass (no base) sizes the lease, a carving pass over the leased
// block places the arrays.  Host only; no HIP types.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rpccrc {

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

class WsLayout {
 public:
  WsLayout() = default; // a measuring pass: every take returns nullptr and only counts
  WsLayout(void *base, size_t cap) : base_(static_cast<uint8_t *>(base)), cap_(base ? cap : SIZE_MAX) {}

  // count elements of T at the next 256-byte step (count = 0: nothing, legal).
  // Once a take does not fit cap (or overflows size_t) the layout is not ok(),
  // stays so, and every further take returns nullptr.
  template <class T> T *take(size_t count) {
    if (count > (SIZE_MAX - 255) / sizeof(T)) ok_ = false;
    const size_t bytes = ok_ ? align256(count * sizeof(T)) : 0;
    if (bytes > cap_ - used_) ok_ = false;
    if (!ok_) return nullptr;
    uint8_t *p = base_ ? base_ + used_ : nullptr;
    used_ += bytes;
    return reinterpret_cast<T *>(p);
  }
  // What is left behind the arrays taken so far, not rounded (*bytes of it).
  void *rest(size_t *bytes) const {
    *bytes = ok_ && base_ ? cap_ - used_ : 0;
    return ok_ && base_ ? base_ + used_ : nullptr;
  }
  size_t used() const { return used_; }
  bool ok() const { return ok_; }

 private:
  uint8_t *base_ = nullptr;
  size_t cap_ = SIZE_MAX;
  size_t used_ = 0;
  bool ok_ = true;
};

} // namespace rpccrc
