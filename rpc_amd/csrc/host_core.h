// rpc_amd/csrc/host_core.h -- what the host layer's two files share: the CRC
// calls, pools and service (rpccrc_api.cpp) and the frame entry points
// (frames_api.cpp).  Host only and internal: every name here stays hidden
// (-fvisibility=hidden, exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/rpccrc.h"
#include "crc32_kernels.h"
#include "frames.h"
#include "workspace.h"

namespace rpccrc {

int map_hip(hipError_t e);

#define RPCCRC_TRY(expr)                      \
  do {                                        \
    const hipError_t _e = (expr);             \
    if (_e != hipSuccess) return map_hip(_e); \
  } while (0)

// ---- pools -----------------------------------------------------------------

// A cached block of device memory (or pinned host memory) lent to one call at
// a time.  `ev` is recorded on the stream of the block's last use when the
// call returns it.  The next borrower orders itself after that use: a device
// block through hipStreamWaitEvent on its own stream (no host wait, and valid
// even if the earlier stream has been destroyed since -- the event outlives
// it), a pinned block through hipEventSynchronize (the host is about to write
// it).  Replaces per-call hipMallocAsync/hipFreeAsync, whose free blocked the
// calling thread until the GPU reached it (profiles/r01h_*), and the r01
// per-thread cache that hipFree'd on every stream switch.
struct Block {
  void *p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
};

class BlockPool {
 public:
  BlockPool(bool pinned, size_t keep) : pinned_(pinned), keep_(keep) {}

  int acquire(size_t bytes, hipStream_t s, Block *out) {
    {
      std::lock_guard<std::mutex> g(mu_);
      int best = -1;
      for (int i = 0; i < (int)free_.size(); ++i)
        if (free_[i].cap >= bytes && (best < 0 || free_[i].cap < free_[best].cap)) best = i;
      if (best >= 0) {
        *out = free_[best];
        free_.erase(free_.begin() + best);
        cached_ -= out->cap;
      }
    }
    if (out->p) {
      if (out->used) RPCCRC_TRY(pinned_ ? hipEventSynchronize(out->ev) : hipStreamWaitEvent(s, out->ev, 0));
      return RPCCRC_OK;
    }
    size_t cap = pinned_ ? (64u << 10) : (1u << 20);
    while (cap < bytes) cap <<= 1;
    Block b;
    hipError_t e = pinned_ ? hipHostMalloc(&b.p, cap, hipHostMallocDefault) : hipMalloc(&b.p, cap);
    if (e != hipSuccess) {
      b.p = nullptr;
      return map_hip(e);
    }
    e = hipEventCreateWithFlags(&b.ev, hipEventDisableTiming);
    if (e != hipSuccess) {
      (void)(pinned_ ? hipHostFree(b.p) : hipFree(b.p));
      return map_hip(e);
    }
    b.cap = cap;
    *out = b;
    return RPCCRC_OK;
  }

  // Returns the block after the call has enqueued its last use on stream s.
  // recorded: the call's last kernel already recorded b.ev as its completion
  // signal (hipExtLaunchKernel stopEvent), so no marker packet is needed here.
  void release(Block &b, hipStream_t s, bool recorded = false) {
    if (!b.p) return;
    b.used = recorded || hipEventRecord(b.ev, s) == hipSuccess;
    if (!b.used) (void)hipStreamSynchronize(s); // no event: make the block idle now
    std::vector<Block> evict;
    {
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back(b);
      cached_ += b.cap;
      // Over the keep limit: drop the largest idle blocks (rare; e.g. after a
      // one-off huge batch).
      while (cached_ > keep_ && !free_.empty()) {
        auto it = std::max_element(free_.begin(), free_.end(),
                                   [](const Block &x, const Block &y) { return x.cap < y.cap; });
        cached_ -= it->cap;
        evict.push_back(*it);
        free_.erase(it);
      }
    }
    for (Block &x : evict) {
      if (x.used) (void)hipEventSynchronize(x.ev);
      (void)(pinned_ ? hipHostFree(x.p) : hipFree(x.p));
      (void)hipEventDestroy(x.ev);
    }
    b = Block();
  }

 private:
  std::mutex mu_;
  std::vector<Block> free_;
  size_t cached_ = 0;
  const bool pinned_;
  const size_t keep_;
};

// A block borrowed for the duration of one call (returned by the destructor,
// after the call has enqueued all its work on `s`).
struct Lease {
  BlockPool *pool = nullptr;
  Block b;
  hipStream_t s = nullptr;
  bool recorded = false; // the call's last launch recorded b.ev (done_event())
  Lease() = default;
  Lease(const Lease &) = delete;
  Lease &operator=(const Lease &) = delete;
  ~Lease() {
    if (pool) pool->release(b, s, recorded);
  }
  // The block's event, for the call's LAST launch on s to record as its own
  // completion (then set `recorded`).
  hipEvent_t done_event() const { return b.ev; }
  int get(BlockPool *p, size_t bytes, hipStream_t stream) {
    pool = p;
    s = stream;
    return p->acquire(bytes, stream, &b);
  }
  uint8_t *ptr() const { return static_cast<uint8_t *>(b.p); }
  // A block for the arrays that layout(WsLayout &) takes, and slack bytes behind
  // them: a measuring pass sizes the lease, the same function then carves it.
  template <class F> int get(BlockPool *p, hipStream_t stream, F &&layout, size_t slack = 0) {
    WsLayout m;
    layout(m);
    if (!m.ok()) return RPCCRC_EINVAL;
    if (const int rc = get(p, m.used() + slack, stream)) return rc;
    WsLayout w(ptr(), m.used());
    layout(w);
    return w.ok() ? RPCCRC_OK : RPCCRC_EINVAL;
  }
};

// ---- the device context ----------------------------------------------------
// Per-device state (rpccrc_api.cpp).  get_async_ctx: the calling thread's
// current device for an asynchronous call -- its initialisation status, or
// RPCCRC_EIO while the device error word holds an uncleared error.
struct DeviceCtx;
int get_async_ctx(DeviceCtx **out);
BlockPool *ws_pool(const DeviceCtx &c); // device workspaces

// ---- a ragged batch on the device (rpccrc_api.cpp) --------------------------
struct FramesCmp {
  const uint32_t *expected;
  const uint8_t *pre;
  uint8_t *verdict;
};
struct RaggedCall {
  const uint8_t *base; // the batch
  const uint64_t *offsets;
  const uint32_t *lengths;
  uint64_t n;
  uint32_t *out;
  uint32_t mode = kModeFinal;
  bool small_bodies = false; // hints
  bool route = false;
  uint32_t max_len = 0; // the caller's bound on every length (0: none)
  uint64_t span_bytes = 0;
  uint32_t *err = nullptr; // the launches' error word (as items())
  const FramesCmp *cmp = nullptr; // frames hooks
  const FramesParse *parse = nullptr;
  const FramesStamp *stamp = nullptr;
  bool compared = false; // results
  bool stamped = false;
};
int ragged(const DeviceCtx &c, RaggedCall &q, hipStream_t s);

} // namespace rpccrc
