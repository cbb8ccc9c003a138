// rpc_amd/csrc/frames_stage.h -- the staging rounds of the walks over delivered
// bodies, shared by the frame route, the frame resolve and the frame args
// (frames_route.hip, frames_resolve.hip, frames_args.hip): a
// workgroup of kRouteEntries lanes, one entry each, brings its bodies (the
// args: its `params` spans) into LDS in rounds of kRouteStage bytes and each
// lane walks its own there through an LdsBody.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frames_route.h"

namespace rpccrc {

// A staged body: the lane walks it word by word (one aligned LDS read per four
// bytes; a byte read per byte at 64 unrelated addresses would be four times the
// LDS instructions and their bank conflicts).
struct LdsBody {
  const uint32_t *lds;
  uint32_t base; // byte offset of the body in the staging area
  uint32_t pos = 0, w = 0;
  __device__ __forceinline__ LdsBody(const uint32_t *l, uint32_t b) : lds(l), base(b) {}
  __device__ __forceinline__ uint32_t next() {
    const uint32_t p = base + pos;
    if ((p & 3u) == 0 || pos == 0) w = lds[p >> 2];
    ++pos;
    return (w >> (8 * (p & 3u))) & 0xFFu;
  }
  __device__ __forceinline__ bool aligned() const { return ((base + pos) & 3u) == 0; }
  __device__ __forceinline__ uint32_t word() const { return lds[(base + pos) >> 2]; }
  __device__ __forceinline__ void skip4() { pos += 4; }
  __device__ __forceinline__ uint32_t at(uint32_t i) const {
    const uint32_t p = base + i;
    return (lds[p >> 2] >> (8 * (p & 3u))) & 0xFFu;
  }
};

// Every lane of a workgroup of kRouteEntries lanes calls this once, with its
// entry's body (off, len inside [0, bodies_bytes)) when pending.  The bodies
// are staged in LDS in rounds: a round's window starts at the 16-byte address
// step at or below the first pending body and takes every pending body that
// lies inside its kRouteStage bytes (the unpack's bodies are back to back: a
// run of consecutive entries; any other order still ends, a body per round at
// the least).  Whole 16-byte blocks inside the buffer come with aligned
// 16-byte loads, the edges that would leave [bodies, bodies + bodies_bytes)
// bytewise.  Then each lane of the round calls walk(LdsBody &) on its own body
// in LDS.  The first barrier of the first round also orders what the caller
// wrote to LDS before the call.
template <class Walk>
__device__ __forceinline__ void stage_rounds(const uint8_t *bodies, uint64_t bodies_bytes, uint64_t off, uint32_t len,
                                             bool pending, Walk walk) {
  constexpr uint32_t kNone32 = 0xFFFFFFFFu;
  __shared__ uint4 s_stage[kRouteStage / 16];
  __shared__ uint64_t s_off[kRouteEntries];
  __shared__ uint32_t s_first, s_end;
  const uint32_t t = threadIdx.x;
  s_off[t] = off;
  const uint64_t base_addr = (uint64_t)reinterpret_cast<uintptr_t>(bodies);
  const uint32_t mis = (uint32_t)(base_addr & 15u);
  const uint32_t *stage32 = reinterpret_cast<const uint32_t *>(s_stage);

  for (;;) {
    if (t == 0) s_first = kNone32, s_end = 0;
    __syncthreads(); // (also: s_off and the caller's LDS are written; the last round's walks are over)
    if (pending) atomicMin(&s_first, t);
    __syncthreads();
    const uint32_t first = s_first;
    if (first == kNone32) break;
    // the window in "aligned space": offsets from bodies - mis, so that a multiple
    // of 16 there is a 16-byte address step
    const uint64_t w0 = (s_off[first] + mis) & ~(uint64_t)15;
    const uint64_t x0 = off + mis;
    const bool mine = pending && x0 >= w0 && x0 + len <= w0 + kRouteStage;
    if (mine) atomicMax(&s_end, (uint32_t)(x0 + len - w0));
    __syncthreads();
    const uint32_t blocks = (s_end + 15u) / 16u; // >= 1: the first pending body is in
    const uint64_t lim = bodies_bytes + mis;     // the buffer is [mis, lim) in aligned space
    for (uint32_t k = t; k < blocks; k += kRouteEntries) {
      const uint64_t x = w0 + (uint64_t)k * 16u;
      if (x >= mis && x + 16u <= lim) {
        s_stage[k] = *reinterpret_cast<const uint4 *>(bodies + (x - mis));
      } else { // the buffer's first or last block: only its bytes inside the buffer
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t b = 0; b < 16; ++b)
          if (x + b >= mis && x + b < lim) w[b >> 2] |= (uint32_t)bodies[x + b - mis] << (8 * (b & 3u));
        s_stage[k] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    __syncthreads();
    if (mine) {
      LdsBody body(stage32, (uint32_t)(x0 - w0));
      walk(body);
      pending = false;
    }
  }
}

} // namespace rpccrc
