// rpc_amd/csrc/crc32_gather.hip -- the gather fold for gfx950 (crc32_gather.h,
// DESIGN.md 4.10): folds the per-segment CRCs of bodies given as segment lists
// (rpc_crc32_device_gather) into per-body CRCs, optionally continuing from a
// running CRC per body (zlib's crc32(crc, buf, len)).
//
//  * gather_lane_kernel: one lane per body, 64 consecutive bodies per wave.  A
//    body of <= kGatherLaneMax segments is folded serially by its lane; a longer
//    one is appended to a worklist (one atomicAdd per wave and list), and a wide
//    one (>= kGatherWideMin segments) is cut into tiles of kGatherTile segments,
//    each an entry of the tile list.
//  * gather_block_kernel: grid-strides over a worklist, one workgroup per body.
//    A tile is NT runs of R consecutive pairs: each thread Horner-folds its
//    run, the lanes of a wave are combined with the monoid in 6 shuffle steps,
//    the waves through LDS, and thread 0 carries the tiles forward from the seed.
//    Narrow bodies: the pairs are the segments' (crc, len).  Wide bodies: the
//    pairs are their tiles' values (64-bit lengths), from
//  * gather_tile_kernel: grid-strides over the tile list, one workgroup per
//    tile, the same tree; stores the tile's pair.  This is what spreads one
//    enormous body over the chip.
// The shift maps (32 KiB, kShiftNibWords) sit in LDS in all three, copied as
// the chunk combine copies them.  Every value is exact GF(2) arithmetic: the
// result does not depend on how a body is cut into runs, waves and tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "crc32_gather.h"
#include "crc32_kernels.h"
#include "crc32_nib.h"

namespace rpccrc {
namespace {

constexpr uint32_t kLaneNT = 256;

template <uint32_t NT>
__device__ __forceinline__ void copy_nib(uint32_t *nib, const uint4 *src, uint32_t t) {
  uint4 *dst = reinterpret_cast<uint4 *>(nib);
#pragma unroll
  for (uint32_t q = 0; q < kShiftNibWords / 4 / NT; ++q) dst[q * NT + t] = src[q * NT + t];
}

// Body i's segment range, inside [0, nseg] whatever seg_first holds (a list that
// breaks the caller's contract gives wrong CRCs, never an access outside the
// call's arrays; the worklists are guarded by their capacities the same way).
__device__ __forceinline__ void body_range(const GatherArgs &a, uint64_t i, uint64_t *s0, uint64_t *s1) {
  const uint64_t e = a.seg_first[i + 1] < a.nseg ? a.seg_first[i + 1] : a.nseg;
  const uint64_t b = a.seg_first[i] < e ? a.seg_first[i] : e;
  *s0 = b;
  *s1 = e;
}

// (c, l) . pairs [r0, r1) in order; four pairs' loads in flight.  A pair past
// r1 enters as the identity (0, 0).
template <class LenT>
__device__ __forceinline__ void fold_run(const uint32_t *nib, const uint32_t *crc, const LenT *len, uint64_t r0,
                                         uint64_t r1, uint32_t *c, uint64_t *l) {
  uint32_t acc = *c;
  uint64_t sum = *l;
  for (uint64_t s = r0; s < r1; s += 4) {
    LenT L[4];
    uint32_t C[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const bool live = s + q < r1;
      L[q] = live ? len[s + q] : (LenT)0;
      C[q] = live ? crc[s + q] : 0u;
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      acc = nib_shift(nib, L[q], acc) ^ C[q];
      sum += L[q];
    }
  }
  *c = acc;
  *l = sum;
}

// One step of an ordered tree reduction: lane t with (t & (2m - 1)) == 0 takes
// lane t + m's pair on its right.
__device__ __forceinline__ void tree_step(const uint32_t *nib, uint32_t lane, uint32_t m, uint32_t *c, uint64_t *l) {
  const uint32_t c2 = (uint32_t)__shfl_down((int)*c, m, 64);
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)*l, m, 64);
  const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(*l >> 32), m, 64);
  const uint64_t l2 = ((uint64_t)hi << 32) | lo;
  if ((lane & (2u * m - 1u)) == 0u) {
    *c = nib_shift(nib, l2, *c) ^ c2;
    *l += l2;
  }
}

// The product of the pairs [r0, r1), r1 - r0 <= NT * R, by the whole workgroup:
// thread t folds the run r0 + t R .. + R, then the lanes, then the waves.  The
// result is thread 0's.  Two barriers; wave_c / wave_l are free again after it.
template <uint32_t NT, class LenT>
__device__ __forceinline__ void block_tile(const uint32_t *nib, const uint32_t *crc, const LenT *len, uint64_t r0,
                                           uint64_t r1, uint64_t R, uint32_t *wave_c, uint64_t *wave_l, uint32_t *c,
                                           uint64_t *l) {
  constexpr uint32_t NW = NT / 64;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint64_t a = r0 + t * R, b = a + R;
  a = a < r1 ? a : r1;
  b = b < r1 ? b : r1;
  *c = 0;
  *l = 0;
  fold_run(nib, crc, len, a, b, c, l);
#pragma unroll
  for (uint32_t m = 1; m < 64; m <<= 1) tree_step(nib, lane, m, c, l);
  if (lane == 0) {
    wave_c[wave] = *c;
    wave_l[wave] = *l;
  }
  __syncthreads();
  if (wave == 0) {
    *c = lane < NW ? wave_c[lane] : 0u;
    *l = lane < NW ? wave_l[lane] : 0ull;
#pragma unroll
    for (uint32_t m = 1; m < NW; m <<= 1) tree_step(nib, lane, m, c, l);
  }
  __syncthreads();
}

__device__ __forceinline__ uint64_t wave_bcast64(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
  return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(kLaneNT) gather_lane_kernel(GatherArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t nib[kShiftNibWords];
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t & 63u;
  copy_nib<kLaneNT>(nib, a.shift_nib, t);
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kLaneNT;
  for (uint64_t b0 = (uint64_t)blockIdx.x * kLaneNT; b0 < a.n; b0 += stride) { // (block-uniform)
    const uint64_t i = b0 + t;
    const bool live = i < a.n;
    uint64_t s0 = 0, s1 = 0;
    if (live) body_range(a, i, &s0, &s1);
    const uint64_t cnt = s1 - s0;
    if (live && cnt <= kGatherLaneMax) {
      uint32_t c = a.seed ? a.seed[i] : 0u; // read before out[i] is written (out may be seed)
      uint64_t l = 0;
      fold_run(nib, a.seg_crc, a.seg_len, s0, s1, &c, &l);
      a.out[i] = c;
    }
    // Longer bodies: one atomicAdd per wave and list, the lanes take
    // consecutive slots in lane order.
#pragma unroll
    for (uint32_t w = 0; w < 2; ++w) {
      const bool mine = live && cnt > kGatherLaneMax && (cnt >= kGatherWideMin) == (w == 1u);
      const uint64_t mask = __ballot(mine);
      if (mask == 0) continue; // (wave-uniform)
      const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
      uint64_t pos = 0;
      if (lane == leader) pos = atomicAdd(reinterpret_cast<unsigned long long *>(a.work_n + w),
                                          (unsigned long long)__popcll(mask));
      const uint64_t slot = wave_bcast64(pos, leader) + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
      const bool keep = mine && slot < a.work_cap[w];
      if (keep) a.work[w][slot] = i;
      if (w == 1u && keep) { // a wide body: its tiles, consecutive in the tile list
        const uint64_t nt = (cnt + kGatherTile - 1) / kGatherTile;
        const uint64_t tb = atomicAdd(reinterpret_cast<unsigned long long *>(a.work_n + 2), (unsigned long long)nt);
        a.wide_tile0[slot] = tb;
        for (uint64_t q = tb; q < tb + nt && q < a.tile_cap; ++q) a.tile_slot[q] = slot;
      }
    }
  }
}

// A wide body's tiles in the tile list, inside [0, tile_cap].
__device__ __forceinline__ void wide_tiles(const GatherArgs &a, uint64_t slot, uint64_t cnt, uint64_t *q0, uint64_t *q1) {
  const uint64_t tb = a.wide_tile0[slot] < a.tile_cap ? a.wide_tile0[slot] : a.tile_cap;
  const uint64_t nt = (cnt + kGatherTile - 1) / kGatherTile;
  *q0 = tb;
  *q1 = nt < a.tile_cap - tb ? tb + nt : a.tile_cap;
}

// One workgroup per tile of a wide body: the tile's pair into tile_crc / tile_len.
__global__ void __launch_bounds__(kGatherWideNT) gather_tile_kernel(GatherArgs a) {
  constexpr uint32_t NT = kGatherWideNT;
  __shared__ __attribute__((aligned(16))) uint32_t nib[kShiftNibWords];
  __shared__ uint32_t wave_c[NT / 64];
  __shared__ uint64_t wave_l[NT / 64];
  const uint64_t wides = a.work_n[1] < a.work_cap[1] ? a.work_n[1] : a.work_cap[1];
  const uint64_t tiles = a.work_n[2] < a.tile_cap ? a.work_n[2] : a.tile_cap;
  if (blockIdx.x >= tiles) return; // (block-uniform) nothing for this workgroup
  copy_nib<NT>(nib, a.shift_nib, threadIdx.x);
  __syncthreads();
  for (uint64_t q = blockIdx.x; q < tiles; q += gridDim.x) { // (block-uniform)
    uint32_t c = 0;
    uint64_t l = 0;
    const uint64_t slot = a.tile_slot[q];
    if (slot < wides) { // (block-uniform; always, for a list that keeps the contract)
      uint64_t s0, s1, q0, q1;
      body_range(a, a.work[1][slot], &s0, &s1);
      wide_tiles(a, slot, s1 - s0, &q0, &q1);
      if (q >= q0 && q < q1) {
        const uint64_t r0 = s0 + (q - q0) * kGatherTile;
        const uint64_t r1 = s1 - r0 < kGatherTile ? s1 : r0 + kGatherTile;
        block_tile<NT>(nib, a.seg_crc, a.seg_len, r0, r1, (r1 - r0 + NT - 1) / NT, wave_c, wave_l, &c, &l);
      }
    }
    if (threadIdx.x == 0) {
      a.tile_crc[q] = c;
      a.tile_len[q] = l;
    }
  }
}

// One workgroup per body of worklist W: list 0 folds the body's segments,
// list 1 the body's tile values.
template <uint32_t W>
__global__ void __launch_bounds__(kGatherNarrowNT) gather_block_kernel(GatherArgs a) {
  constexpr uint32_t NT = kGatherNarrowNT;
  using LenT = typename std::conditional<W == 0, uint32_t, uint64_t>::type;
  __shared__ __attribute__((aligned(16))) uint32_t nib[kShiftNibWords];
  __shared__ uint32_t wave_c[NT / 64];
  __shared__ uint64_t wave_l[NT / 64];
  const uint64_t count = a.work_n[W] < a.work_cap[W] ? a.work_n[W] : a.work_cap[W];
  if (blockIdx.x >= count) return; // (block-uniform) nothing for this workgroup
  const uint32_t t = threadIdx.x;
  copy_nib<NT>(nib, a.shift_nib, t);
  __syncthreads();
  const uint32_t *crc = W == 0 ? a.seg_crc : a.tile_crc;
  const LenT *len = reinterpret_cast<const LenT *>(W == 0 ? (const void *)a.seg_len : (const void *)a.tile_len);
  for (uint64_t k = blockIdx.x; k < count; k += gridDim.x) { // (block-uniform)
    const uint64_t i = a.work[W][k];
    uint64_t p0, p1;
    body_range(a, i, &p0, &p1);
    if (W == 1) wide_tiles(a, k, p1 - p0, &p0, &p1);
    const uint64_t per = (p1 - p0 + NT - 1) / NT;
    const uint64_t R = per < kGatherRunMax ? (per ? per : 1) : kGatherRunMax;
    uint32_t carry = (t == 0 && a.seed) ? a.seed[i] : 0u; // thread 0's: (seed, .) . tile . tile ...
    for (uint64_t base = p0; base < p1; base += R * NT) { // (block-uniform)
      uint32_t c;
      uint64_t l;
      block_tile<NT>(nib, crc, len, base, p1 - base < R * NT ? p1 : base + R * NT, R, wave_c, wave_l, &c, &l);
      if (t == 0) carry = nib_shift(nib, l, carry) ^ c;
    }
    if (t == 0) a.out[i] = carry; // after the seed's read above (out may be seed)
  }
}

uint64_t cap_narrow(uint64_t n, uint64_t nseg) { return std::min<uint64_t>(n, nseg / (kGatherLaneMax + 1)); }
uint64_t cap_wide(uint64_t n, uint64_t nseg) { return std::min<uint64_t>(n, nseg / kGatherWideMin); }
// ceil(cnt / tile) summed over bodies with disjoint segment ranges
uint64_t cap_tiles(uint64_t n, uint64_t nseg) { return nseg / kGatherTile + cap_wide(n, nseg); }

} // namespace

void gather_layout(WsLayout &w, uint64_t n, uint64_t nseg, GatherArgs *a) {
  a->work_n = w.take<uint64_t>(32); // (a 256-byte line of its own)
  a->work_cap[0] = cap_narrow(n, nseg);
  a->work_cap[1] = cap_wide(n, nseg);
  a->tile_cap = cap_tiles(n, nseg);
  a->work[0] = w.take<uint64_t>(a->work_cap[0]);
  a->work[1] = w.take<uint64_t>(a->work_cap[1]);
  a->wide_tile0 = w.take<uint64_t>(a->work_cap[1]);
  a->tile_slot = w.take<uint64_t>(a->tile_cap);
  a->tile_len = w.take<uint64_t>(a->tile_cap);
  a->tile_crc = w.take<uint32_t>(a->tile_cap);
}

hipError_t launch_gather_fold(const GatherArgs &a, int cus, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint64_t cu = cus > 0 ? (uint64_t)cus : 256u;
  hipError_t e = hipMemsetAsync(a.work_n, 0, 3 * sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  // LDS (32 KiB a workgroup) admits four 256-thread workgroups a CU, the wave
  // limit two of 1024 threads.
  const uint64_t lane_blocks = std::min<uint64_t>((a.n + kLaneNT - 1) / kLaneNT, 4 * cu);
  hipLaunchKernelGGL(gather_lane_kernel, dim3((unsigned)lane_blocks), dim3(kLaneNT), 0, s, a);
  if (a.work_cap[0] > 0)
    hipLaunchKernelGGL(gather_block_kernel<0>, dim3((unsigned)std::min<uint64_t>(a.work_cap[0], 4 * cu)),
                       dim3(kGatherNarrowNT), 0, s, a);
  if (a.work_cap[1] > 0) {
    hipLaunchKernelGGL(gather_tile_kernel, dim3((unsigned)std::min<uint64_t>(a.tile_cap, 2 * cu)), dim3(kGatherWideNT),
                       0, s, a);
    hipLaunchKernelGGL(gather_block_kernel<1>, dim3((unsigned)std::min<uint64_t>(a.work_cap[1], 4 * cu)),
                       dim3(kGatherNarrowNT), 0, s, a);
  }
  return hipGetLastError();
}

} // namespace rpccrc
