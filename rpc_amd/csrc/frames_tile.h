// rpc_amd/csrc/frames_tile.h -- the device side of the destination-centric copy
// that the frame pack, unpack and carry share (frames_pack.hip,
// frames_unpack.hip, frames_carry.hip; the rules they run: frames_pack.h) and
// that the reply, the request and the values run through frames_splice.h: the
// readers of the layout and of the source, the wave-wide entry search, the
// masked store, a tile's entry range with its LDS staging, the lane walker, and
// the tile driver that is the body of the unpack, reply, request and values
// kernels.
#pragma once
#include "frames_pack.h"

#if defined(__HIPCC__)
namespace rpccrc {

// Entries a tile stages in LDS (offsets and source offsets: 24 KiB).  A pack
// tile of heartbeats has 1366 of them and an unpack tile of 64-byte bodies 256;
// runs of zero-size entries, or 16384 empty bodies with nul, read global memory.
constexpr uint32_t kTileLdsEntries = 1536;
static_assert(kPackWide == 64, "wave_find is one wave64");

inline dim3 grid_of(uint64_t n, int threads) { return dim3((unsigned)(n ? (n + threads - 1) / threads : 1)); } // (never 0 blocks)

// The layout, from global memory or from the tile's own slice staged in LDS
// (two types, so that each read is a plain global or LDS load, not a flat one).
struct DevOff {
  const uint64_t *o;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return o[i]; }
};
struct LdsOff {
  const uint64_t *lds;
  uint64_t base;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return lds[(uint32_t)(i - base)]; }
};
// The source buffer (Src of frames_pack.h).
struct DevSrc {
  const uint8_t *b;
  uint64_t n;
  __device__ __forceinline__ uint64_t addr() const { return (uint64_t)reinterpret_cast<uintptr_t>(b); }
  __device__ __forceinline__ uint64_t bytes() const { return n; }
  __device__ __forceinline__ void block16(uint64_t p, uint32_t w[4]) const {
    const uint4 v = *reinterpret_cast<const uint4 *>(b + p);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
  }
  __device__ __forceinline__ uint8_t byte(uint64_t p) const { return b[p]; }
};

// pack_find over all n entries by one whole wave: the 64 lanes probe 64 evenly
// spaced entries per round (4 rounds for 16M entries instead of 24 dependent
// loads).  Every lane of the wave calls it with the same x; off[0] = 0 <= x.
__device__ __forceinline__ uint64_t wave_find(const uint64_t *off, uint64_t n, uint64_t x) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint64_t probe = pack_wide_probe(lo, hi, lane);
    const bool le = probe <= hi && off[probe] <= x;
    pack_wide_step(&lo, &hi, (uint32_t)__popcll(__ballot(le)));
  }
  return lo;
}

// One piece under its byte mask (a stream or tail end, out_cap, the edge of an
// entry that is not written): a 16-byte store when whole, else whole words where
// the mask has them and single bytes otherwise.  Plain stores of exactly the
// masked bytes; nothing is read and written back -- the byte next to a masked
// one may be in flight from another copy (frames_carry.h).
__device__ __forceinline__ void store_piece(uint8_t *dst, const PackPiece &p) {
  if (p.mask == 0xFFFFu) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(p.w[0], p.w[1], p.w[2], p.w[3]);
    return;
  }
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t m = (p.mask >> (4 * j)) & 15u;
    if (m == 15u) {
      *reinterpret_cast<uint32_t *>(dst + 4 * j) = p.w[j];
    } else {
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
        if ((m >> b) & 1u) dst[4 * j + b] = (uint8_t)(p.w[j] >> (8 * b));
    }
  }
}

// A tile's entry range: waves 0 and 1 find the entries lo0 and hi covering its
// first and last byte (x0, x_last), then the layout and the source offsets of
// those entries go to LDS when they fit (`staged` offsets, else 0), so that the
// lanes' own searches cost LDS reads, not dependent global loads.  Called by the
// whole workgroup of kThreads; it returns behind the barrier that publishes
// s_off and s_src, and the caller puts a barrier before the next call.
struct TileRange {
  uint64_t lo0, hi;
  uint32_t staged;
};
template <int kThreads>
__device__ __forceinline__ TileRange tile_range(const uint64_t *offs, const uint64_t *src_off, uint64_t n, uint64_t x0,
                                                uint64_t x_last, uint64_t s_range[2], uint64_t *s_off, uint64_t *s_src) {
  const uint32_t wave = threadIdx.x >> 6;
  if (wave < 2) {
    const uint64_t e = wave_find(offs, n, wave == 0 ? x0 : x_last);
    if ((threadIdx.x & 63u) == 0) s_range[wave] = e;
  }
  __syncthreads();
  const uint64_t lo0 = s_range[0], hi = s_range[1];
  const uint64_t want = hi + 2 - lo0; // offsets lo0 .. hi + 1
  const uint32_t staged = want <= kTileLdsEntries ? (uint32_t)want : 0u;
  for (uint32_t i = threadIdx.x; i < staged; i += kThreads) {
    s_off[i] = offs[lo0 + i];
    if (i + 1 < staged) s_src[i] = src_off[lo0 + i]; // (entries lo0 .. hi: one fewer than the offsets)
  }
  __syncthreads();
  return TileRange{lo0, hi, staged};
}

// What a kernel's plan says of one piece: nothing of it is stored; it is sixteen
// source bytes through the window w (w.ok); or it goes through the resolver.
struct TilePlan {
  bool some;
  PackWin w;
};

// Lane l's piece k of a tile dealt out to kThreads lanes, in bytes from the
// tile's start.
__device__ __forceinline__ uint64_t tile_piece(uint32_t k, int threads) {
  return ((uint64_t)k * threads + threadIdx.x) * kPackPiece;
}

// The lane walker: a lane's kPieces pieces, piece k at dst + piece_at(k) (16-byte
// aligned).  plan(k), in order of k, resolves every piece first; then both block
// loads (at src + w.blk) of all whole pieces are issued before any is used; then
// they are shifted and stored; the few others go one by one through
// slow_store(k).
template <uint32_t kPieces, class At, class Plan, class Slow>
__device__ __forceinline__ void tile_walk(const uint8_t *src, uint8_t *dst, const At piece_at, Plan plan, const Slow slow_store) {
  uint64_t blk[kPieces]; // source offsets of the first blocks
  uint32_t shift[kPieces];
  uint32_t fast = 0, slow = 0; // bit k: piece k takes the fast path / goes through slow_store
#pragma unroll
  for (uint32_t k = 0; k < kPieces; ++k) {
    const TilePlan p = plan(k);
    blk[k] = 0;
    shift[k] = 0;
    if (p.some) {
      if (p.w.ok) {
        fast |= 1u << k;
        blk[k] = p.w.blk;
        shift[k] = p.w.k;
      } else {
        slow |= 1u << k;
      }
    }
  }
  uint4 l0[kPieces], l1[kPieces];
#pragma unroll
  for (uint32_t k = 0; k < kPieces; ++k) {
    if ((fast >> k) & 1u) {
      l0[k] = *reinterpret_cast<const uint4 *>(src + blk[k]);
      l1[k] = *reinterpret_cast<const uint4 *>(src + blk[k] + 16);
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kPieces; ++k) {
    if ((fast >> k) & 1u) {
      uint32_t win[4];
      pack_win_select8(l0[k].x, l0[k].y, l0[k].z, l0[k].w, l1[k].x, l1[k].y, l1[k].z, l1[k].w, shift[k], win);
      *reinterpret_cast<uint4 *>(dst + piece_at(k)) = make_uint4(win[0], win[1], win[2], win[3]);
    }
  }
  // (not unrolled: the resolvers are long and few pieces come here.  Each lane
  // walks its own set bits, so a wave makes as many rounds as its busiest lane
  // has such pieces -- mostly one -- not one round per k.)
  for (; slow; slow &= slow - 1) slow_store((uint32_t)__ffs((int)slow) - 1u);
}

// An output of `total` laid-out bytes at `out`, cut at out_cap, as tiles.
struct TileOut {
  uint64_t total;
  uint32_t mis;    // out's low four address bits
  uint8_t *out0;   // out - mis: 16-byte aligned; bytes before out are never touched
  uint64_t ntiles; // nothing at or beyond out_cap is ever written, so tiles beyond it have no work
};
__device__ __forceinline__ TileOut tile_out(const uint64_t *offs, uint64_t n, uint8_t *out, uint64_t out_cap) {
  const uint64_t total = offs[n];
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
  return TileOut{total, mis, out - mis, pack_tiles(total < out_cap ? total : out_cap, mis, kPackTile)};
}
// The tile driver: one workgroup of kThreads per tile of kPackTile output bytes
// (striding when the grid is smaller).  Per tile: tile_range over the n entries'
// layout and source offsets, then
//   tile(off, src_of, out0, tile index, mis, tile_x1, lo0, hi)
// with the readers of the staged slices or, when the range did not fit, of
// global memory; tile_x1: the layout offset the tile's bytes end at; [lo0, hi]:
// the entries covering its first and last byte.  (Scalars, not a struct: through
// one the compiler lost that mis < 16 and pack_span() kept a branch per piece.)
// s_off and s_src hold kTileLdsEntries words.
template <int kThreads, class Tile>
__device__ __forceinline__ void tile_drive(const uint64_t *offs, const uint64_t *src_off, uint64_t n, uint8_t *out,
                                           uint64_t out_cap, uint64_t s_range[2], uint64_t *s_off, uint64_t *s_src,
                                           const Tile tile) {
  const TileOut o = tile_out(offs, n, out, out_cap);
  for (uint64_t t = blockIdx.x; t < o.ntiles; t += gridDim.x) {
    const PackSpan ts = pack_span(t * kPackTile, kPackTile, o.mis, o.total); // x0 < x1: the tile holds a byte
    const TileRange r = tile_range<kThreads>(offs, src_off, n, ts.x0, ts.x1 - 1, s_range, s_off, s_src);
    if (r.staged)
      tile(LdsOff{s_off, r.lo0}, LdsOff{s_src, r.lo0}, o.out0, t, o.mis, ts.x1, r.lo0, r.hi);
    else
      tile(DevOff{offs}, DevOff{src_off}, o.out0, t, o.mis, ts.x1, r.lo0, r.hi);
    __syncthreads(); // s_range, s_off and s_src are rewritten for the next tile
  }
}

} // namespace rpccrc
#endif
