// rpc_amd/csrc/frames_pack.hip -- device-side frame pack (rpc_frames_pack_device;
// the rules and the piece resolver: frames_pack.h).
//
//   size pass -> exclusive scan (the layout) -> [CRC pass over the source
//   bodies, the caller's ragged() call] -> pack kernel -> finish pass
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_pack.h"

namespace rpccrc {

static_assert(kPackLiftCap == RPC_FRAMES_LIFT_CAP, "frames_pack.h restates the flag bit");
static_assert(kPackTypePing == RPC_FRAME_TYPE_PING && kPackTypePong == RPC_FRAME_TYPE_PONG &&
                  kPackTypeNone == RPC_FRAME_TYPE_NONE,
              "and the type codes");
static_assert(kPackMaxBody == RPC_MAX_BODY_LEN && kPackHeaderLen == RPC_HEADER_LEN_BYTES, "and the lengths");
static_assert(kPackOk == RPC_FRAME_OK && kPackControl == RPC_FRAME_CONTROL && kPackTooLarge == RPC_FRAME_TOO_LARGE &&
                  kPackMalformed == RPC_FRAME_MALFORMED && kPackSkipped == RPC_FRAME_SKIPPED,
              "and the verdicts");

namespace {

constexpr int kPackThreads = 256;
constexpr uint32_t kPiecesPerLane = kPackTile / kPackPiece / kPackThreads;
static_assert(kPiecesPerLane * kPackPiece * kPackThreads == kPackTile, "a tile is whole rounds of the workgroup");
constexpr unsigned kPackMaxGrid = 1u << 18; // workgroups; they stride over the tiles
constexpr uint32_t kPackLdsEntries = 1536;  // entries a tile stages in LDS (offsets and source offsets: 24 KiB)
static_assert(kPackWide == 64, "wave_find is one wave64");

// ---- size pass: one lane per entry -------------------------------------------
__global__ __launch_bounds__(256) void pack_size_kernel(PackArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t t = a.types ? a.types[i] : a.type;
  uint64_t off = 0;
  uint32_t len = 0;
  if (pack_is_data(t)) { // (only a data entry's offset and length are looked at)
    off = a.body_off[i];
    len = a.body_len[i];
  }
  const PackSize z = pack_size_one(t, off, len, a.bodies_bytes, a.flags);
  a.sizes[i] = z.size;
  a.src_off[i] = z.off;
  a.src_len[i] = z.len;
  a.pre[i] = z.verdict;
}

// ---- pack kernel ---------------------------------------------------------------
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
struct DevEnt {
  const uint64_t *src_off;
  const uint32_t *src_len, *crc;
  const uint16_t *types, *versions;
  uint16_t type, version;
  __device__ __forceinline__ uint64_t src(uint64_t e) const { return src_off[e]; }
  __device__ __forceinline__ void header(uint64_t e, uint32_t h[3]) const {
    const uint32_t t = types ? types[e] : type;
    const uint32_t v = versions ? versions[e] : version;
    pack_header_words(v, t, src_len[e], crc[e], h); // (a heartbeat's length and CRC are 0 here)
  }
};
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

__device__ __forceinline__ void store_piece(uint8_t *dst, const PackPiece &p) {
  if (p.mask == 0xFFFFu) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(p.w[0], p.w[1], p.w[2], p.w[3]);
  } else if (p.mask) { // a stream end, out_cap, or the edge of a frame that is not written: bytewise
    for (uint32_t b = 0; b < kPackPiece; ++b) {
      const uint32_t w = b < 4 ? p.w[0] : b < 8 ? p.w[1] : b < 12 ? p.w[2] : p.w[3];
      if ((p.mask >> b) & 1u) dst[b] = (uint8_t)(w >> (8 * (b & 3)));
    }
  }
}

// One tile's pieces (steps 3 and 4 below), over the readers of the layout and
// of the entries' source offsets.
template <class Off>
__device__ __forceinline__ void pack_tile(const PackArgs &a, const Off off, const Off src_of, const DevEnt &ent, const DevSrc &src,
                                          uint8_t *out0, uint64_t tile, uint32_t mis, uint64_t tile_x1, uint64_t lo0,
                                          uint64_t hi) {
  const auto piece_at = [&](uint32_t k) {
    return tile * kPackTile + ((uint64_t)k * kPackThreads + threadIdx.x) * kPackPiece;
  };
  uint64_t blk[kPiecesPerLane]; // source offsets of the first blocks
  uint32_t shift[kPiecesPerLane];
  uint32_t fast = 0, slow = 0; // bit k: piece k takes the fast path / goes through pack_piece
  uint64_t lo = lo0;
#pragma unroll
  for (uint32_t k = 0; k < kPiecesPerLane; ++k) {
    const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
    blk[k] = 0;
    shift[k] = 0;
    if (ps.x0 < ps.x1) {
      const uint64_t e = pack_find(off, lo, hi, ps.x0);
      const uint64_t fo = off(e), fe = off(e + 1);
      lo = e; // (the lane's next piece lies further on)
      PackWin w{false, 0, 0};
      if (pack_piece_is_body(fo, fe, ps.x0, ps.x1, ps.b0, a.out_cap))
        w = pack_win_plan(src, src_of(e) + (ps.x0 - fo - kPackHeaderLen), 0);
      if (w.ok) {
        fast |= 1u << k;
        blk[k] = w.blk;
        shift[k] = w.k;
      } else {
        slow |= 1u << k;
      }
    }
  }
  uint4 l0[kPiecesPerLane], l1[kPiecesPerLane];
#pragma unroll
  for (uint32_t k = 0; k < kPiecesPerLane; ++k) {
    if ((fast >> k) & 1u) {
      l0[k] = *reinterpret_cast<const uint4 *>(a.bodies + blk[k]);
      l1[k] = *reinterpret_cast<const uint4 *>(a.bodies + blk[k] + 16);
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kPiecesPerLane; ++k) {
    if ((fast >> k) & 1u) {
      uint32_t win[4];
      pack_win_select8(l0[k].x, l0[k].y, l0[k].z, l0[k].w, l1[k].x, l1[k].y, l1[k].z, l1[k].w, shift[k], win);
      *reinterpret_cast<uint4 *>(out0 + piece_at(k)) = make_uint4(win[0], win[1], win[2], win[3]);
    }
  }
  // (not unrolled: the resolver is long and few pieces come here.  Each lane
  // walks its own set bits, so a wave makes as many rounds as its busiest lane
  // has such pieces -- mostly one -- not one round per k.)
  for (; slow; slow &= slow - 1) {
    const uint32_t k = (uint32_t)__ffs((int)slow) - 1u;
    const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
    uint64_t last;
    store_piece(out0 + piece_at(k), pack_piece(off, ent, src, lo0, hi, ps.x0, ps.x1, ps.b0, a.out_cap, &last));
  }
}

// One workgroup per tile of kPackTile output bytes (striding when the grid is
// smaller); every lane produces kPiecesPerLane aligned 16-byte pieces, a whole
// wave writing 1 KiB of consecutive bytes per round.  Per tile:
//  1. waves 0 and 1 find the entries covering its first and last byte;
//  2. the layout and the source offsets of those entries go to LDS (when they
//     fit: a tile of heartbeats has 1366 of them, more only with runs of
//     zero-size entries), so the lanes' own searches cost LDS reads, not
//     dependent global loads;
//  3. every lane resolves all its pieces; for those that are sixteen body bytes
//     of one frame (pack_piece_is_body: nearly all) it issues the block loads of
//     all of them before it uses any, then shifts and stores;
//  4. the other pieces -- headers, frame edges, stream ends -- go through
//     pack_piece one by one.
__global__ __launch_bounds__(kPackThreads) void pack_kernel(PackArgs a) {
  __shared__ uint64_t s_range[2];
  __shared__ uint64_t s_off[kPackLdsEntries], s_src[kPackLdsEntries];
  const uint64_t total = a.offs[a.n];
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(a.out) & 15u);
  uint8_t *const out0 = a.out - mis; // 16-byte aligned; bytes before a.out are never touched
  // nothing at or beyond out_cap is ever written, so tiles beyond it have no work
  const uint64_t ntiles = pack_tiles(total < a.out_cap ? total : a.out_cap, mis, kPackTile);
  const DevEnt ent{a.src_off, a.src_len, a.crc, a.types, a.versions, a.type, a.version};
  const DevSrc src{a.bodies, a.bodies_bytes};
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const PackSpan ts = pack_span(tile * kPackTile, kPackTile, mis, total); // x0 < x1: the tile holds a byte
    const uint32_t wave = threadIdx.x >> 6;
    if (wave < 2) { // the entries covering the tile's first and last byte
      const uint64_t e = wave_find(a.offs, a.n, wave == 0 ? ts.x0 : ts.x1 - 1);
      if ((threadIdx.x & 63u) == 0) s_range[wave] = e;
    }
    __syncthreads();
    const uint64_t lo0 = s_range[0], hi = s_range[1];
    const uint64_t want = hi + 2 - lo0; // offsets lo0 .. hi + 1
    const uint32_t staged = want <= kPackLdsEntries ? (uint32_t)want : 0u;
    for (uint32_t i = threadIdx.x; i < staged; i += kPackThreads) {
      s_off[i] = a.offs[lo0 + i];
      if (i + 1 < staged) s_src[i] = a.src_off[lo0 + i]; // (entries lo0 .. hi: one fewer than the offsets)
    }
    __syncthreads();
    if (staged)
      pack_tile(a, LdsOff{s_off, lo0}, LdsOff{s_src, lo0}, ent, src, out0, tile, mis, ts.x1, lo0, hi);
    else
      pack_tile(a, DevOff{a.offs}, DevOff{a.src_off}, ent, src, out0, tile, mis, ts.x1, lo0, hi);
    __syncthreads(); // s_range, s_off and s_src are rewritten for the next tile
  }
}

// ---- finish: final verdicts, offsets, per-connection byte CSR, total ----------
__global__ __launch_bounds__(256) void pack_finish_kernel(PackArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t total = a.offs[a.n];
  if (i == 0 && a.total) *a.total = total;
  if (i < a.n) {
    const uint64_t at = a.offs[i];
    if (a.frame_off) a.frame_off[i] = at;
    if (a.verdict) a.verdict[i] = pack_final_verdict(a.pre[i], at, a.offs[i + 1] - at, a.out_cap);
  }
  if (a.conn_bytes_first && i <= a.nconn) {
    uint64_t f = i < a.nconn ? a.conn_first[i] : a.n;
    if (f > a.n) f = a.n; // (a CSR that runs past the entries reads as the end)
    a.conn_bytes_first[i] = a.offs[f];
  }
}

dim3 grid_of(uint64_t n, int threads) { return dim3((unsigned)(n ? (n + threads - 1) / threads : 1)); }

} // namespace

hipError_t launch_frames_pack_layout(const PackArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(pack_size_kernel, grid_of(a.n, 256), dim3(256), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return excl_scan(a.sizes, a.offs, a.n, a.scan_tmp, s);
}

hipError_t launch_frames_pack_write(const PackArgs &a, hipStream_t s) {
  if (a.out && a.out_cap && a.n) {
    // (the total is on the device only: the grid covers what out_cap and n allow,
    // and workgroups past the last tile leave at once)
    uint64_t most = a.out_cap;
    if (!(a.flags & RPC_FRAMES_LIFT_CAP)) most = std::min<uint64_t>(most, a.n * (uint64_t)(kPackHeaderLen + kPackMaxBody));
    const uint64_t tiles = pack_tiles(most, 15, kPackTile);
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)std::min<uint64_t>(tiles, kPackMaxGrid)), dim3(kPackThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pack_finish_kernel, grid_of(std::max(a.n, a.nconn + 1), 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

} // namespace rpccrc
