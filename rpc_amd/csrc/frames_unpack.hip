// rpc_amd/csrc/frames_unpack.hip -- device-side frame unpack
// (rpc_frames_unpack_device; the rules and the piece resolver: frames_unpack.h,
// DESIGN.md 4.13).
//
//   size pass -> exclusive scan (the layout) -> unpack kernel -> finish pass
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_unpack.h"

namespace rpccrc {

static_assert(kUnpackServer == RPC_FRAMES_SERVER && kUnpackClient == RPC_FRAMES_CLIENT,
              "frames_unpack.h restates the role bits");
static_assert(kUnpackTypeData == RPC_FRAME_TYPE_DATA, "and the data type code");

namespace {

constexpr int kUnpackThreads = 256;
constexpr uint32_t kPiecesPerLane = kPackTile / kPackPiece / kUnpackThreads;
static_assert(kPiecesPerLane * kPackPiece * kUnpackThreads == kPackTile, "a tile is whole rounds of the workgroup");
constexpr unsigned kUnpackMaxGrid = 1u << 18; // workgroups; they stride over the tiles
// Entries a tile stages in LDS (offsets and source offsets: 24 KiB).  A tile of
// 64-byte bodies has 256 of them; one of empty bodies with nul has 16384 and
// reads global memory.
constexpr uint32_t kUnpackLdsEntries = 1536;
static_assert(kPackWide == 64, "wave_find is one wave64");

struct DevHdr {
  const uint8_t *b;
  __device__ __forceinline__ uint8_t byte(uint64_t p) const { return b[p]; }
};

// ---- size pass: one lane per entry -------------------------------------------
__global__ __launch_bounds__(256) void unpack_size_kernel(UnpackArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint8_t v = a.verdict_in[i];
  uint64_t off = 0;
  if (v == kPackOk || v == kPackControl) off = a.frame_off[i]; // (only then is the offset looked at)
  const UnpackSize z = unpack_size_one(DevHdr{a.stream}, v, off, a.stream_bytes, a.flags, a.nul);
  a.sizes[i] = z.size;
  a.src_off[i] = z.src;
  a.ver[i] = z.version;
  a.pre[i] = z.verdict;
}

// ---- unpack kernel -------------------------------------------------------------
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

// pack_find over all n entries by one whole wave (frames_pack.hip's wave_find).
// Every lane of the wave calls it with the same x; off[0] = 0 <= x.
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
  } else if (p.mask) { // an entry edge next to one not written, out_cap, the output's ends: bytewise
    for (uint32_t b = 0; b < kPackPiece; ++b) {
      const uint32_t w = b < 4 ? p.w[0] : b < 8 ? p.w[1] : b < 12 ? p.w[2] : p.w[3];
      if ((p.mask >> b) & 1u) dst[b] = (uint8_t)(w >> (8 * (b & 3)));
    }
  }
}

// One tile's pieces, over the readers of the layout and of the entries' source
// offsets: every lane resolves all its pieces; for those that are sixteen body
// bytes of one entry it issues the block loads of all of them before it uses
// any, then shifts and stores; the others go through unpack_piece one by one.
template <class Off>
__device__ __forceinline__ void unpack_tile(const UnpackArgs &a, const Off off, const Off src_of, const DevSrc &src,
                                            uint8_t *out0, uint64_t tile, uint32_t mis, uint64_t tile_x1, uint64_t lo0,
                                            uint64_t hi) {
  const auto piece_at = [&](uint32_t k) {
    return tile * kPackTile + ((uint64_t)k * kUnpackThreads + threadIdx.x) * kPackPiece;
  };
  uint64_t blk[kPiecesPerLane]; // stream offsets of the first blocks
  uint32_t shift[kPiecesPerLane];
  uint32_t fast = 0, slow = 0; // bit k: piece k takes the fast path / goes through unpack_piece
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
      if (unpack_piece_is_body(fo, fe, ps.x0, ps.x1, ps.b0, a.nul, a.out_cap))
        w = pack_win_plan(src, src_of(e) + (ps.x0 - fo), 0);
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
      l0[k] = *reinterpret_cast<const uint4 *>(a.stream + blk[k]);
      l1[k] = *reinterpret_cast<const uint4 *>(a.stream + blk[k] + 16);
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
  // (not unrolled: the resolver is long.  Each lane walks its own set bits.)
  for (; slow; slow &= slow - 1) {
    const uint32_t k = (uint32_t)__ffs((int)slow) - 1u;
    const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
    store_piece(out0 + piece_at(k), unpack_piece(off, src_of, src, lo0, hi, ps.x0, ps.x1, ps.b0, a.nul, a.out_cap));
  }
}

// One workgroup per tile of kPackTile output bytes (striding when the grid is
// smaller), as the pack kernel: waves 0 and 1 find the entries covering the
// tile's first and last byte, the layout and the source offsets of those
// entries go to LDS when they fit, then every lane produces its pieces.
// Five waves per SIMD (96 VGPRs, no scratch) where the compiler settles on four
// (98): interleaved on one box 904 -> 813 us on 1.9M small frames and 403 -> 384
// us on 64 MiB bodies; six (80 VGPRs, 80 bytes of scratch) gave 856 and 450.
__global__ __launch_bounds__(kUnpackThreads) __attribute__((amdgpu_waves_per_eu(5))) void unpack_kernel(UnpackArgs a) {
  __shared__ uint64_t s_range[2];
  __shared__ uint64_t s_off[kUnpackLdsEntries], s_src[kUnpackLdsEntries];
  const uint64_t total = a.offs[a.n];
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(a.out) & 15u);
  uint8_t *const out0 = a.out - mis; // 16-byte aligned; bytes before a.out are never touched
  // nothing at or beyond out_cap is ever written, so tiles beyond it have no work
  const uint64_t ntiles = pack_tiles(total < a.out_cap ? total : a.out_cap, mis, kPackTile);
  const DevSrc src{a.stream, a.stream_bytes};
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
    const uint32_t staged = want <= kUnpackLdsEntries ? (uint32_t)want : 0u;
    for (uint32_t i = threadIdx.x; i < staged; i += kUnpackThreads) {
      s_off[i] = a.offs[lo0 + i];
      if (i + 1 < staged) s_src[i] = a.src_off[lo0 + i]; // (entries lo0 .. hi: one fewer than the offsets)
    }
    __syncthreads();
    if (staged)
      unpack_tile(a, LdsOff{s_off, lo0}, LdsOff{s_src, lo0}, src, out0, tile, mis, ts.x1, lo0, hi);
    else
      unpack_tile(a, DevOff{a.offs}, DevOff{a.src_off}, src, out0, tile, mis, ts.x1, lo0, hi);
    __syncthreads(); // s_range, s_off and s_src are rewritten for the next tile
  }
}

// ---- finish: final verdicts, reply plan, layout, per-connection byte CSR, total --
__global__ __launch_bounds__(256) void unpack_finish_kernel(UnpackArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t total = a.offs[a.n];
  if (i == 0 && a.total) *a.total = total;
  if (i < a.n) {
    const uint64_t at = a.offs[i], size = a.offs[i + 1] - at;
    const uint8_t pre = a.pre[i], v = unpack_final_verdict(pre, at, size, a.out_cap);
    if (a.body_off) a.body_off[i] = at;
    if (a.body_len) a.body_len[i] = unpack_body_len(pre, size, a.nul);
    if (a.reply_types) a.reply_types[i] = unpack_reply_type(v, a.flags);
    if (a.versions) a.versions[i] = a.ver[i];
    if (a.verdict_out) a.verdict_out[i] = v;
  }
  if (a.conn_bytes_first && i <= a.nconn) {
    uint64_t f = i < a.nconn ? a.conn_first[i] : a.n;
    if (f > a.n) f = a.n; // (a CSR that runs past the entries reads as the end)
    a.conn_bytes_first[i] = a.offs[f];
  }
}

dim3 grid_of(uint64_t n, int threads) { return dim3((unsigned)(n ? (n + threads - 1) / threads : 1)); }

} // namespace

hipError_t launch_frames_unpack(const UnpackArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(unpack_size_kernel, grid_of(a.n, 256), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = excl_scan(a.sizes, a.offs, a.n, a.scan_tmp, s)) != hipSuccess) return e;
  if (a.out && a.out_cap && a.n) {
    // (the total is on the device only: the grid covers what out_cap, the stream
    // and n allow, and workgroups past the last tile leave at once)
    uint64_t most = a.out_cap;
    if (!(a.flags & RPC_FRAMES_LIFT_CAP)) most = std::min<uint64_t>(most, a.n * (uint64_t)(kPackMaxBody + 1));
    const uint64_t tiles = pack_tiles(most, 15, kPackTile);
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)std::min<uint64_t>(tiles, kUnpackMaxGrid)), dim3(kUnpackThreads), 0,
                       s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(unpack_finish_kernel, grid_of(std::max(a.n, a.nconn + 1), 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

} // namespace rpccrc
