// rpc_amd/csrc/frames_pack.hip -- device-side frame pack (rpc_frames_pack_device;
// the rules and the piece resolver: frames_pack.h; the tile range, the lane
// walker, the search and the store it shares with the unpack and the carry:
// frames_tile.h).
//
//   size pass -> exclusive scan (the layout) -> [CRC pass over the source
//   bodies, the caller's ragged() call] -> pack kernel -> finish pass
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_tile.h"

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

// One tile's pieces (steps 3 and 4 below), over the readers of the layout and
// of the entries' source offsets.
template <class Off>
__device__ __forceinline__ void pack_tile(const PackArgs &a, const Off off, const Off src_of, const DevEnt &ent, const DevSrc &src,
                                          uint8_t *out0, uint64_t tile, uint32_t mis, uint64_t tile_x1, uint64_t lo0,
                                          uint64_t hi) {
  const auto piece_at = [&](uint32_t k) { return tile * kPackTile + tile_piece(k, kPackThreads); };
  uint64_t lo = lo0;
  tile_walk<kPiecesPerLane>(
      a.bodies, out0, piece_at,
      [&](uint32_t k) {
        const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
        TilePlan p{ps.x0 < ps.x1, {false, 0, 0}};
        if (p.some) {
          const uint64_t e = pack_find(off, lo, hi, ps.x0);
          const uint64_t fo = off(e), fe = off(e + 1);
          lo = e; // (the lane's next piece lies further on)
          if (pack_piece_is_body(fo, fe, ps.x0, ps.x1, ps.b0, a.out_cap))
            p.w = pack_win_plan(src, src_of(e) + (ps.x0 - fo - kPackHeaderLen), 0);
        }
        return p;
      },
      [&](uint32_t k) {
        const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
        uint64_t last;
        store_piece(out0 + piece_at(k), pack_piece(off, ent, src, lo0, hi, ps.x0, ps.x1, ps.b0, a.out_cap, &last));
      });
}

// One workgroup per tile of kPackTile output bytes (striding when the grid is
// smaller); every lane produces kPiecesPerLane aligned 16-byte pieces, a whole
// wave writing 1 KiB of consecutive bytes per round.  Per tile:
//  1. waves 0 and 1 find the entries covering its first and last byte;
//  2. the layout and the source offsets of those entries go to LDS when they fit
//     (steps 1 and 2: tile_range);
//  3. every lane resolves all its pieces; for those that are sixteen body bytes
//     of one frame (pack_piece_is_body: nearly all) it issues the block loads of
//     all of them before it uses any, then shifts and stores;
//  4. the other pieces -- headers, frame edges, stream ends -- go through
//     pack_piece one by one (steps 3 and 4: tile_walk).
__global__ __launch_bounds__(kPackThreads) void pack_kernel(PackArgs a) {
  __shared__ uint64_t s_range[2];
  __shared__ uint64_t s_off[kTileLdsEntries], s_src[kTileLdsEntries];
  const uint64_t total = a.offs[a.n];
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(a.out) & 15u);
  uint8_t *const out0 = a.out - mis; // 16-byte aligned; bytes before a.out are never touched
  // nothing at or beyond out_cap is ever written, so tiles beyond it have no work
  const uint64_t ntiles = pack_tiles(total < a.out_cap ? total : a.out_cap, mis, kPackTile);
  const DevEnt ent{a.src_off, a.src_len, a.crc, a.types, a.versions, a.type, a.version};
  const DevSrc src{a.bodies, a.bodies_bytes};
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const PackSpan ts = pack_span(tile * kPackTile, kPackTile, mis, total); // x0 < x1: the tile holds a byte
    const TileRange r = tile_range<kPackThreads>(a.offs, a.src_off, a.n, ts.x0, ts.x1 - 1, s_range, s_off, s_src);
    if (r.staged)
      pack_tile(a, LdsOff{s_off, r.lo0}, LdsOff{s_src, r.lo0}, ent, src, out0, tile, mis, ts.x1, r.lo0, r.hi);
    else
      pack_tile(a, DevOff{a.offs}, DevOff{a.src_off}, ent, src, out0, tile, mis, ts.x1, r.lo0, r.hi);
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
  if (a.conn_bytes_first && i <= a.nconn)
    a.conn_bytes_first[i] = pack_conn_begin(DevOff{a.offs}, a.conn_first, i, a.nconn, a.n);
}

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
