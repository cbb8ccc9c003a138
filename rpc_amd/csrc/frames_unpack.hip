// rpc_amd/csrc/frames_unpack.hip -- device-side frame unpack
// (rpc_frames_unpack_device; the rules and the piece resolver: frames_unpack.h;
// the tile driver, the tile range, the lane walker, the search and the store:
// frames_tile.h).
//
//   size pass -> exclusive scan (the layout) -> unpack kernel -> finish pass
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_tile.h"
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
// One tile's pieces, over the readers of the layout and of the entries' source
// offsets (tile_walk): the pieces that are sixteen body bytes of one entry
// through the window, the others through unpack_piece.
template <class Off>
__device__ __forceinline__ void unpack_tile(const UnpackArgs &a, const Off off, const Off src_of, const DevSrc &src,
                                            uint8_t *out0, uint64_t tile, uint32_t mis, uint64_t tile_x1, uint64_t lo0,
                                            uint64_t hi) {
  const auto piece_at = [&](uint32_t k) { return tile * kPackTile + tile_piece(k, kUnpackThreads); };
  uint64_t lo = lo0;
  tile_walk<kPiecesPerLane>(
      a.stream, out0, piece_at,
      [&](uint32_t k) {
        const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
        TilePlan p{ps.x0 < ps.x1, {false, 0, 0}};
        if (p.some) {
          const uint64_t e = pack_find(off, lo, hi, ps.x0);
          const uint64_t fo = off(e), fe = off(e + 1);
          lo = e; // (the lane's next piece lies further on)
          if (unpack_piece_is_body(fo, fe, ps.x0, ps.x1, ps.b0, a.nul, a.out_cap))
            p.w = pack_win_plan(src, src_of(e) + (ps.x0 - fo), 0);
        }
        return p;
      },
      [&](uint32_t k) {
        const PackSpan ps = pack_span(piece_at(k), kPackPiece, mis, tile_x1);
        store_piece(out0 + piece_at(k), unpack_piece(off, src_of, src, lo0, hi, ps.x0, ps.x1, ps.b0, a.nul, a.out_cap));
      });
}

// One workgroup per tile of kPackTile output bytes (striding when the grid is
// smaller), as the pack kernel: waves 0 and 1 find the entries covering the
// tile's first and last byte, the layout and the source offsets of those
// entries go to LDS when they fit (tile_range), then every lane produces its
// pieces.
// Five waves per SIMD (96 VGPRs, no scratch) where the compiler settles on four
// (98): interleaved on one box 904 -> 813 us on 1.9M small frames and 403 -> 384
// us on 64 MiB bodies; six (80 VGPRs, 80 bytes of scratch) gave 856 and 450.
__global__ __launch_bounds__(kUnpackThreads) __attribute__((amdgpu_waves_per_eu(5))) void unpack_kernel(UnpackArgs a) {
  __shared__ uint64_t s_range[2];
  __shared__ uint64_t s_off[kTileLdsEntries], s_src[kTileLdsEntries];
  const DevSrc src{a.stream, a.stream_bytes};
  tile_drive<kUnpackThreads>(a.offs, a.src_off, a.n, a.out, a.out_cap, s_range, s_off, s_src,
                             [&](const auto off, const auto src_of, auto... tile) {
                               unpack_tile(a, off, src_of, src, tile...);
                             });
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
  if (a.conn_bytes_first && i <= a.nconn)
    a.conn_bytes_first[i] = pack_conn_begin(DevOff{a.offs}, a.conn_first, i, a.nconn, a.n);
}

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
