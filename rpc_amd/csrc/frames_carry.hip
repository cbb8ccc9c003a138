// rpc_amd/csrc/frames_carry.hip -- device-side frame carry
// (rpc_frames_carry_device; the rule and the piece resolver: frames_carry.h; the
// lane walker, the search and the masked store: frames_tile.h).
//
//   short route: one kernel, a group of lanes per connection
//   long route:  plan pass -> exclusive scan of the chunk counts -> chunk kernel
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_carry.h"
#include "frames_tile.h"

namespace rpccrc {

static_assert(kCarryOk == RPC_CARRY_OK && kCarryClosed == RPC_CARRY_CLOSED && kCarryInvalid == RPC_CARRY_INVALID &&
                  kCarryNoRoom == RPC_CARRY_NO_ROOM && kCarryConnOpen == RPC_CONN_OPEN,
              "frames_carry.h restates the status and state codes");
static_assert(kCarryShortRoom >= RPC_FRAMES_CARRY_ROOM, "an in-cap server takes the short route");
static_assert(RPC_FRAMES_CARRY_ROOM >= kPackHeaderLen + RPC_MAX_BODY_LEN - 1 && RPC_FRAMES_CARRY_ROOM % 16 == 0,
              "the default room holds any tail the scan leaves with the cap in force");

namespace {

constexpr int kCarryThreads = 256;
// Lanes per connection on the short route.  A tail with the cap in force is at
// most 66 pieces and 33 on average: sixteen lanes walk it in one to five steps
// and a wave holds four connections.
constexpr int kCarryGroup = 16;
constexpr uint32_t kPiecesPerLane = kCarryChunk / kPackPiece / kCarryThreads;
static_assert(kPiecesPerLane * kPackPiece * kCarryThreads == kCarryChunk, "a chunk is whole rounds of the workgroup");
constexpr unsigned kCarryMaxGrid = 1u << 18; // workgroups; they stride over the chunks

// The connection's words, then the rule.  Only the state of a closed connection
// is read.
__device__ __forceinline__ CarryPlan plan_of(const CarryArgs &a, uint64_t c) {
  const bool closed = a.conn_state && a.conn_state[c] != kCarryConnOpen;
  uint64_t off = 0, len = 0, consumed = 0, at = 0, nl = 0;
  if (!closed) {
    off = a.conn_off[c];
    len = a.conn_len[c];
    consumed = a.conn_consumed[c];
    at = a.next_at[c];
    if (a.new_len) nl = a.new_len[c];
  }
  return carry_plan_one(closed, off, len, consumed, a.stream_bytes, at, nl, a.next_bytes, a.room);
}

// Adds every lane's `mine` to *carried: one atomic per wave that carried a byte.
// Called by all 64 lanes.
__device__ __forceinline__ void add_carried(uint64_t *carried, uint64_t mine) {
  if (!carried) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += (uint64_t)__shfl_xor((unsigned long long)mine, d, 64);
  if ((threadIdx.x & 63u) == 0 && mine)
    atomicAdd(reinterpret_cast<unsigned long long *>(carried), (unsigned long long)mine);
}

// ---- short route: kCarryGroup lanes per connection ----------------------------
// Every lane of the group reads the connection's words (one address: a
// broadcast) and applies the rule; lane l produces pieces l, l + G, ...; the
// group's first lane writes the next round's connection, after the group's
// reads: next_off / next_len may be conn_off / conn_len.
__global__ __launch_bounds__(kCarryThreads) void carry_short_kernel(CarryArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * kCarryThreads + threadIdx.x;
  const uint64_t c = t / kCarryGroup;
  const uint32_t l = (uint32_t)(t % kCarryGroup);
  uint64_t mine = 0;
  if (c < a.nconn) {
    const CarryPlan p = plan_of(a, c);
    if (p.tail) {
      const DevSrc src{a.stream, a.stream_bytes};
      const uint64_t d = (uint64_t)reinterpret_cast<uintptr_t>(a.next) + p.next_off;
      const uint32_t mis = carry_mis(d, kPackPiece);
      uint8_t *const d0 = reinterpret_cast<uint8_t *>(static_cast<uintptr_t>(d - mis)); // bytes before d are never touched
      const uint64_t pieces = pack_tiles(p.tail, mis, kPackPiece);
      for (uint64_t k = l; k < pieces; k += kCarryGroup) {
        const PackSpan ps = pack_span(k * kPackPiece, kPackPiece, mis, p.tail);
        store_piece(d0 + k * kPackPiece, carry_piece(src, p.src, ps));
      }
    }
    if (l == 0) {
      a.next_off[c] = p.next_off;
      a.next_len[c] = p.next_len;
      if (a.status) a.status[c] = p.status;
      mine = p.tail;
    }
  }
  add_carried(a.carried, mine);
}

// ---- long route ---------------------------------------------------------------
// Plan pass: one lane per connection.  The chunk kernel reads the workspace
// only, so the connection words may be overwritten here.
__global__ __launch_bounds__(256) void carry_plan_kernel(CarryArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t mine = 0;
  if (c < a.nconn) {
    const CarryPlan p = plan_of(a, c);
    a.next_off[c] = p.next_off;
    a.next_len[c] = p.next_len;
    if (a.status) a.status[c] = p.status;
    a.src[c] = p.src;
    a.dst[c] = p.next_off;
    a.tail[c] = p.tail;
    a.cnt[c] = carry_chunks(p.tail, (uint64_t)reinterpret_cast<uintptr_t>(a.next) + p.next_off, kCarryChunk);
    mine = p.tail;
  }
  add_carried(a.carried, mine);
}

// One workgroup per chunk (striding when the grid is smaller): wave 0 finds the
// chunk's connection, then every lane produces its pieces (tile_walk): the whole
// ones through the window, the tail's first and last piece and those whose
// window would leave the stream through carry_piece.
__global__ __launch_bounds__(kCarryThreads) void carry_chunk_kernel(CarryArgs a) {
  __shared__ uint64_t s_conn;
  const uint64_t total = a.offs[a.nconn];
  const DevSrc src{a.stream, a.stream_bytes};
  for (uint64_t ch = blockIdx.x; ch < total; ch += gridDim.x) {
    if (threadIdx.x < 64) {
      const uint64_t e = wave_find(a.offs, a.nconn, ch);
      if (threadIdx.x == 0) s_conn = e;
    }
    __syncthreads();
    const uint64_t c = s_conn;
    const uint64_t s0 = a.src[c], tail = a.tail[c];
    const uint64_t d = (uint64_t)reinterpret_cast<uintptr_t>(a.next) + a.dst[c];
    const uint32_t mis = carry_mis(d, kCarryChunk);
    const uint64_t start = (ch - a.offs[c]) * kCarryChunk; // of the chunk, from the aligned address d - mis
    uint8_t *const d0 = reinterpret_cast<uint8_t *>(static_cast<uintptr_t>(d - mis + start));
    const auto piece_at = [&](uint32_t k) { return tile_piece(k, kCarryThreads); };
    tile_walk<kPiecesPerLane>(
        a.stream, d0, piece_at,
        [&](uint32_t k) {
          const PackSpan ps = pack_span(start + piece_at(k), kPackPiece, mis, tail);
          TilePlan p{ps.x0 < ps.x1, {false, 0, 0}};
          if (p.some && carry_piece_is_whole(ps)) p.w = pack_win_plan(src, s0 + ps.x0, 0);
          return p;
        },
        [&](uint32_t k) {
          const PackSpan ps = pack_span(start + piece_at(k), kPackPiece, mis, tail);
          store_piece(d0 + piece_at(k), carry_piece(src, s0, ps));
        });
    __syncthreads(); // s_conn is rewritten for the next chunk
  }
}

} // namespace

hipError_t launch_frames_carry_short(const CarryArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(carry_short_kernel, grid_of(a.nconn * kCarryGroup, kCarryThreads), dim3(kCarryThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_frames_carry_long(const CarryArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(carry_plan_kernel, grid_of(a.nconn, 256), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = excl_scan(a.cnt, a.offs, a.nconn, a.scan_tmp, s)) != hipSuccess) return e;
  // (the chunk count is on the device only: the grid covers what room and the
  // stream allow -- a tail of t bytes is at most t / chunk + 2 chunks -- and
  // workgroups past the last chunk leave at once; connections that overlap in
  // the stream can exceed the second bound, and then the workgroups stride)
  const uint64_t per_conn = a.room / kCarryChunk + 2;
  uint64_t most = a.nconn > kCarryMaxGrid / per_conn ? kCarryMaxGrid : a.nconn * per_conn;
  most = std::min<uint64_t>(most, a.stream_bytes / kCarryChunk + 2 * a.nconn);
  if (a.stream_bytes == 0) return hipSuccess; // every tail is empty
  hipLaunchKernelGGL(carry_chunk_kernel, dim3((unsigned)std::min<uint64_t>(most, kCarryMaxGrid)), dim3(kCarryThreads),
                     0, s, a);
  return hipGetLastError();
}

} // namespace rpccrc
