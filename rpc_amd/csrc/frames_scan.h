// rpc_amd/csrc/frames_scan.h -- the frame walk: find the frames in raw
// connection bytes (rpc_frames_scan_device).
//
// A connection is a byte run of the stream.  Its frames are defined by the walk
// of scan_walk(): read the 12-byte header at p (type and body_len only), apply
// the reference's stop rules (rpc_server_main.c:189-195 over-cap header,
// rpc_async.c:330-349 empty non-PONG frame at a client), jump 12 + body_len.
// A trailing partial frame is not emitted and not consumed.
//
// Two routes give the same result:
//  * serial: one lane per connection walks its headers from global memory;
//  * tiled:  a long connection is cut into tiles of kScanTile bytes.  With the
//    MAX_BODY_LEN cap in force a chain can enter a tile only at one of
//    kScanEntries = 12 + 1024 offsets, so each tile's "entry -> exit into the
//    next tile" map is computed for every entry at once, the maps are composed
//    kScanGroup at a time level by level (up-sweep), and the true entry of every
//    tile is resolved back down (down-sweep).  Each tile then walks only its
//    true chain.  With RPC_FRAMES_LIFT_CAP an exit can land anywhere, so those
//    calls always take the serial route.
//
// Everything in this first part is plain inline code shared by the kernels
// (frames_scan.hip) and the CPU emulator (tests/cpu_emu/scan_emu.cpp), which
// instantiates it with small tiles and groups as well.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "excl_scan.h"
#define SCAN_HD __host__ __device__ __forceinline__
#else
#define SCAN_HD inline
#endif

namespace rpccrc {

constexpr uint32_t kScanHeaderLen = 12;                         // RPC_HEADER_LEN, rpc.h:15
constexpr uint32_t kScanMaxBody = 1024;                         // MAX_BODY_LEN, rpc.h:17
constexpr uint32_t kScanEntries = kScanHeaderLen + kScanMaxBody; // E: entry offsets of a tile, cap in force
constexpr uint32_t kScanStop = kScanEntries;                    // map value / index: the chain has stopped
constexpr uint32_t kScanMapLen = kScanEntries + 1;              // uint16 words of one map
constexpr uint32_t kScanHalo = 7;                               // header bytes 2..7 past the tile's last byte
// The kernels' instantiation.
constexpr uint32_t kScanTile = 32768;   // T: bytes per tile
constexpr uint32_t kScanGroup = 8;      // G: maps composed into one per up-sweep level
constexpr uint32_t kScanMaxLevels = 4;  // up-sweep levels: at most G^(levels + 1) tiles (1 GiB) are tiled per call
// AUTO: connections longer than this take the tiled route.  Measured
// (tools/scan_bench.py --sweep, one connection): at 64 KiB the
// serial walk takes 83 us against 91 us tiled, at 128 KiB 168 us against 111 us;
// the lines cross near 73 KiB.  The constant is the midpoint of the two
// bracketing runs, 96 KiB (three tiles).
constexpr uint64_t kScanTiledMin = 98304;
static_assert(kScanTile >= kScanEntries, "an exit must land inside the next tile");
static_assert(kScanMapLen <= 0xFFFF, "maps are uint16");

// Flag bits and type codes as include/rpccrc.h has them (the emulator builds
// without that header's HIP surroundings).
constexpr int kScanServer = 0x1, kScanClient = 0x2, kScanLiftCap = 0x4;
constexpr uint32_t kScanTypePing = 1, kScanTypePong = 2;

enum : uint32_t { kStepFrame = 0, kStepStop = 1, kStepClose = 2 };
struct ScanStep {
  uint32_t kind; // kStepFrame: emit and go on; kStepStop: not here yet; kStepClose: emit, the connection is closed
  uint64_t adv;
};

// One header.  rd(q) is byte q of the connection; only bytes p+2 .. p+7 are read,
// and only when the whole header lies inside the connection.  0 <= p <= len.
template <class Rd>
SCAN_HD ScanStep scan_step(const Rd &rd, uint64_t p, uint64_t len, int flags) {
  if (len - p < kScanHeaderLen) return ScanStep{kStepStop, 0}; // clean end or partial header
  const uint32_t type = ((uint32_t)rd(p + 2) << 8) | (uint32_t)rd(p + 3);
  const uint32_t bl = ((uint32_t)rd(p + 4) << 24) | ((uint32_t)rd(p + 5) << 16) | ((uint32_t)rd(p + 6) << 8) |
                      (uint32_t)rd(p + 7);
  if ((type == kScanTypePing && (flags & kScanServer)) || (type == kScanTypePong && (flags & kScanClient)))
    return ScanStep{kStepFrame, kScanHeaderLen};
  if (bl > kScanMaxBody && !(flags & kScanLiftCap)) return ScanStep{kStepClose, kScanHeaderLen};
  if (bl == 0 && (flags & kScanClient)) return ScanStep{kStepClose, kScanHeaderLen};
  if (len - (p + kScanHeaderLen) < bl) return ScanStep{kStepStop, 0}; // partial body
  return ScanStep{kStepFrame, (uint64_t)kScanHeaderLen + bl};
}

// What a walk leaves behind.
struct ScanWalk {
  uint64_t count;   // frames emitted
  uint64_t p;       // where the walk stands: the stop position, or >= limit
  uint32_t stopped; // 1: the walk met the connection's stop here (p is `consumed`)
  uint32_t closed;  // with stopped: RPC_CONN_CLOSED
};
struct ScanNoSink {
  SCAN_HD void operator()(uint64_t, uint64_t) const {}
};
// Walks the chain from p while p < limit; sink(k, q) takes the k-th frame of
// this walk, at connection offset q.  The serial route is the walk from 0 with
// no limit; a tile is the walk from its true entry to its end.
template <class Rd, class Sink>
SCAN_HD ScanWalk scan_walk(const Rd &rd, uint64_t p, uint64_t limit, uint64_t len, int flags, const Sink &sink) {
  ScanWalk w{0, p, 0, 0};
  while (w.p < limit) {
    const ScanStep st = scan_step(rd, w.p, len, flags);
    if (st.kind == kStepStop) {
      w.stopped = 1;
      return w;
    }
    sink(w.count, w.p);
    w.count += 1;
    w.p += st.adv;
    if (st.kind == kStepClose) {
      w.stopped = 1;
      w.closed = 1;
      return w;
    }
  }
  return w;
}

// ---- tiled route -----------------------------------------------------------
// A connection of len bytes has len / T + 1 tiles: the last one (possibly
// empty) is where every chain meets the end of the connection.
template <uint32_t T>
SCAN_HD uint64_t scan_tiles_of(uint64_t len) {
  return len / T + 1;
}

// Tile pass: the exit of the chain that enters the tile starting at `t0` at
// offset e.  The value is the offset in the next tile where the chain leaves
// (< kScanEntries with the cap in force) or kScanStop: the chain met a closing
// header, a partial frame or the connection's end inside this tile.
template <uint32_t T, class Rd>
SCAN_HD uint16_t scan_tile_exit(const Rd &rd, uint64_t t0, uint32_t e, uint64_t len, int flags) {
  if (t0 + e > len) return (uint16_t)kScanStop; // no chain can stand past the end
  const ScanWalk w = scan_walk(rd, t0 + e, t0 + T, len, flags, ScanNoSink{});
  if (w.stopped) return (uint16_t)kScanStop;
  const uint64_t x = w.p - (t0 + T);
  return (uint16_t)(x < kScanEntries ? x : kScanStop); // (x >= E cannot happen with the cap in force)
}
// A map is kScanMapLen uint16 words: m[e] for the entries, and m[kScanStop] for
// a chain that has already stopped.  An ordinary tile has m[kScanStop] =
// kScanStop.  The FIRST tile of a connection is entered at 0 whatever came
// before it, so its map is constant: every word, m[kScanStop] included, is the
// exit of the chain from 0.  With that the tiles of all tiled connections form
// one sequence, and composing maps across a connection boundary is right
// without a special case: compose is m_b[m_a[e]].

// Up-sweep: the composition of `count` consecutive maps (kScanMapLen apart), at entry e.
SCAN_HD uint16_t scan_compose(const uint16_t *maps, uint32_t count, uint32_t e) {
  uint32_t v = e;
  for (uint32_t i = 0; i < count; ++i) v = maps[(uint64_t)i * kScanMapLen + v];
  return (uint16_t)v;
}
// Maps at level l (level 0: the tiles) when the live tiles are nt.
template <uint32_t G>
SCAN_HD uint64_t scan_level_count(uint64_t nt, uint32_t level) {
  for (uint32_t i = 0; i < level; ++i) nt = (nt + G - 1) / G;
  return nt;
}
// Down-sweep: one group.  `e` is the group's entry (the parent's resolved
// entry); writes the entry of each of the group's `count` maps.
SCAN_HD void scan_resolve(const uint16_t *maps, uint32_t count, uint32_t e, uint16_t *entry) {
  for (uint32_t i = 0; i < count; ++i) {
    entry[i] = (uint16_t)e;
    e = maps[(uint64_t)i * kScanMapLen + e];
  }
}
// The connection of tile j: tbase is the exclusive scan of the connections'
// tile counts (nconn + 1 words, 0 tiles for a connection on the serial route):
// the c with tbase[c] <= j < tbase[c + 1].  j < tbase[nconn].
SCAN_HD uint64_t scan_find_conn(const uint64_t *tbase, uint64_t nconn, uint64_t j) {
  uint64_t lo = 0, hi = nconn; // first index i in [0, nconn] with tbase[i] > j
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (tbase[mid] > j)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo - 1;
}

// ---- the call (frames_scan.hip) ---------------------------------------------
struct ScanArgs {
  const uint8_t *stream = nullptr;
  uint64_t stream_bytes = 0;
  const uint64_t *conn_off = nullptr;
  const uint64_t *conn_len = nullptr;
  uint64_t nconn = 0;
  int flags = 0;
  // outputs (the caller's)
  uint64_t *frame_off = nullptr; // may be nullptr (count only)
  uint32_t *frame_conn = nullptr; // may be nullptr
  uint64_t frame_cap = 0;
  uint64_t *conn_first = nullptr; // nconn + 1
  uint64_t *consumed = nullptr;
  uint8_t *state = nullptr;
  uint64_t *nframes = nullptr;
  // workspace, every route
  uint64_t *conn_cnt = nullptr; // nconn: frames per connection
  uint64_t *scan_tmp = nullptr; // scan_tmp_words(max(nconn, tile_cap))
  // workspace, tiled route (tile_cap == 0: every connection walks serially)
  uint64_t tile_cap = 0;        // tiles the workspace holds; a connection whose tiles do not fit walks serially
  uint64_t tiled_min = 0;       // connections longer than this are tiled
  int levels = 0;               // down-sweep levels L: ceil(tile_cap / G^L) == 1; up-sweep builds levels 1 .. L-1
  uint64_t *conn_tiles = nullptr; // nconn: tiles wanted (0: serial)
  uint64_t *tbase = nullptr;      // nconn + 1
  uint64_t *nt_live = nullptr;    // 1 word: tiles in use (the tiled connections are a prefix of those that want tiles)
  uint32_t *tconn = nullptr;      // tile_cap: the tile's connection
  uint64_t *tile_cnt = nullptr;   // tile_cap
  uint64_t *tpre = nullptr;       // tile_cap + 1
  uint16_t *maps[kScanMaxLevels + 1] = {};  // level l: ceil(tile_cap / G^l) maps
  uint16_t *entry[kScanMaxLevels + 2] = {}; // level l: as many resolved entries
};
// The tiled route's arrays in pool workspace, over a WsLayout (workspace.h) or
// anything with its take<T>(count); a.nconn, a.tile_cap and a.levels are set.
template <class Layout> inline void scan_tiled_ws_layout(Layout &w, ScanArgs &a) {
  a.conn_tiles = w.template take<uint64_t>(a.nconn);
  a.tbase = w.template take<uint64_t>(a.nconn + 1);
  a.nt_live = w.template take<uint64_t>(32); // (a 256-byte line of its own)
  a.tconn = w.template take<uint32_t>(a.tile_cap);
  a.tile_cnt = w.template take<uint64_t>(a.tile_cap);
  a.tpre = w.template take<uint64_t>(a.tile_cap + 1);
  for (int l = 0; l < a.levels; ++l) {
    const uint64_t nl = scan_level_count<kScanGroup>(a.tile_cap, (uint32_t)l);
    a.maps[l] = w.template take<uint16_t>(nl * kScanMapLen);
    a.entry[l] = w.template take<uint16_t>(nl);
  }
}
// Every route's arrays; a.nconn and a.frame_cap are set.  reach: the fused
// call's first_close (nconn; the reach pass's, no field of `a`); own_conn: the
// reach pass's frame_conn where the caller gave none.
template <class Layout>
inline void scan_ws_layout(Layout &w, ScanArgs &a, size_t tmp_words, bool reach, bool own_conn, uint64_t *&first_close) {
  a.conn_cnt = w.template take<uint64_t>(a.nconn);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
  if (reach) first_close = w.template take<uint64_t>(a.nconn);
  if (own_conn) a.frame_conn = w.template take<uint32_t>(a.frame_cap);
}

#if defined(__HIPCC__)
// (scan_tmp_words(n), the words of scan_tmp a scan over n words needs: excl_scan.h)
// Levels L for a workspace of tile_cap tiles (see ScanArgs::levels).
int scan_levels_for(uint64_t tile_cap);
// Enqueues the whole scan on s.
hipError_t launch_frames_scan(const ScanArgs &a, hipStream_t s);
// The fused call's reach pass, after verify has written verdict / crc for
// frame_cap entries: frames behind a connection's first closing verdict
// (BAD_CRC, TOO_LARGE, RECV_ERR) become RPC_FRAME_NOT_REACHED with crc 0, and a
// connection closed by a BAD_CRC becomes RPC_CONN_CLOSED.  first_close: nconn words.
hipError_t launch_frames_reach(const uint32_t *frame_conn, uint64_t frame_cap, const uint64_t *nframes, uint64_t nconn,
                               uint64_t *first_close, uint8_t *verdict, uint32_t *crc, uint8_t *state, hipStream_t s);
#endif

} // namespace rpccrc
