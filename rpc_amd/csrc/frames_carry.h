// rpc_amd/csrc/frames_carry.h -- the frame carry: partial frames join the next
// read (rpc_frames_carry_device).  What sits between two rounds
// of scan -> unpack -> handlers -> pack.
//
// Connection c's tail is stream bytes [off + consumed, off + len): the start of a
// frame whose rest the next recv() brings.  carry_plan_one() applies rules 1-4 of
// include/rpccrc.h: whether the tail is carried, from where to where, and the
// next round's connection.  A tail is produced destination-centric with the
// pack's machinery (frames_pack.h: whole 16-byte pieces aligned to the
// destination's address, two aligned source blocks and the byte funnel);
// carry_piece() resolves one piece.  The first and last piece of a tail are
// partial and go out under their byte mask: the byte behind a tail may be in
// flight from another copy, so nothing is read and written back.  On the long
// route a tail is dealt out in chunks aligned to the destination's address
// (carry_chunks), and a chunk finds its connection by search in the exclusive
// scan of the chunk counts (pack_find and its wave-wide form).
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_carry.hip) and the CPU emulator (tests/cpu_emu/carry_emu.cpp).
#pragma once
#include "frames_pack.h"

namespace rpccrc {

constexpr uint8_t kCarryOk = 0, kCarryClosed = 1, kCarryInvalid = 2, kCarryNoRoom = 3; // RPC_CARRY_*
constexpr uint8_t kCarryConnOpen = 0;                                                   // RPC_CONN_OPEN
// Destination bytes per chunk of the long route: 256 lanes x 4 pieces, as a pack tile.
constexpr uint32_t kCarryChunk = 16384;
// `room` up to which one launch does everything (a group of lanes per
// connection walks the whole tail): 4 x RPC_FRAMES_CARRY_ROOM, rounded.
constexpr uint64_t kCarryShortRoom = 4096;
static_assert(kCarryChunk % kPackPiece == 0 && (kCarryChunk & (kCarryChunk - 1)) == 0,
              "a chunk is whole pieces, and a power of two");

// ---- the rule ----------------------------------------------------------------
struct CarryPlan {
  uint64_t src;  // stream offset of the tail's first byte
  uint64_t tail; // bytes to copy: 0 unless status is OK
  uint64_t next_off, next_len; // the next round's connection; next_off is where the tail goes
  uint8_t status;
};
// Rules 1-4, in that order.  closed: d_conn_state is given and says so; then
// nothing else is looked at (pass anything).
PACK_HD CarryPlan carry_plan_one(bool closed, uint64_t off, uint64_t len, uint64_t consumed, uint64_t stream_bytes,
                                 uint64_t at, uint64_t nl, uint64_t next_bytes, uint64_t room) {
  if (closed) return CarryPlan{0, 0, 0, 0, kCarryClosed};
  if (!(off <= stream_bytes && len <= stream_bytes - off) || consumed > len) return CarryPlan{0, 0, 0, 0, kCarryInvalid};
  const uint64_t tail = len - consumed;
  if (tail > room || tail > at || at > next_bytes || nl > next_bytes - at) return CarryPlan{0, 0, 0, 0, kCarryNoRoom};
  return CarryPlan{off + consumed, tail, at - tail, tail + nl, kCarryOk};
}

// ---- pieces and chunks -------------------------------------------------------
// A tail of `tail` bytes whose first byte goes to address d is cut at the
// multiples of `unit` (16 for pieces, the chunk size for chunks; a power of two):
// with mis = carry_mis(d, unit), unit number u covers tail bytes
// pack_span(u * unit, unit, mis, tail), and pack_tiles(tail, mis, unit) units hold
// a byte.
PACK_HD uint32_t carry_mis(uint64_t d, uint32_t unit) { return (uint32_t)(d & (uint64_t)(unit - 1)); }
PACK_HD uint64_t carry_chunks(uint64_t tail, uint64_t d, uint32_t chunk) {
  return pack_tiles(tail, carry_mis(d, chunk), chunk);
}
// Is the piece sixteen tail bytes?  Then it is pack_win_plan(src, s0 + ps.x0, 0),
// two block loads, pack_win_select and one 16-byte store.
PACK_HD bool carry_piece_is_whole(const PackSpan &ps) { return ps.b0 == 0 && ps.x1 - ps.x0 == kPackPiece; }
// One 16-byte piece (PackPiece: the words and the bytes to store) holding tail
// bytes [ps.x0, ps.x1) at piece bytes ps.b0 ..; s0: the stream offset of the
// tail's first byte; Src as in frames_pack.h.  A window that would leave the
// stream goes bytewise.
template <class Src>
PACK_HD PackPiece carry_piece(const Src &src, uint64_t s0, const PackSpan &ps) {
  PackPiece p{{0, 0, 0, 0}, 0};
  if (ps.x0 >= ps.x1) return p;
  const uint32_t cnt = (uint32_t)(ps.x1 - ps.x0); // 1 .. 16 - b0
  const uint64_t s = s0 + ps.x0;
  if (!pack_window(src, s, ps.b0, p.w)) {
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint32_t pos = ps.b0 + i, sh = 8 * (pos & 3), v = src.byte(s + i);
      PACK_UNROLL
      for (uint32_t j = 0; j < 4; ++j)
        if ((pos >> 2) == j) p.w[j] |= v << sh;
    }
  }
  p.mask = ((1u << cnt) - 1u) << ps.b0;
  return p;
}

// ---- the call (frames_carry.hip) ---------------------------------------------
struct CarryArgs {
  const uint8_t *stream = nullptr;
  uint64_t stream_bytes = 0;
  const uint64_t *conn_off = nullptr, *conn_len = nullptr, *conn_consumed = nullptr;
  const uint8_t *conn_state = nullptr; // or nullptr: every connection is open
  uint64_t nconn = 0;
  uint8_t *next = nullptr;
  uint64_t next_bytes = 0;
  const uint64_t *next_at = nullptr;
  uint64_t room = 0;
  const uint64_t *new_len = nullptr; // or nullptr: 0 everywhere
  // outputs (the caller's; status and carried optional, *carried zeroed by the caller)
  uint64_t *next_off = nullptr, *next_len = nullptr; // may be conn_off / conn_len
  uint8_t *status = nullptr;
  uint64_t *carried = nullptr;
  // workspace (long route only)
  uint64_t *cnt = nullptr;      // nconn: chunks per connection
  uint64_t *offs = nullptr;     // nconn + 1: their exclusive scan
  uint64_t *src = nullptr;      // nconn: CarryPlan.src
  uint64_t *dst = nullptr;      // nconn: CarryPlan.next_off
  uint64_t *tail = nullptr;     // nconn: CarryPlan.tail
  uint64_t *scan_tmp = nullptr; // scan_tmp_words(nconn)
};
// The long route's arrays in pool workspace (as pack_ws_layout); a.nconn is set.
template <class Layout> inline void carry_ws_layout(Layout &w, CarryArgs &a, size_t tmp_words) {
  a.cnt = w.template take<uint64_t>(a.nconn);
  a.offs = w.template take<uint64_t>(a.nconn + 1);
  a.src = w.template take<uint64_t>(a.nconn);
  a.dst = w.template take<uint64_t>(a.nconn);
  a.tail = w.template take<uint64_t>(a.nconn);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
}

#if defined(__HIPCC__)
// One launch: rule, copy, next round's connections (room <= kCarryShortRoom).
hipError_t launch_frames_carry_short(const CarryArgs &a, hipStream_t s);
// Plan pass, exclusive scan, chunk kernel.
hipError_t launch_frames_carry_long(const CarryArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
