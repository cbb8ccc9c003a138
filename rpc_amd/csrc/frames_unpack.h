// rpc_amd/csrc/frames_unpack.h -- the frame unpack: verified bodies as C strings
// and the reply plan (rpc_frames_unpack_device).  What sits
// between the fused scan + verify and the dispatcher, and what feeds the pack.
//
// Entry i is a verdict and a frame offset into the raw stream.
// unpack_size_one() applies rules 1-5 of include/rpccrc.h: how many bytes of
// the output the entry takes (0, or body_len + nul), where its body starts in
// the stream, the header's version and the provisional verdict; the exclusive
// scan of the sizes is the layout.  The output is produced destination-centric
// with the pack's machinery (frames_pack.h: tiles aligned to the output's
// address, whole aligned 16-byte pieces, two aligned source blocks and the byte
// funnel); unpack_piece() resolves one piece.  An entry here is its body bytes
// and then, with nul, one 0 byte -- no header -- so sizes can be 1 and a piece
// can touch 16 entries where the pack's touches three.
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_unpack.hip) and the CPU emulator (tests/cpu_emu/unpack_emu.cpp).
#pragma once
#include "frames_pack.h"

namespace rpccrc {

constexpr int kUnpackServer = 0x1, kUnpackClient = 0x2; // RPC_FRAMES_SERVER / _CLIENT
constexpr uint32_t kUnpackTypeData = 0;                 // RPC_FRAME_TYPE_DATA

// ---- sizing rule -----------------------------------------------------------
struct UnpackSize {
  uint64_t size;    // bytes of the output: 0, or body_len + nul
  uint64_t src;     // stream offset of the body (0 when nothing is delivered)
  uint16_t version; // the header's, 0 when the header is not read or contradicts the verdict
  uint8_t verdict;  // provisional: the capacity check comes with the layout (unpack_final_verdict)
};
// The heartbeat that is a control frame in this role.
PACK_HD uint32_t unpack_ctl(int flags) { return (flags & kUnpackServer) ? kPackTypePing : kPackTypePong; }
// Rules 1-5, in that order.  Hdr: uint8_t byte(uint64_t p), a stream byte; it
// is asked only for the 12 header bytes, and only when they lie inside the
// stream.  off: looked at by the caller only when v is OK or CONTROL (pass
// anything otherwise).
template <class Hdr>
PACK_HD UnpackSize unpack_size_one(const Hdr &hdr, uint8_t v, uint64_t off, uint64_t stream_bytes, int flags, int nul) {
  if (v != kPackOk && v != kPackControl) return UnpackSize{0, 0, 0, v};
  const UnpackSize bad{0, 0, 0, kPackMalformed};
  if (!(off <= stream_bytes && kPackHeaderLen <= stream_bytes - off)) return bad;
  uint32_t b[8]; // version, type, body_len: big-endian as rpc_server_main.c:165-169
  PACK_UNROLL
  for (uint32_t i = 0; i < 8; ++i) b[i] = hdr.byte(off + i);
  const uint16_t version = (uint16_t)((b[0] << 8) | b[1]);
  const uint32_t type = (b[2] << 8) | b[3];
  const uint32_t len = (b[4] << 24) | (b[5] << 16) | (b[6] << 8) | b[7];
  const uint32_t ctl = unpack_ctl(flags);
  if (v == kPackControl) return type == ctl ? UnpackSize{0, 0, version, kPackControl} : bad;
  if (type == ctl) return bad;
  if (len > kPackMaxBody && !(flags & kPackLiftCap)) return bad;
  if (len == 0 && (flags & kUnpackClient)) return bad; // rpc_async.c:330-349: never delivered
  if (len > stream_bytes - off - kPackHeaderLen) return bad;
  return UnpackSize{(uint64_t)len + (uint64_t)nul, off + kPackHeaderLen, version, kPackOk};
}
PACK_HD uint8_t unpack_final_verdict(uint8_t v, uint64_t at, uint64_t size, uint64_t out_cap) {
  return pack_final_verdict(v, at, size, out_cap);
}
// The pack's `types` entry for a final verdict: OK -> DATA, CONTROL -> PONG at a
// server and nothing at a client (which consumes a PONG, rpc_async.c:303-309),
// everything else -> NONE.
PACK_HD uint16_t unpack_reply_type(uint8_t final_verdict, int flags) {
  if (final_verdict == kPackOk) return (uint16_t)kUnpackTypeData;
  if (final_verdict == kPackControl && (flags & kUnpackServer)) return (uint16_t)kPackTypePong;
  return (uint16_t)kPackTypeNone;
}
// The body length of an entry of `size` bytes with provisional verdict v.
PACK_HD uint32_t unpack_body_len(uint8_t v, uint64_t size, int nul) {
  return v == kPackOk ? (uint32_t)(size - (uint64_t)nul) : 0u;
}

// ---- the piece resolver ----------------------------------------------------
// The entry behind e that covers x = off(e + 1) < total: mostly e + 1 itself
// (one probe), else the search, which skips the zero-size entries.
template <class Off>
PACK_HD uint64_t unpack_next(const Off &off, uint64_t e, uint64_t hi, uint64_t x) {
  if (e + 1 >= hi || off(e + 2) > x) return e + 1;
  return pack_find(off, e + 2, hi, x);
}
// Is the piece [x0, x1) at piece byte b0 sixteen body bytes of the one written
// entry [fo, fe)?  (The entry's last byte is its NUL when nul is set.)
PACK_HD bool unpack_piece_is_body(uint64_t fo, uint64_t fe, uint64_t x0, uint64_t x1, uint32_t b0, int nul,
                                  uint64_t out_cap) {
  return b0 == 0 && x1 - x0 == kPackPiece && x0 >= fo && x1 + (uint64_t)nul <= fe && fe <= out_cap;
}
// One 16-byte piece (PackPiece: the words and the bytes to store).  A byte is
// stored iff it belongs to an entry that is written.  SrcOf: uint64_t
// operator()(e), the stream offset of entry e's body; Src as in frames_pack.h.
// The piece holds output bytes [x0, x1) at piece bytes b0 .., x1 - x0 <= 16 - b0,
// x0 < x1 <= total.  [lo, hi]: entries that can cover it (off(lo) <= x0, and the
// entry that covers x1 - 1 is <= hi).
template <class Off, class SrcOf, class Src>
PACK_HD PackPiece unpack_piece(const Off &off, const SrcOf &src_of, const Src &src, uint64_t lo, uint64_t hi,
                               uint64_t x0, uint64_t x1, uint32_t b0, int nul, uint64_t out_cap) {
  PackPiece p{{0, 0, 0, 0}, 0};
  uint64_t x = x0;
  uint32_t b = b0;
  uint64_t e = pack_find(off, lo, hi, x); // the last entry with offset <= x covers x (see pack_find)
  for (;;) {
    const uint64_t fo = off(e), fe = off(e + 1);
    const uint32_t cnt = (uint32_t)((fe < x1 ? fe : x1) - x); // >= 1: fe > x
    if (fe <= out_cap) { // the entry is written
      const uint64_t at = x - fo, len = fe - fo - (uint64_t)nul;
      if (at < len) { // body bytes; what is left of cnt is the NUL, and p.w is 0 there
        const uint32_t bc = len - at < cnt ? (uint32_t)(len - at) : cnt;
        const uint64_t s = src_of(e) + at;
        uint32_t win[4];
        if (pack_window(src, s, b, win)) {
          PACK_UNROLL
          for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t m = pack_range_mask(j, b, b + bc);
            p.w[j] = (p.w[j] & ~m) | (win[j] & m);
          }
        } else { // a window that would leave the stream: bytewise
          for (uint32_t i = 0; i < bc; ++i) {
            const uint32_t pos = b + i, sh = 8 * (pos & 3), v = src.byte(s + i);
            PACK_UNROLL
            for (uint32_t j = 0; j < 4; ++j)
              if ((pos >> 2) == j) p.w[j] = (p.w[j] & ~(0xFFu << sh)) | (v << sh);
          }
        }
      }
      p.mask |= ((1u << cnt) - 1u) << b;
    }
    x += cnt;
    b += cnt;
    if (x >= x1) break;
    e = unpack_next(off, e, hi, x);
  }
  return p;
}

// ---- the call (frames_unpack.hip) -------------------------------------------
struct UnpackArgs {
  const uint8_t *stream = nullptr;
  uint64_t stream_bytes = 0;
  const uint64_t *frame_off = nullptr;
  const uint8_t *verdict_in = nullptr;
  uint64_t n = 0;
  const uint64_t *conn_first = nullptr; // nconn + 1, or nullptr
  uint64_t nconn = 0;
  int flags = 0, nul = 0;
  // outputs (the caller's; all but out optional)
  uint8_t *out = nullptr;
  uint64_t out_cap = 0;
  uint64_t *body_off = nullptr;
  uint32_t *body_len = nullptr;
  uint16_t *reply_types = nullptr, *versions = nullptr;
  uint8_t *verdict_out = nullptr; // may be verdict_in
  uint64_t *conn_bytes_first = nullptr;
  uint64_t *total = nullptr;
  // workspace
  uint64_t *sizes = nullptr;    // n
  uint64_t *offs = nullptr;     // n + 1: the layout
  uint64_t *src_off = nullptr;  // n: where each delivered body starts in the stream
  uint16_t *ver = nullptr;      // n
  uint8_t *pre = nullptr;       // n: provisional verdicts
  uint64_t *scan_tmp = nullptr; // scan_tmp_words(n)
};
// Its arrays in pool workspace (as pack_ws_layout); a.n is set.
template <class Layout> inline void unpack_ws_layout(Layout &w, UnpackArgs &a, size_t tmp_words) {
  a.sizes = w.template take<uint64_t>(a.n);
  a.src_off = w.template take<uint64_t>(a.n);
  a.offs = w.template take<uint64_t>(a.n + 1);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
  a.ver = w.template take<uint16_t>(a.n);
  a.pre = w.template take<uint8_t>(a.n);
}

#if defined(__HIPCC__)
// Size pass, exclusive scan, unpack kernel (when a.out is set), finish pass.
hipError_t launch_frames_unpack(const UnpackArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
