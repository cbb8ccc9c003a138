// rpc_amd/csrc/frames_pack.h -- the frame pack: build wire streams from bodies
// (rpc_frames_pack_device).  The mirror image of the scan.
//
// Entry i is a type, a version and a body [off, off + len) of the source
// buffer.  pack_size_one() says how many bytes of the output it takes (0, 12 or
// 12 + len) and with which verdict; the exclusive scan of the sizes is the
// layout.  The output is then produced destination-centric: it is dealt out in
// tiles of kPackTile bytes, each lane produces whole aligned 16-byte pieces of
// it, and pack_piece() resolves one piece: which entries cover it (at most
// three: a 1-byte body tail, a whole 12-byte heartbeat, 3 bytes of the next
// header), which of its bytes are header and which body, and at which source
// byte the body bytes start.  Body bytes come through aligned 16-byte source
// blocks and a byte funnel shift, or bytewise where an aligned block would
// leave the source buffer.
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_pack.hip) and the CPU emulator (tests/cpu_emu/pack_emu.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PACK_HD __host__ __device__ __forceinline__
#define PACK_UNROLL _Pragma("unroll")
#else
#define PACK_HD inline
#define PACK_UNROLL
#endif

namespace rpccrc {

constexpr uint32_t kPackHeaderLen = 12; // RPC_HEADER_LEN, rpc.h:15
constexpr uint32_t kPackMaxBody = 1024; // MAX_BODY_LEN, rpc.h:17
constexpr uint32_t kPackPiece = 16;     // bytes a lane produces with one store
// Output bytes per tile: 256 lanes x 4 pieces.  One entry search per tile side
// (4 dependent loads each, wave-wide) is paid per 16 KiB written.
constexpr uint32_t kPackTile = 16384;
static_assert(kPackTile % kPackPiece == 0, "a tile is whole pieces");

// Type codes, the flag bit and the verdicts as include/rpccrc.h has them (the
// emulator builds without that header's HIP surroundings).
constexpr uint32_t kPackTypePing = 1, kPackTypePong = 2, kPackTypeNone = 0xFFFF;
constexpr int kPackLiftCap = 0x4;
constexpr uint8_t kPackOk = 1, kPackControl = 2, kPackTooLarge = 3, kPackMalformed = 4, kPackSkipped = 7;

// ---- sizing rule -----------------------------------------------------------
// Only a data entry's offset and length are looked at.
PACK_HD bool pack_is_data(uint32_t type) {
  return type != kPackTypeNone && type != kPackTypePing && type != kPackTypePong;
}
struct PackSize {
  uint64_t size;   // bytes of the output: 0, 12 or 12 + len
  uint64_t off;    // the body the CRC pass reads: an in-range empty one for everything that is no data frame
  uint32_t len;
  uint8_t verdict; // provisional: the capacity check comes with the layout (pack_final_verdict)
};
// Rules 1-5 of include/rpccrc.h, in that order.  off / len: the entry's, or
// anything when !pack_is_data(type).
PACK_HD PackSize pack_size_one(uint32_t type, uint64_t off, uint32_t len, uint64_t bodies_bytes, int flags) {
  if (type == kPackTypeNone) return PackSize{0, 0, 0, kPackSkipped};
  if (type == kPackTypePing || type == kPackTypePong) // conn_pool.c:248-257, rpc_server_main.c:172-187
    return PackSize{kPackHeaderLen, 0, 0, kPackControl};
  if (!(off <= bodies_bytes && len <= bodies_bytes - off)) return PackSize{0, 0, 0, kPackMalformed};
  if (len > kPackMaxBody && !(flags & kPackLiftCap)) return PackSize{0, 0, 0, kPackTooLarge}; // rpc_async.c:499-501
  return PackSize{(uint64_t)kPackHeaderLen + len, off, len, kPackOk};
}
// An entry of `size` bytes at output offset `at` that does not end inside
// out_cap is not written, not even in part.
PACK_HD bool pack_fits(uint64_t at, uint64_t size, uint64_t out_cap) { return at <= out_cap && size <= out_cap - at; }
PACK_HD uint8_t pack_final_verdict(uint8_t v, uint64_t at, uint64_t size, uint64_t out_cap) {
  return (size != 0 && !pack_fits(at, size, out_cap)) ? kPackMalformed : v;
}

// ---- search ----------------------------------------------------------------
// off(i), 0 <= i <= n, is the exclusive scan of the sizes (off(n) = total).
// The last i in [lo, hi] with off(i) <= x; off(lo) <= x is required.
// Zero-size entries share their offset with the next non-zero one, so for
// x < total "the last entry with offset <= x" is always the non-zero entry
// that covers byte x: it has off(i) <= x < off(i + 1).
template <class Off>
PACK_HD uint64_t pack_find(const Off &off, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off(mid) <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// The same search by kPackWide lanes at once (the kernel: one wave, a ballot):
// per round lane l probes entry pack_wide_probe() (when <= hi), `cnt` lanes find
// off(probe) <= x -- off is monotone, so they are the first cnt -- and
// pack_wide_step() narrows [lo, hi] to what lies between the last yes and the
// first no.  Start: lo = 0 (off(0) = 0 <= x), hi = n - 1; done when lo == hi.
constexpr uint32_t kPackWide = 64;
PACK_HD uint64_t pack_wide_stride(uint64_t lo, uint64_t hi) { return (hi - lo + kPackWide - 1) / kPackWide; }
PACK_HD uint64_t pack_wide_probe(uint64_t lo, uint64_t hi, uint32_t lane) {
  return lo + (uint64_t)(lane + 1) * pack_wide_stride(lo, hi);
}
PACK_HD void pack_wide_step(uint64_t *lo, uint64_t *hi, uint32_t cnt) {
  const uint64_t stride = pack_wide_stride(*lo, *hi);
  const uint64_t below_no = *lo + (uint64_t)(cnt + 1) * stride - 1; // the first probe that said no, less one
  *lo += (uint64_t)cnt * stride;
  if (below_no < *hi) *hi = below_no;
}

// ---- byte plumbing ---------------------------------------------------------
// Words are little-endian images of output bytes: byte b of a piece is bits
// 8 * (b & 3) of word b >> 2.
PACK_HD uint32_t pack_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}
// The 12 header bytes (version, type, body_len, crc32 big-endian: rpc_async.c:521-530).
PACK_HD void pack_header_words(uint32_t version, uint32_t type, uint32_t len, uint32_t crc, uint32_t h[3]) {
  h[0] = ((version >> 8) & 0xFFu) | ((version & 0xFFu) << 8) | (((type >> 8) & 0xFFu) << 16) | ((type & 0xFFu) << 24);
  h[1] = pack_bswap(len);
  h[2] = pack_bswap(crc);
}
// Bytes r .. r + 3 of the 8-byte run {lo, hi}, r in 0 .. 3.
PACK_HD uint32_t pack_funnel(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
  return r ? (lo >> (8 * r)) | (hi << (32 - 8 * r)) : lo;
#endif
}
// Header bytes hs .. hs + 3 as a word; bytes outside 0 .. 11 read 0.  -15 <= hs <= 27.
PACK_HD uint32_t pack_header_at(const uint32_t h[3], int hs) {
  const uint32_t u = (uint32_t)(hs + 16), k = u >> 2, r = u & 3; // word k - 4 of the header
  const uint32_t a = k == 4 ? h[0] : k == 5 ? h[1] : k == 6 ? h[2] : 0u;
  const uint32_t b = k == 3 ? h[0] : k == 4 ? h[1] : k == 5 ? h[2] : 0u;
  return pack_funnel(b, a, r);
}
// The bytes of word j (piece bytes 4j .. 4j + 3) that lie in [b, e).
PACK_HD uint32_t pack_range_mask(uint32_t j, uint32_t b, uint32_t e) {
  const uint32_t w0 = 4 * j, w1 = w0 + 4;
  const uint32_t lo = b > w0 ? (b < w1 ? b - w0 : 4u) : 0u;
  const uint32_t hi = e > w0 ? (e < w1 ? e - w0 : 4u) : 0u;
  if (hi <= lo) return 0u;
  const uint32_t upto_hi = hi >= 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u;
  const uint32_t upto_lo = (1u << (8 * lo)) - 1u; // lo <= 3 here
  return upto_hi & ~upto_lo;
}
// Two consecutive aligned 16-byte blocks as words a0 .. a7, k in 0 .. 15: bytes
// k .. k + 15.  Words q .. q + 4 (q = k / 4) come from a two-stage barrel shift
// on plain values: selects, not an indexed read -- an array indexed by a lane's
// own q would live in scratch memory.
PACK_HD uint32_t pack_pick(bool c, uint32_t yes, uint32_t no) { return c ? yes : no; }
PACK_HD void pack_win_select8(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4, uint32_t a5, uint32_t a6,
                              uint32_t a7, uint32_t k, uint32_t win[4]) {
  const uint32_t r = k & 3;
  const bool one = (k & 4) != 0, two = (k & 8) != 0;
  const uint32_t t0 = pack_pick(one, a1, a0), t1 = pack_pick(one, a2, a1), t2 = pack_pick(one, a3, a2),
                 t3 = pack_pick(one, a4, a3), t4 = pack_pick(one, a5, a4), t5 = pack_pick(one, a6, a5),
                 t6 = pack_pick(one, a7, a6);
  const uint32_t s0 = pack_pick(two, t2, t0), s1 = pack_pick(two, t3, t1), s2 = pack_pick(two, t4, t2),
                 s3 = pack_pick(two, t5, t3), s4 = pack_pick(two, t6, t4);
  win[0] = pack_funnel(s1, s0, r);
  win[1] = pack_funnel(s2, s1, r);
  win[2] = pack_funnel(s3, s2, r);
  win[3] = pack_funnel(s4, s3, r);
}
PACK_HD void pack_win_select(const uint32_t w8[8], uint32_t k, uint32_t win[4]) {
  pack_win_select8(w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7], k, win);
}

// ---- the piece resolver ----------------------------------------------------
// Src: the source buffer.
//   uint64_t addr()                       its address (only the low 4 bits and the order matter)
//   uint64_t bytes()                      its size
//   void block16(uint64_t p, uint32_t w[4])   the aligned 16 bytes at buffer offset p (addr() + p is a multiple of 16)
//   uint8_t byte(uint64_t p)              one byte
// Source bytes [s - bb, s - bb + 16) -- so that source byte s lands on piece
// byte bb -- through two aligned blocks; false when a block would leave
// [addr(), addr() + bytes()): the aligned loads over-read up to 15 bytes on
// either side of a body, and at the buffer's edges that is not allowed.
struct PackWin {
  bool ok;      // both aligned blocks lie inside the buffer
  uint64_t blk; // buffer offset of the first block
  uint32_t k;   // the window starts k bytes into it
};
template <class Src>
PACK_HD PackWin pack_win_plan(const Src &src, uint64_t s, uint32_t bb) {
  const uint64_t a = src.addr() + s - bb, lo = a & ~(uint64_t)15;
  const bool ok = !(src.addr() + s < bb || lo < src.addr() || lo + 32 > src.addr() + src.bytes());
  return PackWin{ok, lo - src.addr(), (uint32_t)(a & 15)};
}
template <class Src>
PACK_HD bool pack_window(const Src &src, uint64_t s, uint32_t bb, uint32_t win[4]) {
  const PackWin w = pack_win_plan(src, s, bb);
  if (!w.ok) return false;
  uint32_t w8[8];
  src.block16(w.blk, w8);
  src.block16(w.blk + 16, w8 + 4);
  pack_win_select(w8, w.k, win);
  return true;
}
// Is the piece [x0, x1) at piece byte b0 sixteen body bytes of the one written
// frame [fo, fe)?  Then it is pack_win_plan(src, source offset of x0, 0), two
// block loads, pack_win_select and one 16-byte store: the kernel resolves all
// pieces of a lane first and has the loads of those in flight together.
PACK_HD bool pack_piece_is_body(uint64_t fo, uint64_t fe, uint64_t x0, uint64_t x1, uint32_t b0, uint64_t out_cap) {
  return b0 == 0 && x1 - x0 == kPackPiece && x0 >= fo + kPackHeaderLen && x1 <= fe && fe <= out_cap;
}

// One 16-byte piece: the words and which of its bytes are to be stored (bit b =
// piece byte b).  A byte is stored iff it belongs to a frame that is written.
struct PackPiece {
  uint32_t w[4];
  uint32_t mask;
};
// Ent: the entries.
//   uint64_t src(uint64_t e)                  source offset of entry e's body
//   void header(uint64_t e, uint32_t h[3])    its 12 header bytes (pack_header_words)
// The piece holds output bytes [x0, x1) at piece bytes b0 .., x1 - x0 <= 16 - b0,
// x0 < x1 <= total.  [lo, hi]: entries that can cover it (off(lo) <= x0, and the
// entry that covers x1 - 1 is <= hi).  *last: the entry covering x1 - 1 (the
// next piece's lo).
template <class Off, class Ent, class Src>
PACK_HD PackPiece pack_piece(const Off &off, const Ent &ent, const Src &src, uint64_t lo, uint64_t hi, uint64_t x0,
                             uint64_t x1, uint32_t b0, uint64_t out_cap, uint64_t *last) {
  PackPiece p{{0, 0, 0, 0}, 0};
  uint64_t x = x0;
  uint32_t b = b0;
  uint64_t e = pack_find(off, lo, hi, x); // the last entry with offset <= x covers x (see pack_find)
  for (;;) {
    const uint64_t fo = off(e), fe = off(e + 1);
    const uint32_t cnt = (uint32_t)((fe < x1 ? fe : x1) - x); // >= 1: fe > x
    if (fe <= out_cap) { // the frame is written
      const uint64_t at = x - fo;
      uint32_t done = 0;
      if (at < kPackHeaderLen) {
        const uint32_t room = kPackHeaderLen - (uint32_t)at;
        done = cnt < room ? cnt : room;
        uint32_t h[3];
        ent.header(e, h);
        PACK_UNROLL
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t m = pack_range_mask(j, b, b + done);
          p.w[j] = (p.w[j] & ~m) | (pack_header_at(h, (int)(4 * j) + (int)at - (int)b) & m);
        }
      }
      if (done < cnt) {
        const uint32_t bb = b + done, bc = cnt - done;
        const uint64_t s = ent.src(e) + (at + done - kPackHeaderLen);
        uint32_t win[4];
        if (pack_window(src, s, bb, win)) {
          PACK_UNROLL
          for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t m = pack_range_mask(j, bb, bb + bc);
            p.w[j] = (p.w[j] & ~m) | (win[j] & m);
          }
        } else { // at the source buffer's edge: bytewise
          for (uint32_t i = 0; i < bc; ++i) {
            const uint32_t pos = bb + i, sh = 8 * (pos & 3), v = src.byte(s + i);
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
    e = pack_find(off, e + 1, hi, x); // (off(e + 1) == x; skips zero-size entries)
  }
  *last = e;
  return p;
}

// The tiles and pieces are aligned to the output's address, not to its first
// byte: with mis = address of d_out mod 16, piece P covers output bytes
// [16 P - mis, 16 P - mis + 16), cut to [0, limit).
struct PackSpan {
  uint64_t x0, x1; // output bytes (x0 < x1), or x0 == x1: nothing
  uint32_t b0;     // piece byte of x0
};
PACK_HD PackSpan pack_span(uint64_t start, uint64_t nbytes, uint32_t mis, uint64_t limit) {
  // start, nbytes: relative to the aligned-down output address
  const uint64_t end = start + nbytes;
  PackSpan s{0, 0, 0};
  if (end <= mis) return s;
  s.x0 = start > mis ? start - mis : 0;
  s.b0 = start > mis ? 0u : (uint32_t)(mis - start);
  s.x1 = end - mis < limit ? end - mis : limit;
  if (s.x1 < s.x0) s.x1 = s.x0;
  return s;
}
// Tiles that hold a byte of [0, limit).
PACK_HD uint64_t pack_tiles(uint64_t limit, uint32_t mis, uint32_t tile) {
  return limit ? (limit + mis + tile - 1) / tile : 0;
}
// The finish pass's connection rule: the output byte at which connection i
// begins, i <= nconn (i == nconn: the end).  conn_first is the CSR over the n
// entries; one that runs past them reads as the end.
template <class Off>
PACK_HD uint64_t pack_conn_begin(const Off &off, const uint64_t *conn_first, uint64_t i, uint64_t nconn, uint64_t n) {
  const uint64_t f = i < nconn ? conn_first[i] : n;
  return off(f < n ? f : n);
}

// ---- the call (frames_pack.hip) ---------------------------------------------
struct PackArgs {
  const uint8_t *bodies = nullptr;
  uint64_t bodies_bytes = 0;
  const uint64_t *body_off = nullptr; // may be nullptr when no entry can be a data frame
  const uint32_t *body_len = nullptr;
  uint64_t n = 0;
  const uint16_t *types = nullptr; // nullptr: `type` for all
  const uint16_t *versions = nullptr;
  uint16_t type = 0, version = 0;
  const uint64_t *conn_first = nullptr; // nconn + 1, or nullptr
  uint64_t nconn = 0;
  int flags = 0;
  // outputs (the caller's; all optional)
  uint8_t *out = nullptr;
  uint64_t out_cap = 0;
  uint64_t *frame_off = nullptr;
  uint8_t *verdict = nullptr;
  uint64_t *conn_bytes_first = nullptr;
  uint64_t *total = nullptr;
  // workspace
  uint64_t *sizes = nullptr; // n
  uint64_t *offs = nullptr;  // n + 1: the layout
  uint64_t *src_off = nullptr; // n: the bodies the CRC pass and the pack kernel read
  uint32_t *src_len = nullptr; // n
  uint32_t *crc = nullptr;     // n (the caller's d_crc, or workspace): written by the CRC pass between the two launches
  uint8_t *pre = nullptr;      // n: provisional verdicts
  uint64_t *scan_tmp = nullptr; // scan_tmp_words(n)
};
// Its arrays in pool workspace, over a WsLayout (workspace.h) or anything with
// its take<T>(count); a.n is set.
template <class Layout> inline void pack_ws_layout(Layout &w, PackArgs &a, size_t tmp_words) {
  a.sizes = w.template take<uint64_t>(a.n);
  a.src_off = w.template take<uint64_t>(a.n);
  a.offs = w.template take<uint64_t>(a.n + 1);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
  a.src_len = w.template take<uint32_t>(a.n);
  a.crc = w.template take<uint32_t>(a.n); // (reserved also when the caller's d_crc takes its place)
  a.pre = w.template take<uint8_t>(a.n);
}

#if defined(__HIPCC__)
// Size pass and exclusive scan: everything the CRC pass needs.
hipError_t launch_frames_pack_layout(const PackArgs &a, hipStream_t s);
// Pack kernel (when a.out is set; a.crc must hold the CRCs) and the finish pass.
hipError_t launch_frames_pack_write(const PackArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
