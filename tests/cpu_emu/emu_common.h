// tests/cpu_emu/emu_common.h -- what the emulators share.  All of them
// (pack_emu.cpp, unpack_emu.cpp, carry_emu.cpp, reply_emu.cpp, request_emu.cpp,
// values_emu.cpp): the abort, the checked readers of a layout and of a source
// buffer, the check of the 64-wide search, and the out file.  The reply, the
// request and the values: splice_run(), their main kernel's tiles, lanes and
// pieces over the stage's policy (rpc_amd/csrc/frames_splice.h), with the checks
// of the fast path against the resolver.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../rpc_amd/csrc/frames_splice.h"

namespace emu {

[[noreturn]] inline void die(const char *prog, const char *what) {
  fprintf(stderr, "%s: %s\n", prog, what);
  abort();
}

// An exclusive scan (Off of frames_pack.h); aborts, saying `outside`, on a read
// beyond it.
struct Off {
  const char *prog;
  const std::vector<uint64_t> *o;
  const char *outside;
  uint64_t operator()(uint64_t i) const {
    if (i >= o->size()) die(prog, outside);
    return (*o)[i];
  }
};

// A source buffer at a pretended address (Src of frames_pack.h); aborts on a
// byte or a block outside it and on an unaligned block.
struct Src {
  const char *prog;
  const std::vector<uint8_t> *b;
  uint64_t base;
  const char *byte_outside, *block_outside;
  uint64_t addr() const { return base; }
  uint64_t bytes() const { return b->size(); }
  uint8_t byte(uint64_t p) const {
    if (p >= b->size()) die(prog, byte_outside);
    return (*b)[p];
  }
  void block16(uint64_t p, uint32_t w[4]) const {
    if ((base + p) & 15u) die(prog, "block16 at an unaligned address");
    if (p > b->size() || b->size() - p < 16) die(prog, block_outside);
    memcpy(w, b->data() + p, 16); // (little-endian host)
  }
};

// The wave-wide search for x over entries 0 .. n - 1 as the kernels' wave_find
// runs it, 64 lanes simulated, and the plain one it must agree with.
// not_covering: what to say when off(e) <= x < off(e + 1) does not hold for the
// entry found, or nullptr where that is not required.
inline uint64_t wide_find(const Off &off, uint64_t n, uint64_t x, const char *not_covering) {
  uint64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    uint32_t cnt = 0;
    for (uint32_t lane = 0; lane < rpccrc::kPackWide; ++lane) {
      const uint64_t probe = rpccrc::pack_wide_probe(lo, hi, lane);
      const bool le = probe <= hi && off(probe) <= x;
      if (le && cnt != lane) die(off.prog, "wide search: the lanes that say yes are not a prefix");
      cnt += le;
    }
    rpccrc::pack_wide_step(&lo, &hi, cnt);
  }
  if (lo != rpccrc::pack_find(off, 0, n - 1, x)) die(off.prog, "wide search disagrees with the binary search");
  if (not_covering && !(off(lo) <= x && x < off(lo + 1))) die(off.prog, not_covering);
  return lo;
}

// The main kernel of a splice stage (splice_tile of frames_splice.h under
// tile_drive): tiles of `tile` bytes and pieces aligned to the output's address
// (mis: its low four bits), the pieces dealt out to up to 256 lanes.  Per piece,
// as the kernel: the lane's own search, the fast path when splice_plan() gives a
// window, the resolver otherwise -- and here the resolver always, which the
// fast path must agree with.  Pol: the stage's policy over checked readers
// (its src(m) an emu::Src); n: entries of the layout off; put(x, v): output
// byte x.
template <class Pol, class Put>
inline void splice_run(const char *prog, const Pol &pol, const Off &off, const Off &src_of, uint64_t n, uint64_t total,
                       uint64_t out_cap, uint32_t mis, uint32_t tile, const char *not_covering, const Put &put) {
  using namespace rpccrc;
  const uint64_t ntiles = n && out_cap ? pack_tiles(total < out_cap ? total : out_cap, mis, tile) : 0;
  for (uint64_t t = 0; t < ntiles; ++t) {
    const PackSpan ts = pack_span(t * tile, tile, mis, total);
    if (ts.x0 >= ts.x1) die(prog, "a tile with no byte");
    // the wave-wide search, and the plain one it must agree with
    const uint64_t range[2] = {wide_find(off, n, ts.x0, not_covering), wide_find(off, n, ts.x1 - 1, not_covering)};
    const uint32_t pieces = tile / kPackPiece, lanes = pieces < 256 ? pieces : 256;
    for (uint32_t lane = 0; lane < lanes; ++lane) {
      uint64_t lo = range[0];
      for (uint32_t k = 0; k * lanes + lane < pieces; ++k) {
        const uint64_t at = t * tile + ((uint64_t)k * lanes + lane) * kPackPiece;
        const PackSpan ps = pack_span(at, kPackPiece, mis, ts.x1);
        if (ps.x0 >= ps.x1) continue;
        const uint64_t e = pack_find(off, lo, range[1], ps.x0);
        lo = e;
        bool middle;
        uint64_t src_addr = 0;
        const PackWin w = splice_plan(pol, src_of, e, off(e), off(e + 1), ps.x0, ps.x1, ps.b0, &middle, &src_addr);
        const PackPiece p = splice_piece(pol, off, src_of, range[0], range[1], ps.x0, ps.x1, ps.b0);
        if (p.mask >> 16) die(prog, "mask beyond the piece");
        uint32_t words[4] = {p.w[0], p.w[1], p.w[2], p.w[3]};
        if (middle && p.mask != 0xFFFFu) die(prog, "a middle piece is not stored whole");
        if (w.ok) {
          const Src &src = pol.src(pol.meta(e));
          uint32_t w8[8];
          src.block16(w.blk, w8);
          src.block16(w.blk + 16, w8 + 4);
          pack_win_select(w8, w.k, words);
          if (memcmp(words, p.w, 16) != 0) die(prog, "fast path and resolver disagree");
        }
        for (uint32_t b = 0; b < kPackPiece; ++b) {
          if (!((p.mask >> b) & 1u)) continue;
          if (at + b < mis) die(prog, "store before the output's first byte");
          put(at + b - mis, (uint8_t)(words[b >> 2] >> (8 * (b & 3))));
        }
      }
    }
  }
}

inline void write_out(const char *prog, const char *path, const std::vector<uint8_t> &out) {
  FILE *of = fopen(path, "wb");
  if (!of) die(prog, "cannot write the out file");
  if (!out.empty() && fwrite(out.data(), 1, out.size(), of) != out.size()) die(prog, "short write");
  fclose(of);
}

} // namespace emu
