// tests/cpu_emu/emu_common.h -- what pack_emu.cpp, unpack_emu.cpp and
// carry_emu.cpp share: the abort, the checked readers of a layout and of a
// source buffer, the check of the 64-wide search, and the out file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../rpc_amd/csrc/frames_pack.h"

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

inline void write_out(const char *prog, const char *path, const std::vector<uint8_t> &out) {
  FILE *of = fopen(path, "wb");
  if (!of) die(prog, "cannot write the out file");
  if (!out.empty() && fwrite(out.data(), 1, out.size(), of) != out.size()) die(prog, "short write");
  fclose(of);
}

} // namespace emu
