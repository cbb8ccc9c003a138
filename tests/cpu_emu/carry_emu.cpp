// tests/cpu_emu/carry_emu.cpp -- CPU emulation of the frame carry
// (rpc_amd/csrc/frames_carry.hip) on the shared source of frames_carry.h (and the
// frames_pack.h helpers it uses): the rule, the pieces aligned to the
// destination's address with their funnel shift and byte masks, and on the long
// route the chunk counts, their exclusive scan, the chunk -> connection search
// (binary and the 64-wide form the kernel runs on a wave), run as the kernels run
// them (one loop iteration per workgroup or lane), at the kernel's own
// kCarryChunk or at a small chunk.
//
//   carry_emu <chunk> <group | 0: the long route> <room> <use_state> <src_mis> <next_mis>
//             <next_bytes> <stream file> <conn file> <out file>
//
// conn file: text, "off len consumed state at new_len" per line.  src_mis /
// next_mis: the low address bits the stream and the next buffer pretend to have.
// stdout: per connection "next_off next_len status", then "carried N".  out
// file: next_bytes bytes, 0xA5 where nothing was written.
// The stream reader aborts on any byte outside [0, stream_bytes); the writer
// aborts on any byte outside a tail that is to be written, on a byte written
// twice and, at the end, on a byte of such a tail that was left out.
#include <fstream>
#include <iterator>
#include <string>

#include "../../rpc_amd/csrc/frames_carry.h"
#include "emu_common.h"

using namespace rpccrc;

namespace {

const char kProg[] = "carry_emu";
[[noreturn]] void die(const char *what) { emu::die(kProg, what); }

struct Conn {
  uint64_t off, len, consumed, state, at, nl;
};

} // namespace

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: carry_emu chunk group room use_state src_mis next_mis next_bytes stream conn out\n");
    return 2;
  }
  const uint32_t chunk = (uint32_t)strtoul(argv[1], nullptr, 10);
  const uint32_t group = (uint32_t)strtoul(argv[2], nullptr, 10);
  const uint64_t room = strtoull(argv[3], nullptr, 10);
  const bool use_state = atoi(argv[4]) != 0;
  const uint64_t src_mis = strtoull(argv[5], nullptr, 10) & 15u;
  const uint64_t next_bytes = strtoull(argv[7], nullptr, 10);
  if (chunk == 0 || chunk % kPackPiece || (chunk & (chunk - 1))) die("chunk must be whole pieces and a power of two");
  const uint64_t next_base = (1ull << 24) + strtoull(argv[6], nullptr, 10) % chunk;
  std::ifstream bf(argv[8], std::ios::binary);
  const std::vector<uint8_t> stream((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
  std::vector<Conn> conns;
  {
    std::ifstream cf(argv[9]);
    Conn c;
    while (cf >> c.off >> c.len >> c.consumed >> c.state >> c.at >> c.nl) conns.push_back(c);
  }
  const uint64_t n = conns.size();
  const emu::Src src{kProg, &stream, 4096 + src_mis, "stream byte read outside [0, stream_bytes)",
                     "stream block read outside [0, stream_bytes)"};

  // the rule, as plan_of() in the kernels: only the state of a closed connection is looked at
  std::vector<CarryPlan> plan(n);
  uint64_t carried = 0;
  for (uint64_t c = 0; c < n; ++c) {
    const bool closed = use_state && conns[c].state != kCarryConnOpen;
    const Conn z = closed ? Conn{0, 0, 0, 0, 0, 0} : conns[c];
    plan[c] = carry_plan_one(closed, z.off, z.len, z.consumed, stream.size(), z.at, z.nl, next_bytes, room);
    if (plan[c].status != kCarryOk && (plan[c].tail || plan[c].next_off || plan[c].next_len))
      die("a connection that is not carried has a tail or a next connection");
    carried += plan[c].tail;
  }

  // what is to be written: the tails of the plans
  std::vector<uint8_t> wanted(next_bytes, 0), written(next_bytes, 0), out(next_bytes, 0xA5);
  for (uint64_t c = 0; c < n; ++c)
    for (uint64_t x = 0; x < plan[c].tail; ++x) {
      if (plan[c].next_off + x >= next_bytes) die("a planned tail leaves the next buffer");
      wanted[plan[c].next_off + x] = 1;
    }
  auto put = [&](uint64_t addr, uint8_t v) { // addr: the pretended address
    if (addr < next_base || addr - next_base >= next_bytes) die("store outside the next buffer");
    const uint64_t x = addr - next_base;
    if (!wanted[x]) die("store outside a tail that is to be written");
    if (written[x]) die("byte stored twice");
    written[x] = 1;
    out[x] = v;
  };
  // One piece of connection c at `start` bytes from the aligned address d - mis,
  // as the kernels produce it: the fast path when it is sixteen tail bytes and
  // the window stays inside the stream, the resolver otherwise; both must agree.
  auto piece = [&](uint64_t c, uint64_t d, uint32_t mis, uint64_t start) {
    const PackSpan ps = pack_span(start, kPackPiece, mis, plan[c].tail);
    if (ps.x0 >= ps.x1) return;
    const PackPiece p = carry_piece(src, plan[c].src, ps);
    if (p.mask >> 16) die("mask beyond the piece");
    uint32_t words[4] = {p.w[0], p.w[1], p.w[2], p.w[3]};
    if (carry_piece_is_whole(ps)) {
      if (p.mask != 0xFFFFu) die("a whole piece is not stored whole");
      const PackWin w = pack_win_plan(src, plan[c].src + ps.x0, 0);
      if (w.ok) {
        uint32_t w8[8];
        src.block16(w.blk, w8);
        src.block16(w.blk + 16, w8 + 4);
        pack_win_select(w8, w.k, words);
        if (memcmp(words, p.w, 16) != 0) die("fast path and resolver disagree");
      }
    }
    if ((d - mis + start) & 15u) die("a piece at an unaligned address");
    for (uint32_t b = 0; b < kPackPiece; ++b)
      if ((p.mask >> b) & 1u) put(d - mis + start + b, (uint8_t)(words[b >> 2] >> (8 * (b & 3))));
  };

  if (group) { // short route: `group` lanes per connection
    for (uint64_t c = 0; c < n; ++c) {
      if (!plan[c].tail) continue;
      const uint64_t d = next_base + plan[c].next_off;
      const uint32_t mis = carry_mis(d, kPackPiece);
      const uint64_t pieces = pack_tiles(plan[c].tail, mis, kPackPiece);
      for (uint32_t l = 0; l < group; ++l)
        for (uint64_t k = l; k < pieces; k += group) piece(c, d, mis, k * kPackPiece);
    }
  } else { // long route: chunk counts, exclusive scan, a workgroup per chunk
    std::vector<uint64_t> offs(n + 1, 0);
    for (uint64_t c = 0; c < n; ++c) offs[c + 1] = offs[c] + carry_chunks(plan[c].tail, next_base + plan[c].next_off, chunk);
    const emu::Off off{kProg, &offs, "offset read outside the chunk layout"};
    for (uint64_t ch = 0; ch < offs[n]; ++ch) {
      // the wave-wide search, and the plain one it must agree with
      const uint64_t c = emu::wide_find(off, n, ch, "the connection found does not hold the chunk");
      const uint64_t d = next_base + plan[c].next_off;
      const uint32_t mis = carry_mis(d, chunk);
      const uint64_t start = (ch - off(c)) * chunk;
      const PackSpan cs = pack_span(start, chunk, mis, plan[c].tail);
      if (cs.x0 >= cs.x1) die("a chunk with no byte");
      const uint32_t pieces = chunk / kPackPiece, lanes = pieces < 256 ? pieces : 256;
      for (uint32_t lane = 0; lane < lanes; ++lane)
        for (uint32_t k = 0; k * lanes + lane < pieces; ++k)
          piece(c, d, mis, start + ((uint64_t)k * lanes + lane) * kPackPiece);
    }
  }
  for (uint64_t x = 0; x < next_bytes; ++x)
    if (wanted[x] && !written[x]) die("a byte of a tail was left out");

  for (uint64_t c = 0; c < n; ++c)
    printf("%llu %llu %u\n", (unsigned long long)plan[c].next_off, (unsigned long long)plan[c].next_len,
           (unsigned)plan[c].status);
  printf("carried %llu\n", (unsigned long long)carried);
  emu::write_out(kProg, argv[10], out);
  return 0;
}
