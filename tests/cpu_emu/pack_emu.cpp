// tests/cpu_emu/pack_emu.cpp -- CPU emulation of the frame pack
// (rpc_amd/csrc/frames_pack.hip) on the shared source of frames_pack.h: the
// sizing rule, the exclusive scan, the per-tile entry search (binary and the
// 64-wide form the kernel runs on a wave), the piece resolver and the store, run
// as the kernels run them (one loop iteration per workgroup or lane), at the
// kernels' own kPackTile or at a small tile.
//
//   pack_emu <tile> <flags> <out_cap | -1: the total> <src_mis> <out_mis>
//            <bodies file> <entries file> <conn file | -> <out file>
//
// entries file: text, "type version off len" per line.  conn file: the CSR, one
// word per line.  src_mis / out_mis: the low four address bits the source buffer
// and the output pretend to have.  stdout: "total N", per entry "off verdict
// crc", then "conn b_0 ... b_nconn".  out file: out_cap bytes, 0xA5 where nothing
// was written.
// The source reader aborts on any byte outside [0, bodies_bytes); the output
// writer aborts on any byte outside a frame that is to be written, on a byte
// written twice and, at the end, on a byte of a written frame that was left out.
#include <fstream>
#include <iterator>
#include <string>

#include "emu_common.h"

using namespace rpccrc;

namespace {

const char kProg[] = "pack_emu";
[[noreturn]] void die(const char *what) { emu::die(kProg, what); }

uint32_t crc32_bitwise(const uint8_t *p, uint64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

struct Ent {
  const std::vector<uint64_t> *src_off;
  const std::vector<uint32_t> *src_len, *crc, *type, *version;
  uint64_t src(uint64_t e) const { return (*src_off)[e]; }
  void header(uint64_t e, uint32_t h[3]) const {
    pack_header_words((*version)[e], (*type)[e], (*src_len)[e], (*crc)[e], h);
  }
};

} // namespace

int main(int argc, char **argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: pack_emu tile flags out_cap src_mis out_mis bodies entries conn|- out\n");
    return 2;
  }
  const uint32_t tile = (uint32_t)strtoul(argv[1], nullptr, 10);
  const int flags = atoi(argv[2]);
  const long long cap_arg = atoll(argv[3]);
  const uint32_t src_mis = (uint32_t)atoi(argv[4]) & 15u, mis = (uint32_t)atoi(argv[5]) & 15u;
  if (tile == 0 || tile % kPackPiece) die("tile must be whole pieces");
  std::ifstream bf(argv[6], std::ios::binary);
  const std::vector<uint8_t> bodies((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
  std::vector<uint32_t> type, version, len;
  std::vector<uint64_t> boff;
  {
    std::ifstream ef(argv[7]);
    uint64_t t, v, o, l;
    while (ef >> t >> v >> o >> l) {
      type.push_back((uint32_t)t);
      version.push_back((uint32_t)v);
      boff.push_back(o);
      len.push_back((uint32_t)l);
    }
  }
  std::vector<uint64_t> conn_first;
  if (strcmp(argv[8], "-") != 0) {
    std::ifstream cf(argv[8]);
    uint64_t v;
    while (cf >> v) conn_first.push_back(v);
  }
  const uint64_t n = type.size();

  // size pass, exclusive scan, CRC pass
  std::vector<uint64_t> size(n), src_off(n), offs(n + 1, 0);
  std::vector<uint32_t> src_len(n), crc(n);
  std::vector<uint8_t> pre(n);
  for (uint64_t i = 0; i < n; ++i) {
    const bool data = pack_is_data(type[i]);
    const PackSize z = pack_size_one(type[i], data ? boff[i] : 0, data ? len[i] : 0, bodies.size(), flags);
    size[i] = z.size;
    src_off[i] = z.off;
    src_len[i] = z.len;
    pre[i] = z.verdict;
  }
  for (uint64_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + size[i];
  for (uint64_t i = 0; i < n; ++i) crc[i] = src_len[i] ? crc32_bitwise(bodies.data() + src_off[i], src_len[i]) : 0u;
  const uint64_t total = offs[n];
  const uint64_t out_cap = cap_arg < 0 ? total : (uint64_t)cap_arg;

  // what is to be written: the bytes of every non-empty entry that ends inside out_cap
  std::vector<uint8_t> wanted(out_cap, 0), written(out_cap, 0), out(out_cap, 0xA5);
  for (uint64_t i = 0; i < n; ++i)
    if (size[i] && pack_fits(offs[i], size[i], out_cap))
      for (uint64_t x = offs[i]; x < offs[i + 1]; ++x) wanted[x] = 1;
  auto put = [&](uint64_t x, uint8_t v) {
    if (x >= out_cap) die("store at or beyond out_cap");
    if (!wanted[x]) die("store outside a frame that is to be written");
    if (written[x]) die("byte stored twice");
    written[x] = 1;
    out[x] = v;
  };

  // pack kernel: tiles and pieces aligned to the output's address
  const emu::Off off{kProg, &offs, "offset read outside the layout"};
  const Ent ent{&src_off, &src_len, &crc, &type, &version};
  const emu::Src src{kProg, &bodies, 4096 + src_mis, "source byte read outside [0, bodies_bytes)",
                     "source block read outside [0, bodies_bytes)"};
  const uint64_t ntiles = n ? pack_tiles(total < out_cap ? total : out_cap, mis, tile) : 0;
  for (uint64_t t = 0; t < ntiles; ++t) {
    const PackSpan ts = pack_span(t * tile, tile, mis, total);
    if (ts.x0 >= ts.x1) die("a tile with no byte");
    // the wave-wide search, and the plain one it must agree with
    const uint64_t range[2] = {emu::wide_find(off, n, ts.x0, "the entry found does not cover the byte"),
                               emu::wide_find(off, n, ts.x1 - 1, "the entry found does not cover the byte")};
    const uint32_t pieces = tile / kPackPiece, lanes = pieces < 256 ? pieces : 256;
    for (uint32_t lane = 0; lane < lanes; ++lane) {
      uint64_t lo = range[0];
      for (uint32_t k = 0; k * lanes + lane < pieces; ++k) {
        const uint64_t at = t * tile + ((uint64_t)k * lanes + lane) * kPackPiece;
        const PackSpan ps = pack_span(at, kPackPiece, mis, ts.x1);
        if (ps.x0 >= ps.x1) continue;
        const PackPiece p = pack_piece(off, ent, src, lo, range[1], ps.x0, ps.x1, ps.b0, out_cap, &lo);
        if (p.mask >> 16) die("mask beyond the piece");
        { // the kernel's fast path for a piece of sixteen body bytes must give the same words
          const uint64_t e = pack_find(off, range[0], range[1], ps.x0);
          if (pack_piece_is_body(off(e), off(e + 1), ps.x0, ps.x1, ps.b0, out_cap)) {
            if (p.mask != 0xFFFFu) die("a body piece is not stored whole");
            const PackWin w = pack_win_plan(src, ent.src(e) + (ps.x0 - off(e) - kPackHeaderLen), 0);
            if (w.ok) {
              uint32_t w8[8], win[4];
              src.block16(w.blk, w8);
              src.block16(w.blk + 16, w8 + 4);
              pack_win_select(w8, w.k, win);
              if (memcmp(win, p.w, 16) != 0) die("fast path and resolver disagree");
            }
          }
        }
        for (uint32_t b = 0; b < kPackPiece; ++b) {
          if (!((p.mask >> b) & 1u)) continue;
          if (at + b < mis) die("store before the output's first byte");
          put(at + b - mis, (uint8_t)(p.w[b >> 2] >> (8 * (b & 3))));
        }
      }
    }
  }
  for (uint64_t x = 0; x < out_cap; ++x)
    if (wanted[x] && !written[x]) die("a byte of a written frame was left out");

  // finish pass
  printf("total %llu\n", (unsigned long long)total);
  for (uint64_t i = 0; i < n; ++i)
    printf("%llu %u %u\n", (unsigned long long)offs[i], (unsigned)pack_final_verdict(pre[i], offs[i], size[i], out_cap),
           (unsigned)crc[i]);
  printf("conn");
  for (size_t c = 0; c < conn_first.size(); ++c)
    printf(" %llu", (unsigned long long)pack_conn_begin(off, conn_first.data(), c, conn_first.size() - 1, n));
  printf("\n");
  emu::write_out(kProg, argv[9], out);
  return 0;
}
