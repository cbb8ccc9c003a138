// tests/cpu_emu/unpack_emu.cpp -- CPU emulation of the frame unpack
// (rpc_amd/csrc/frames_unpack.hip) on the shared source of frames_unpack.h (and
// the frames_pack.h helpers it uses): the sizing rule, the exclusive scan, the
// per-tile entry search (binary and the 64-wide form the kernel runs on a wave),
// the piece resolver and the store, run as the kernels run them (one loop
// iteration per workgroup or lane), at the kernels' own kPackTile or at a small
// tile.
//
//   unpack_emu <tile> <flags> <nul> <out_cap | -1: the total> <src_mis> <out_mis>
//              <stream file> <entries file> <conn file | -> <out file>
//
// entries file: text, "offset verdict" per line.  conn file: the CSR, one word
// per line.  src_mis / out_mis: the low four address bits the stream and the
// output pretend to have.  stdout: "total N", per entry "off len reply_type
// version verdict", then "conn b_0 ... b_nconn".  out file: out_cap bytes, 0xA5
// where nothing was written.
// The stream reader aborts on any byte outside [0, stream_bytes); the output
// writer aborts on any byte outside an entry that is to be written, on a byte
// written twice and, at the end, on a byte of a written entry that was left out.
#include <fstream>
#include <iterator>
#include <string>

#include "../../rpc_amd/csrc/frames_unpack.h"
#include "emu_common.h"

using namespace rpccrc;

namespace {

const char kProg[] = "unpack_emu";
[[noreturn]] void die(const char *what) { emu::die(kProg, what); }

} // namespace

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: unpack_emu tile flags nul out_cap src_mis out_mis stream entries conn|- out\n");
    return 2;
  }
  const uint32_t tile = (uint32_t)strtoul(argv[1], nullptr, 10);
  const int flags = atoi(argv[2]), nul = atoi(argv[3]);
  const long long cap_arg = atoll(argv[4]);
  const uint32_t src_mis = (uint32_t)atoi(argv[5]) & 15u, mis = (uint32_t)atoi(argv[6]) & 15u;
  if (tile == 0 || tile % kPackPiece) die("tile must be whole pieces");
  if (nul != 0 && nul != 1) die("nul is 0 or 1");
  std::ifstream bf(argv[7], std::ios::binary);
  const std::vector<uint8_t> stream((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
  std::vector<uint64_t> foff;
  std::vector<uint8_t> vin;
  {
    std::ifstream ef(argv[8]);
    uint64_t o, v;
    while (ef >> o >> v) {
      foff.push_back(o);
      vin.push_back((uint8_t)v);
    }
  }
  std::vector<uint64_t> conn_first;
  if (strcmp(argv[9], "-") != 0) {
    std::ifstream cf(argv[9]);
    uint64_t v;
    while (cf >> v) conn_first.push_back(v);
  }
  const uint64_t n = foff.size();
  const emu::Src src{kProg, &stream, 4096 + src_mis, "stream byte read outside [0, stream_bytes)",
                     "stream block read outside [0, stream_bytes)"};

  // size pass, exclusive scan
  std::vector<uint64_t> size(n), src_off(n), offs(n + 1, 0);
  std::vector<uint16_t> ver(n);
  std::vector<uint8_t> pre(n);
  for (uint64_t i = 0; i < n; ++i) {
    const bool look = vin[i] == kPackOk || vin[i] == kPackControl;
    const UnpackSize z = unpack_size_one(src, vin[i], look ? foff[i] : 0, stream.size(), flags, nul);
    size[i] = z.size;
    src_off[i] = z.src;
    ver[i] = z.version;
    pre[i] = z.verdict;
  }
  for (uint64_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + size[i];
  const uint64_t total = offs[n];
  const uint64_t out_cap = cap_arg < 0 ? total : (uint64_t)cap_arg;

  // what is to be written: the bytes of every non-empty entry that ends inside out_cap
  std::vector<uint8_t> wanted(out_cap, 0), written(out_cap, 0), out(out_cap, 0xA5);
  for (uint64_t i = 0; i < n; ++i)
    if (size[i] && pack_fits(offs[i], size[i], out_cap))
      for (uint64_t x = offs[i]; x < offs[i + 1]; ++x) wanted[x] = 1;
  auto put = [&](uint64_t x, uint8_t v) {
    if (x >= out_cap) die("store at or beyond out_cap");
    if (!wanted[x]) die("store outside an entry that is to be written");
    if (written[x]) die("byte stored twice");
    written[x] = 1;
    out[x] = v;
  };

  // unpack kernel: tiles and pieces aligned to the output's address
  const emu::Off off{kProg, &offs, "offset read outside the layout"};
  const emu::Off src_of{kProg, &src_off, "source offset read outside the entries"};
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
        // as the kernel: the lane's own search, the fast path when the piece is
        // sixteen body bytes of one written entry and the window stays inside
        // the stream, the resolver otherwise
        const uint64_t e = pack_find(off, lo, range[1], ps.x0);
        lo = e;
        PackWin w{false, 0, 0};
        const bool body = unpack_piece_is_body(off(e), off(e + 1), ps.x0, ps.x1, ps.b0, nul, out_cap);
        if (body) w = pack_win_plan(src, src_of(e) + (ps.x0 - off(e)), 0);
        const PackPiece p = unpack_piece(off, src_of, src, range[0], range[1], ps.x0, ps.x1, ps.b0, nul, out_cap);
        if (p.mask >> 16) die("mask beyond the piece");
        uint32_t words[4] = {p.w[0], p.w[1], p.w[2], p.w[3]};
        if (body && p.mask != 0xFFFFu) die("a body piece is not stored whole");
        if (w.ok) {
          uint32_t w8[8];
          src.block16(w.blk, w8);
          src.block16(w.blk + 16, w8 + 4);
          pack_win_select(w8, w.k, words);
          if (memcmp(words, p.w, 16) != 0) die("fast path and resolver disagree");
        }
        for (uint32_t b = 0; b < kPackPiece; ++b) {
          if (!((p.mask >> b) & 1u)) continue;
          if (at + b < mis) die("store before the output's first byte");
          put(at + b - mis, (uint8_t)(words[b >> 2] >> (8 * (b & 3))));
        }
      }
    }
  }
  for (uint64_t x = 0; x < out_cap; ++x)
    if (wanted[x] && !written[x]) die("a byte of a written entry was left out");

  // finish pass
  printf("total %llu\n", (unsigned long long)total);
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t v = unpack_final_verdict(pre[i], offs[i], size[i], out_cap);
    printf("%llu %u %u %u %u\n", (unsigned long long)offs[i], (unsigned)unpack_body_len(pre[i], size[i], nul),
           (unsigned)unpack_reply_type(v, flags), (unsigned)ver[i], (unsigned)v);
  }
  printf("conn");
  for (size_t c = 0; c < conn_first.size(); ++c)
    printf(" %llu", (unsigned long long)pack_conn_begin(off, conn_first.data(), c, conn_first.size() - 1, n));
  printf("\n");
  emu::write_out(kProg, argv[10], out);
  return 0;
}
