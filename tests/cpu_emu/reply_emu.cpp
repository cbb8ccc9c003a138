// tests/cpu_emu/reply_emu.cpp -- CPU emulation of the frame reply
// (rpc_amd/csrc/frames_reply.hip) on the shared source of frames_reply.h (and
// the frames_pack.h / frames_unpack.h helpers it uses): the sizing rule, the
// exclusive scan, the per-tile entry search (binary and the 64-wide form the
// kernel runs on a wave), the fast path, the piece resolver with its generated
// bytes and the store, run as the kernels run them (one loop iteration per
// workgroup or lane), at the kernels' own kPackTile or at a small tile.
//
//   reply_emu <tile> <given> <out_cap | -1: the total> <src_mis> <out_mis>
//             <values file | @N> <entries file> <conn file | -> <out file>
//
// given: bit 0 d_reply_types, bit 1 d_kind, bit 2 d_status.  entries file:
// text, "type kind id status value_offset value_length" per line.  @N: a values
// buffer of N bytes that is only claimed (every read aborts).  conn file: the
// CSR, one word per line.  src_mis / out_mis: the low four address bits the
// values and the output pretend to have.  stdout: "total N", per entry "off len
// type state", then "conn b_0 ... b_nconn".  out file: out_cap bytes, 0xA5 where
// nothing was written.
// The values reader aborts on any byte outside [0, values_bytes); the inputs of
// an entry abort when the rules must not look at them; the output writer aborts
// on any byte outside an entry that is to be written, on a byte written twice
// and, at the end, on a byte of a written entry that was left out.
#include <fstream>
#include <iterator>
#include <string>

#include "../../rpc_amd/csrc/frames_reply.h"
#include "emu_common.h"

using namespace rpccrc;

namespace {

const char kProg[] = "reply_emu";
[[noreturn]] void die(const char *what) { emu::die(kProg, what); }

struct Entry {
  uint32_t type, kind, id;
  int32_t status;
  uint64_t voff;
  uint32_t vlen;
};
// An entry's inputs as the rules ask for them; may_status / may_value: whether
// the header's rules allow the look.
struct In {
  const Entry *e;
  bool stated, may_status, may_value;
  int32_t status() const {
    if (!may_status) die("d_status looked at for an entry that is no CALL");
    return stated ? e->status : 0;
  }
  uint64_t voff() const {
    if (!may_value) die("value offset looked at where the rules do not");
    return e->voff;
  }
  uint32_t vlen() const {
    if (!may_value) die("value length looked at where the rules do not");
    return e->vlen;
  }
};
struct Ent {
  const std::vector<uint16_t> *m;
  const std::vector<Entry> *ents;
  const std::vector<int32_t> *codes;
  uint16_t meta(uint64_t e) const { return m->at(e); }
  uint32_t id(uint64_t e) const { return ents->at(e).id; }
  int32_t code(uint64_t e) const { return codes->at(e); }
};

} // namespace

int main(int argc, char **argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: reply_emu tile given out_cap src_mis out_mis values|@N entries conn|- out\n");
    return 2;
  }
  const uint32_t tile = (uint32_t)strtoul(argv[1], nullptr, 10);
  const int given = atoi(argv[2]);
  const bool typed = given & 1, kinded = given & 2, stated = given & 4;
  const long long cap_arg = atoll(argv[3]);
  const uint32_t src_mis = (uint32_t)atoi(argv[4]) & 15u, mis = (uint32_t)atoi(argv[5]) & 15u;
  if (tile == 0 || tile % kPackPiece) die("tile must be whole pieces");
  std::vector<uint8_t> values;
  uint64_t values_bytes = 0;
  const bool claimed = argv[6][0] == '@';
  if (claimed) {
    values_bytes = strtoull(argv[6] + 1, nullptr, 10);
  } else {
    std::ifstream bf(argv[6], std::ios::binary);
    values.assign((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
    values_bytes = values.size();
  }
  std::vector<Entry> ents;
  {
    std::ifstream ef(argv[7]);
    uint64_t t, k, id, off, len;
    long long st;
    while (ef >> t >> k >> id >> st >> off >> len)
      ents.push_back(Entry{(uint32_t)t, (uint32_t)k, (uint32_t)id, (int32_t)st, off, (uint32_t)len});
  }
  std::vector<uint64_t> conn_first;
  if (strcmp(argv[8], "-") != 0) {
    std::ifstream cf(argv[8]);
    uint64_t v;
    while (cf >> v) conn_first.push_back(v);
  }
  const uint64_t n = ents.size();
  const emu::Src src{kProg, &values, 4096 + src_mis, "values byte read outside [0, values_bytes)",
                     "values block read outside [0, values_bytes)"};

  // size pass, exclusive scan
  std::vector<uint64_t> size(n), src_off(n), offs(n + 1, 0);
  std::vector<int32_t> code(n);
  std::vector<uint16_t> meta(n);
  for (uint64_t i = 0; i < n; ++i) {
    const Entry &e = ents[i];
    const uint32_t type = typed ? e.type : kReplyTypeData;
    const bool data = type == kReplyTypeData;
    const uint32_t kind = !data ? kReplyKindNone : kinded ? e.kind : kReplyKindCall;
    const bool call = data && kind == kReplyKindCall, defer = data && kind == kReplyKindDefer;
    const int32_t s = stated ? e.status : 0;
    const bool fixed = s == -32700 || s == -32600 || s == -32601 || s == -32602 || s == -32603;
    const In in{&e, stated, call, defer || (call && !fixed)};
    const ReplySize z = reply_size_one(in, typed, type, kind, data ? e.id : 0u, values_bytes);
    size[i] = z.size;
    src_off[i] = z.src;
    code[i] = z.code;
    meta[i] = z.meta;
    if (z.size > 0xFFFFFFFFull) die("a body over 32 bits");
    if (reply_pre(z.meta) > z.size && z.size) die("more generated bytes than the entry has");
  }
  for (uint64_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + size[i];
  const uint64_t total = offs[n];
  const uint64_t out_cap = cap_arg < 0 ? total : (uint64_t)cap_arg;
  if (claimed && out_cap != 0) die("a claimed values buffer goes with the layout-only call");

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

  // reply kernel: tiles and pieces aligned to the output's address
  const emu::Off off{kProg, &offs, "offset read outside the layout"};
  const emu::Off src_of{kProg, &src_off, "value offset read outside the entries"};
  const Ent ent{&meta, &ents, &code};
  const uint64_t ntiles = n && out_cap ? pack_tiles(total < out_cap ? total : out_cap, mis, tile) : 0;
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
        // sixteen copied bytes of one written entry and the window stays inside
        // the values, the resolver otherwise
        const uint64_t e = pack_find(off, lo, range[1], ps.x0);
        lo = e;
        PackWin w{false, 0, 0};
        bool middle = false;
        const uint64_t fo = off(e), fe = off(e + 1);
        if (fe - fo >= kPackPiece) {
          const uint16_t m = ent.meta(e);
          const uint32_t pre = reply_pre(m);
          middle = reply_piece_is_middle(fo, fe, pre, reply_suf(reply_form(m)), ps.x0, ps.x1, ps.b0, out_cap);
          if (middle) w = pack_win_plan(src, src_of(e) + (ps.x0 - fo - pre), 0);
        }
        const PackPiece p = reply_piece(off, ent, src_of, src, range[0], range[1], ps.x0, ps.x1, ps.b0, out_cap);
        if (p.mask >> 16) die("mask beyond the piece");
        uint32_t words[4] = {p.w[0], p.w[1], p.w[2], p.w[3]};
        if (middle && p.mask != 0xFFFFu) die("a middle piece is not stored whole");
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
    const uint8_t st = reply_final_status(meta[i], offs[i], size[i], out_cap);
    printf("%llu %u %u %u\n", (unsigned long long)offs[i], (unsigned)(uint32_t)size[i],
           (unsigned)reply_type_out(typed, typed ? ents[i].type : kReplyTypeData, st), (unsigned)st);
  }
  printf("conn");
  for (size_t c = 0; c < conn_first.size(); ++c)
    printf(" %llu", (unsigned long long)pack_conn_begin(off, conn_first.data(), c, conn_first.size() - 1, n));
  printf("\n");
  emu::write_out(kProg, argv[9], out);
  return 0;
}
