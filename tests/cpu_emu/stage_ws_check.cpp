// tests/cpu_emu/stage_ws_check.cpp -- every frame stage's workspace layout (the
// xxx_ws_layout function beside each stage's Args in rpc_amd/csrc/frames*.h)
// over the carver of rpc_amd/csrc/workspace.h, on the host.  For each layout,
// each combination of its conditions, nine counts and three scan sizes: the
// measuring pass and the carving pass agree; the arrays are 256-aligned, in
// order, disjoint, inside the block and at least as long as the kernels index
// them; a block one byte short is refused.  The first and last byte of every
// array are written, for the sanitizer.
//
// The tables of bytes the kernels index are written out here per stage, from
// reading the kernels (the .hip file named at each), not from the layout
// functions.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rpc_amd/csrc/frames.h"
#include "../../rpc_amd/csrc/frames_carry.h"
#include "../../rpc_amd/csrc/frames_pack.h"
#include "../../rpc_amd/csrc/frames_reply.h"
#include "../../rpc_amd/csrc/frames_request.h"
#include "../../rpc_amd/csrc/frames_resolve.h"
#include "../../rpc_amd/csrc/frames_route.h"
#include "../../rpc_amd/csrc/frames_scan.h"
#include "../../rpc_amd/csrc/frames_unpack.h"
#include "../../rpc_amd/csrc/frames_values.h"
#include "../../rpc_amd/csrc/workspace.h"

using namespace rpccrc;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// One array of a carved layout and the bytes the kernels index of it.
struct Arr {
  const void *p;
  size_t bytes;
};

// One layout.  init: the call as its entry point has set it before the
// workspace is taken; lay(w, c): the layout function over it; table(c): the
// arrays in the order they are taken.  Every pass starts from a fresh copy of
// init, as a call does.
template <class Call, class Lay, class Table> void check_layout(const Call &init, Lay lay, Table table) {
  Call m = init;
  WsLayout ml;
  lay(ml, m);
  CHECK(ml.ok());
  for (const Arr &a : table(m)) CHECK(a.p == nullptr); // (a measuring pass places nothing)
  const size_t total = ml.used();
  std::vector<uint8_t> block(total + 256);
  uint8_t *base = block.data();
  Call c = init;
  WsLayout w(base, total);
  lay(w, c);
  CHECK(w.ok() && w.used() == total);
  size_t off = 0;
  int k = 0;
  for (const Arr &a : table(c)) {
    const size_t at = (size_t)(static_cast<const uint8_t *>(a.p) - base);
    CHECK(at == off && at % 256 == 0);
    CHECK(at + a.bytes <= total);
    off += align256(a.bytes);
    CHECK(at + a.bytes <= off);
    if (a.bytes) base[at] = base[at + a.bytes - 1] = (uint8_t)k; // (the sanitizer's view of it)
    ++k;
  }
  CHECK(off == total);
  CHECK(total > 0);
  Call s = init;
  WsLayout sl(base, total - 1);
  lay(sl, s);
  CHECK(!sl.ok());
}

static const uint64_t kCounts[] = {1, 2, 31, 32, 33, 257, 4095, 4096, 100000};
static const size_t kTmps[] = {0, 1, 513};

// frames.hip: the parse, compare, stamp-prep and stamp kernels index [i], i < n,
// and the CRC pass (ragged) writes one word per frame.
struct VerifyCall {
  FramesParse p;
  uint32_t *crc = nullptr;
  uint64_t n = 0;
};
static long check_verify() {
  long layouts = 0;
  for (uint64_t n : kCounts) {
    VerifyCall v;
    v.n = n;
    check_layout(
        v, [](WsLayout &w, VerifyCall &c) { verify_ws_layout(w, c.p, c.crc, c.n); },
        [](const VerifyCall &c) {
          return std::vector<Arr>{
              {c.p.body_off, c.n * 8}, {c.p.body_len, c.n * 4}, {c.p.hdr_crc, c.n * 4}, {c.crc, c.n * 4}, {c.p.pre, c.n}};
        });
    ++layouts;
  }
  return layouts;
}
struct StampCall {
  FramesStamp p;
  uint32_t *crc = nullptr;
  uint64_t n = 0;
};
static long check_stamp() {
  long layouts = 0;
  for (uint64_t n : kCounts) {
    StampCall v;
    v.n = n;
    check_layout(
        v, [](WsLayout &w, StampCall &c) { stamp_ws_layout(w, c.p, c.crc, c.n); },
        [](const StampCall &c) {
          return std::vector<Arr>{{c.p.body_off, c.n * 8}, {c.p.len_eff, c.n * 4}, {c.crc, c.n * 4}, {c.p.pre, c.n}};
        });
    ++layouts;
  }
  return layouts;
}

// The stages with a scan: the call and its scan size.
template <class Args> struct Scanned {
  Args a;
  size_t tmp = 0;
};

// frames_pack.hip: the size pass writes sizes, src_off, src_len, pre [i], i < n;
// the exclusive scan (frames_scan.hip excl_scan) reads sizes [i] and writes
// offs [i], i <= n, over `tmp` words; the CRC pass writes crc [i]; the pack
// kernel and the finish pass read offs [e + 1], e < n.
static long check_pack() {
  long layouts = 0;
  for (uint64_t n : kCounts)
    for (size_t tmp : kTmps) {
      Scanned<PackArgs> v;
      v.a.n = n;
      v.tmp = tmp;
      check_layout(
          v, [](WsLayout &w, Scanned<PackArgs> &c) { pack_ws_layout(w, c.a, c.tmp); },
          [](const Scanned<PackArgs> &c) {
            const uint64_t n = c.a.n;
            return std::vector<Arr>{{c.a.sizes, n * 8},        {c.a.src_off, n * 8}, {c.a.offs, (n + 1) * 8},
                                    {c.a.scan_tmp, c.tmp * 8}, {c.a.src_len, n * 4}, {c.a.crc, n * 4},
                                    {c.a.pre, n}};
          });
      ++layouts;
    }
  return layouts;
}
// frames_unpack.hip: as the pack; ver and pre [i], i < n.
static long check_unpack() {
  long layouts = 0;
  for (uint64_t n : kCounts)
    for (size_t tmp : kTmps) {
      Scanned<UnpackArgs> v;
      v.a.n = n;
      v.tmp = tmp;
      check_layout(
          v, [](WsLayout &w, Scanned<UnpackArgs> &c) { unpack_ws_layout(w, c.a, c.tmp); },
          [](const Scanned<UnpackArgs> &c) {
            const uint64_t n = c.a.n;
            return std::vector<Arr>{{c.a.sizes, n * 8},        {c.a.src_off, n * 8}, {c.a.offs, (n + 1) * 8},
                                    {c.a.scan_tmp, c.tmp * 8}, {c.a.ver, n * 2},     {c.a.pre, n}};
          });
      ++layouts;
    }
  return layouts;
}
// frames_carry.hip, the long route: the plan pass writes cnt, src, dst, tail
// [c], c < nconn; the scan writes offs [c], c <= nconn; the chunk kernel reads
// offs [nconn] and the others at the connection it finds.
static long check_carry() {
  long layouts = 0;
  for (uint64_t nconn : kCounts)
    for (size_t tmp : kTmps) {
      Scanned<CarryArgs> v;
      v.a.nconn = nconn;
      v.tmp = tmp;
      check_layout(
          v, [](WsLayout &w, Scanned<CarryArgs> &c) { carry_ws_layout(w, c.a, c.tmp); },
          [](const Scanned<CarryArgs> &c) {
            const uint64_t n = c.a.nconn;
            return std::vector<Arr>{{c.a.cnt, n * 8}, {c.a.offs, (n + 1) * 8}, {c.a.src, n * 8},
                                    {c.a.dst, n * 8}, {c.a.tail, n * 8},       {c.a.scan_tmp, c.tmp * 8}};
          });
      ++layouts;
    }
  return layouts;
}
// frames_route.hip, the grouping passes: one workgroup per 256 entries; the
// count pass writes counts [k * nwg + wg], k < nmethods + 3 buckets; the scan
// writes offs over those cells and one more; the scatter pass reads offs
// [k * nwg], k <= nmethods + 3; the route kernel writes bucket [e], e < n.
static long check_route() {
  long layouts = 0;
  for (uint64_t n : kCounts)
    for (uint32_t nmethods : {0u, 1u, 256u})
      for (size_t tmp : kTmps) {
        Scanned<RouteArgs> v;
        v.a.n = n;
        v.a.nmethods = nmethods;
        v.tmp = tmp;
        check_layout(
            v, [](WsLayout &w, Scanned<RouteArgs> &c) { route_ws_layout(w, c.a, c.tmp); },
            [](const Scanned<RouteArgs> &c) {
              const uint64_t cells = (uint64_t)(c.a.nmethods + 3) * ((c.a.n + 255) / 256);
              return std::vector<Arr>{
                  {c.a.counts, cells * 8}, {c.a.offs, (cells + 1) * 8}, {c.a.scan_tmp, c.tmp * 8}, {c.a.bucket, c.a.n * 2}};
            });
        ++layouts;
      }
  return layouts;
}
// frames_reply.hip: as the unpack; code (32 bits) and meta (16 bits) [i], i < n.
static long check_reply() {
  long layouts = 0;
  for (uint64_t n : kCounts)
    for (size_t tmp : kTmps) {
      Scanned<ReplyArgs> v;
      v.a.n = n;
      v.tmp = tmp;
      check_layout(
          v, [](WsLayout &w, Scanned<ReplyArgs> &c) { reply_ws_layout(w, c.a, c.tmp); },
          [](const Scanned<ReplyArgs> &c) {
            const uint64_t n = c.a.n;
            return std::vector<Arr>{{c.a.sizes, n * 8},        {c.a.src_off, n * 8}, {c.a.offs, (n + 1) * 8},
                                    {c.a.scan_tmp, c.tmp * 8}, {c.a.code, n * 4},    {c.a.meta, n * 2}};
          });
      ++layouts;
    }
  return layouts;
}
// frames_values.hip: `unit` items per entry; the size pass writes sizes,
// src_off, meta, text0..2 [i * unit + k], k < unit, and pre [i]; the scan writes
// offs over items + 1 words; the work list of very long strings takes one
// record per item at the most (long_off, long_len, long_entry, long_bad) and
// one counter word.
static long check_values() {
  long layouts = 0;
  for (uint64_t n : kCounts)
    for (uint32_t unit : {1u, 3u, (uint32_t)RPC_ARGS_MAX_PARAMS})
      for (size_t tmp : kTmps) {
        Scanned<ValuesArgs> v;
        v.a.n = n;
        v.a.unit = unit;
        v.a.items = n * unit;
        v.tmp = tmp;
        check_layout(
            v, [](WsLayout &w, Scanned<ValuesArgs> &c) { values_ws_layout(w, c.a, c.tmp); },
            [](const Scanned<ValuesArgs> &c) {
              const uint64_t it = c.a.n * c.a.unit;
              return std::vector<Arr>{{c.a.sizes, it * 8},    {c.a.src_off, it * 8},    {c.a.offs, (it + 1) * 8},
                                      {c.a.scan_tmp, c.tmp * 8}, {c.a.text0, it * 8},   {c.a.text1, it * 8},
                                      {c.a.text2, it * 8},    {c.a.long_off, it * 8},   {c.a.meta, it * 4},
                                      {c.a.long_len, it * 4}, {c.a.long_entry, it * 4}, {c.a.long_bad, it * 4},
                                      {c.a.long_count, 4},    {c.a.pre, c.a.n}};
            });
        ++layouts;
      }
  return layouts;
}
// frames_request.hip: as the reply with a 32-bit meta word; the table pass
// writes name_word [m], m < nmethods <= RPC_ROUTE_MAX_METHODS.
static long check_request() {
  long layouts = 0;
  for (uint64_t n : kCounts)
    for (size_t tmp : kTmps) {
      Scanned<RequestArgs> v;
      v.a.n = n;
      v.tmp = tmp;
      check_layout(
          v, [](WsLayout &w, Scanned<RequestArgs> &c) { request_ws_layout(w, c.a, c.tmp); },
          [](const Scanned<RequestArgs> &c) {
            const uint64_t n = c.a.n;
            return std::vector<Arr>{{c.a.sizes, n * 8},        {c.a.src_off, n * 8}, {c.a.offs, (n + 1) * 8},
                                    {c.a.scan_tmp, c.tmp * 8}, {c.a.meta, n * 4},    {c.a.name_word, RPC_ROUTE_MAX_METHODS * 4}};
          });
      ++layouts;
    }
  return layouts;
}
// frames_resolve.hip, npending > 0: the table is 2^bits cells (emptied whole,
// probed under a mask of bits) and must keep half of them empty for a probe to
// end; slot_entry [s], s < npending, and slot [e], e < n, are the caller's or
// workspace; with `open` the finish pass writes flags [s], the scan offs
// [s], s <= npending, and the compaction reads offs [npending].
static long check_resolve() {
  static uint32_t callers[1]; // (stands for a caller's array: only its address is looked at)
  long layouts = 0;
  for (uint64_t count : kCounts)
    for (size_t tmp : kTmps)
      for (int cond = 0; cond < 16; ++cond) {
        const bool open = cond & 1, own_entry = cond & 2, own_slot = cond & 4, empty = cond & 8;
        Scanned<ResolveArgs> v;
        v.a.n = empty ? 0 : count;
        v.a.npending = (uint32_t)count;
        v.a.bits = resolve_table_bits(v.a.npending);
        CHECK((1ull << v.a.bits) >= 2ull * v.a.npending);
        v.a.open = open ? callers : nullptr;
        v.a.slot_entry = own_entry ? callers : nullptr;
        v.a.slot = own_slot ? callers : nullptr;
        v.tmp = open ? tmp : 0;
        check_layout(
            v, [](WsLayout &w, Scanned<ResolveArgs> &c) { resolve_ws_layout(w, c.a, c.tmp); },
            [&](const Scanned<ResolveArgs> &c) {
              const uint64_t np = c.a.npending;
              std::vector<Arr> t;
              if (open) {
                t.push_back({c.a.flags, np * 8});
                t.push_back({c.a.offs, (np + 1) * 8});
                t.push_back({c.a.scan_tmp, c.tmp * 8});
              } else {
                CHECK(!c.a.flags && !c.a.offs && !c.a.scan_tmp);
              }
              t.push_back({c.a.cells, (size_t)4 << c.a.bits});
              if (!own_entry) t.push_back({c.a.slot_entry, np * 4});
              else CHECK(c.a.slot_entry == callers);
              if (!own_slot && c.a.n) t.push_back({c.a.slot, c.a.n * 4});
              else CHECK(c.a.slot == (own_slot ? callers : nullptr));
              return t;
            });
        ++layouts;
      }
  return layouts;
}
// frames_scan.hip, every route: the units write conn_cnt [c], c < nconn; the
// scans run over `tmp` words; the reach pass indexes first_close [c], c < nconn,
// and frame_conn [i], i < frame_cap (its own where the caller gave none).
struct ScanCall {
  ScanArgs a;
  size_t tmp = 0;
  bool reach = false, own_conn = false;
  uint64_t *first_close = nullptr;
};
static long check_scan() {
  static uint32_t callers[1];
  long layouts = 0;
  for (uint64_t nconn : kCounts)
    for (size_t tmp : kTmps)
      for (int cond = 0; cond < 3; ++cond) { // plain; reach with the caller's frame_conn; reach with its own
        ScanCall v;
        v.a.nconn = nconn;
        v.a.frame_cap = 3 * nconn + 1;
        v.tmp = tmp;
        v.reach = cond >= 1;
        v.own_conn = cond == 2;
        v.a.frame_conn = v.own_conn ? nullptr : callers;
        check_layout(
            v, [](WsLayout &w, ScanCall &c) { scan_ws_layout(w, c.a, c.tmp, c.reach, c.own_conn, c.first_close); },
            [](const ScanCall &c) {
              std::vector<Arr> t{{c.a.conn_cnt, c.a.nconn * 8}, {c.a.scan_tmp, c.tmp * 8}};
              if (c.reach) t.push_back({c.first_close, c.a.nconn * 8});
              else CHECK(!c.first_close);
              if (c.own_conn) t.push_back({c.a.frame_conn, c.a.frame_cap * 4});
              else CHECK(c.a.frame_conn == callers);
              return t;
            });
        ++layouts;
      }
  return layouts;
}
// frames_scan.hip, the tiled route: conn_tiles [c], c < nconn; tbase [c],
// c <= nconn; nt_live one word (the layout reserves 32, a 256-byte line of its
// own: at least); tconn, tile_cnt [j], j < tile_cap; tpre [j], j <= tile_cap;
// level l < levels holds ceil(tile_cap / 8^l) maps of kScanMapLen 16-bit words
// and as many entries.  Tile caps that give 1, 2 and the maximum number of
// levels.
static int levels_of(uint64_t tile_cap) { // until one map is left (frames_scan.hip scan_levels_for)
  int levels = 1;
  for (uint64_t maps = (tile_cap + 7) / 8; maps > 1; maps = (maps + 7) / 8) ++levels;
  return levels;
}
static long check_scan_tiled() {
  CHECK(levels_of(8) == 1 && levels_of(9) == 2 && levels_of(4097) == (int)kScanMaxLevels + 1);
  long layouts = 0;
  for (uint64_t nconn : kCounts)
    for (uint64_t tile_cap : {(uint64_t)8, (uint64_t)9, (uint64_t)4097}) {
      ScanArgs v;
      v.nconn = nconn;
      v.tile_cap = tile_cap;
      v.levels = levels_of(tile_cap);
      check_layout(
          v, [](WsLayout &w, ScanArgs &a) { scan_tiled_ws_layout(w, a); },
          [](const ScanArgs &a) {
            std::vector<Arr> t{{a.conn_tiles, a.nconn * 8},   {a.tbase, (a.nconn + 1) * 8},  {a.nt_live, 8},
                               {a.tconn, a.tile_cap * 4},     {a.tile_cnt, a.tile_cap * 8}, {a.tpre, (a.tile_cap + 1) * 8}};
            uint64_t maps = a.tile_cap;
            for (int l = 0; l < a.levels; ++l, maps = (maps + 7) / 8) {
              t.push_back({a.maps[l], maps * (1024 + 12 + 1) * 2});
              t.push_back({a.entry[l], maps * 2});
            }
            for (int l = a.levels; l <= (int)kScanMaxLevels; ++l) CHECK(!a.maps[l] && !a.entry[l]);
            return t;
          });
      ++layouts;
    }
  return layouts;
}

int main() {
  printf("ok verify %ld layouts\n", check_verify());
  printf("ok stamp %ld layouts\n", check_stamp());
  printf("ok pack %ld layouts\n", check_pack());
  printf("ok unpack %ld layouts\n", check_unpack());
  printf("ok carry %ld layouts\n", check_carry());
  printf("ok route %ld layouts\n", check_route());
  printf("ok reply %ld layouts\n", check_reply());
  printf("ok values %ld layouts\n", check_values());
  printf("ok request %ld layouts\n", check_request());
  printf("ok resolve %ld layouts\n", check_resolve());
  printf("ok scan %ld layouts\n", check_scan());
  printf("ok scan_tiled %ld layouts\n", check_scan_tiled());
  return 0;
}
