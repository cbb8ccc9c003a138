// tests/cpu_emu/resolve_emu.cpp -- CPU emulation of the frame resolve
// (rpc_amd/csrc/frames_resolve.hip) on the shared source of frames_resolve.h
// and frames_route.h: the precheck, the staging rounds of a workgroup, the
// strict automaton with the reply's key policy over the staged bytes, and the
// join's passes (table: a compare-and-swap per probe; probe and claim: the
// lowest entry per slot; finish: MATCHED / DUPLICATE off slot_entry, the open
// slots flagged, scanned and compacted), run as the kernels run them, at the
// kernel's own staging size or at a small one.
//
//   resolve_emu <stage bytes> <mis> <types 0|1> <descending 0|1>
//               <bodies file> <entries file> <pending file>
//
// entries file: text, "offset length type" per line (type ignored with types 0:
// the call without d_reply_types).  pending file: one id per line.  mis: the low
// four address bits the body buffer pretends to have.  descending: workgroups,
// lanes and slots are visited from the last to the first in every pass (the
// outputs must not depend on it).  stdout: per entry "kind id result_off
// result_len error_off error_len slot", then "slot_entry ..." and "open ...".
// The body reader aborts on any byte outside [0, bodies_bytes) and on a 16-byte
// load that is not aligned or not wholly inside; the staged reader aborts on a
// byte outside what the round staged; the table's readers on a cell outside the
// table and an id outside [0, npending).
// With RPC_EMU_STAGE_TRACE=<file> in the environment the staging rounds are
// written there as well, one line per round: "workgroup w0 bodies-taken
// blocks-read-bytewise" (w0 in aligned space; tests/stage_cases.py, trace()).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../rpc_amd/csrc/frames_resolve.h"

using namespace rpccrc;

namespace {

[[noreturn]] void die(const char *what) {
  fprintf(stderr, "resolve_emu: %s\n", what);
  abort();
}

struct Bodies { // the buffer at a pretended address
  const std::vector<uint8_t> *b;
  uint32_t mis;
  uint8_t byte(uint64_t p) const {
    if (p >= b->size()) die("body byte read outside [0, bodies_bytes)");
    return (*b)[p];
  }
  void block16(uint64_t p, uint8_t *dst) const {
    if ((mis + p) & 15u) die("block16 at an unaligned address");
    if (p > b->size() || b->size() - p < 16) die("block read outside [0, bodies_bytes)");
    memcpy(dst, b->data() + p, 16);
  }
};

struct Staged { // LdsBody of the kernels: word-wise walk, bytes again through at()
  const std::vector<uint8_t> *lds;
  uint32_t staged; // bytes the round wrote
  uint32_t base;
  uint32_t pos = 0, w = 0;
  uint32_t word(uint32_t p) const {
    if (p + 4 > staged) die("staged word read outside the round's bytes");
    uint32_t v;
    memcpy(&v, lds->data() + p, 4);
    return v;
  }
  uint32_t next() {
    const uint32_t p = base + pos;
    if ((p & 3u) == 0 || pos == 0) w = word(p & ~3u);
    ++pos;
    return (w >> (8 * (p & 3u))) & 0xFFu;
  }
  bool aligned() const { return ((base + pos) & 3u) == 0; }
  uint32_t word() const {
    if (!aligned()) die("whole-word step at an unaligned staged byte");
    return word(base + pos);
  }
  void skip4() { pos += 4; }
  uint32_t at(uint32_t i) const {
    const uint32_t p = base + i;
    return (word(p & ~3u) >> (8 * (p & 3u))) & 0xFFu;
  }
};

struct Table { // the join's cells and the caller's ids
  std::vector<uint32_t> *cells;
  const std::vector<uint32_t> *ids;
  uint32_t operator()(uint32_t c, uint32_t expect, uint32_t value) { // the compare-and-swap
    if (c >= cells->size()) die("cell written outside the table");
    const uint32_t old = (*cells)[c];
    if (old == expect) (*cells)[c] = value;
    return old;
  }
  uint32_t cell(uint32_t c) const {
    if (c >= cells->size()) die("cell read outside the table");
    return (*cells)[c];
  }
  uint32_t id(uint32_t s) const {
    if (s >= ids->size()) die("id read outside [0, npending)");
    return (*ids)[s];
  }
};

std::vector<uint8_t> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot open an input file");
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

} // namespace

int main(int argc, char **argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: resolve_emu stage mis types descending bodies entries pending\n");
    return 2;
  }
  const uint32_t stage = (uint32_t)strtoul(argv[1], nullptr, 10);
  const uint32_t mis = (uint32_t)strtoul(argv[2], nullptr, 10) & 15u;
  const bool has_type = atoi(argv[3]) != 0, desc = atoi(argv[4]) != 0;
  if (stage % 16 || stage < kRouteMaxBody + 32) die("stage must be a multiple of 16 that holds any one body");
  const std::vector<uint8_t> buf = slurp(argv[5]);
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, type, ids;
  {
    std::ifstream f(argv[6]);
    unsigned long long o, l, t;
    while (f >> o >> l >> t) off.push_back(o), len.push_back((uint32_t)l), type.push_back((uint32_t)t);
    std::ifstream g(argv[7]);
    while (g >> o) ids.push_back((uint32_t)o);
  }
  const uint64_t n = off.size(), bodies_bytes = buf.size();
  const uint32_t npending = (uint32_t)ids.size();
  if (npending > kResolveMaxPending) die("too many pending ids");
  const Bodies src{&buf, mis};
  // i-th of count in the visiting order
  const auto visit = [desc](uint64_t i, uint64_t count) { return desc ? count - 1 - i : i; };

  // ---- table pass ---------------------------------------------------------------
  const uint32_t bits = resolve_table_bits(npending);
  std::vector<uint32_t> cells(npending ? (size_t)1 << bits : 0, kResolveEmpty);
  if (npending && cells.size() < 2ull * npending) die("table below two cells per slot");
  std::vector<uint32_t> slot_entry(npending, kResolveNoSlot);
  Table table{&cells, &ids};
  for (uint32_t k = 0; k < npending; ++k) {
    const uint32_t s = (uint32_t)visit(k, npending);
    resolve_insert(table, s, ids[s], bits);
  }

  // ---- resolve kernel: one workgroup per kRouteEntries entries ---------------
  std::vector<ResolveOut> out(n);
  std::vector<uint32_t> slot(n, kResolveNoSlot);
  const auto put = [&](uint64_t e, ResolveOut o) { // put() of the kernel
    if (o.kind == kResolveUnknown && npending) {
      slot[e] = resolve_probe(table, table, o.id, bits);
      if (slot[e] != kResolveNoSlot) {
        if (slot[e] >= npending) die("slot outside [0, npending)");
        slot_entry[slot[e]] = std::min(slot_entry[slot[e]], (uint32_t)e); // atomicMin
        o.kind = kResolveMatched;
      }
    }
    out[e] = o;
  };
  const uint64_t nwg = (n + kRouteEntries - 1) / kRouteEntries;
  std::vector<uint8_t> lds(stage);
  FILE *trace = getenv("RPC_EMU_STAGE_TRACE") ? fopen(getenv("RPC_EMU_STAGE_TRACE"), "w") : nullptr;
  for (uint64_t w = 0; w < nwg; ++w) {
    const uint64_t wg = visit(w, nwg);
    bool pending[kRouteEntries] = {};
    for (uint32_t k = 0; k < kRouteEntries; ++k) {
      const uint32_t t = (uint32_t)visit(k, kRouteEntries);
      const uint64_t e = wg * kRouteEntries + t;
      if (e >= n) continue;
      // (the offset and the length are looked at only for a DATA entry)
      const bool data = !has_type || type[e] == kRouteTypeData;
      ResolveOut o;
      pending[t] = resolve_precheck(has_type, type[e], data ? off[e] : 0, data ? len[e] : 0, bodies_bytes, &o);
      if (!pending[t]) put(e, o);
    }
    for (;;) {
      uint32_t first = 0xFFFFFFFFu;
      for (uint32_t t = 0; t < kRouteEntries; ++t)
        if (pending[t]) first = std::min(first, t);
      if (first == 0xFFFFFFFFu) break;
      const uint64_t w0 = (off[wg * kRouteEntries + first] + mis) & ~(uint64_t)15;
      bool mine[kRouteEntries] = {};
      uint32_t end = 0;
      for (uint32_t t = 0; t < kRouteEntries; ++t) {
        if (!pending[t]) continue;
        const uint64_t e = wg * kRouteEntries + t, x0 = off[e] + mis;
        mine[t] = x0 >= w0 && x0 + len[e] <= w0 + stage;
        if (mine[t]) end = std::max(end, (uint32_t)(x0 + len[e] - w0));
      }
      const uint32_t blocks = (end + 15u) / 16u;
      const uint64_t lim = bodies_bytes + mis;
      std::fill(lds.begin(), lds.end(), (uint8_t)0xA5);
      uint32_t edge = 0; // blocks read bytewise
      for (uint32_t k = 0; k < blocks; ++k) {
        const uint64_t x = w0 + (uint64_t)k * 16u;
        if (x >= mis && x + 16u <= lim) {
          src.block16(x - mis, lds.data() + 16 * k);
        } else {
          ++edge;
          for (uint32_t b = 0; b < 16; ++b) lds[16 * k + b] = (x + b >= mis && x + b < lim) ? src.byte(x + b - mis) : 0;
        }
      }
      if (trace)
        fprintf(trace, "%llu %llu %u %u\n", (unsigned long long)wg, (unsigned long long)w0,
                (uint32_t)std::count(mine, mine + kRouteEntries, true), edge);
      for (uint32_t k = 0; k < kRouteEntries; ++k) {
        const uint32_t t = (uint32_t)visit(k, kRouteEntries);
        if (!mine[t]) continue;
        const uint64_t e = wg * kRouteEntries + t;
        Staged body{&lds, blocks * 16u, (uint32_t)(off[e] + mis - w0)};
        put(e, resolve_one(body, len[e]));
        pending[t] = false;
      }
    }
  }

  // ---- finish pass, exclusive scan, compaction ------------------------------------
  std::vector<uint64_t> flags(npending), offs((size_t)npending + 1, 0);
  for (uint64_t k = 0; k < std::max<uint64_t>(n, npending); ++k) {
    const uint64_t i = visit(k, std::max<uint64_t>(n, npending));
    if (i < n && npending && slot[i] != kResolveNoSlot) out[i].kind = resolve_final(slot_entry[slot[i]], (uint32_t)i);
    if (i < npending) flags[i] = slot_entry[i] == kResolveNoSlot ? 1u : 0u;
  }
  for (uint32_t s = 0; s < npending; ++s) offs[s + 1] = offs[s] + flags[s];
  std::vector<int64_t> open(offs[npending], -1);
  for (uint32_t k = 0; k < npending; ++k) {
    const uint32_t s = (uint32_t)visit(k, npending);
    if (!flags[s]) continue;
    if (offs[s] >= open.size() || open[offs[s]] != -1) die("open list written outside or twice");
    open[offs[s]] = s;
  }

  for (uint64_t e = 0; e < n; ++e)
    printf("%u %u %u %u %u %u %u\n", out[e].kind, out[e].id, out[e].result_off, out[e].result_len, out[e].error_off,
           out[e].error_len, slot[e]);
  printf("slot_entry");
  for (uint32_t s = 0; s < npending; ++s) printf(" %u", slot_entry[s]);
  printf("\nopen");
  for (int64_t s : open) {
    if (s < 0) die("open slot left out");
    printf(" %lld", (long long)s);
  }
  printf("\n");
  if (trace) fclose(trace);
  return 0;
}
