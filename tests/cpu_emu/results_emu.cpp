// tests/cpu_emu/results_emu.cpp -- CPU emulation of the frame results
// (rpc_amd/csrc/frames_results.hip) on the shared source of frames_results.h:
// the precheck, the staging rounds of a workgroup over the bodies, the strict
// walk over the two spans of each staged body with the conversions, the
// per-slot part and the count, run as the kernels run them (one loop iteration
// per workgroup or lane), at the kernel's own staging size or at a small one.
//
//   results_emu run <stage bytes> <mis> <bodies file> <entries file> <schema file>
//
// entries file: text, "body_off body_len kind slot result_off result_len
// error_off error_len" per line.  schema file: three lines, "pending m ...",
// "types t ...", "slot_entry e ..." (npending and nmethods are the arrays'
// sizes; slot_entry has npending words).  mis: the low four address bits the
// body buffer pretends to have.  stdout: per entry "status value error_status
// error_code error_message", then per slot "status value error_status
// error_code str_base", then the count of deferred entries.
// The body reader aborts on any byte outside [0, bodies_bytes) and on a 16-byte
// load that is not aligned or not wholly inside; the staged reader aborts on a
// byte outside what the round staged; the schema readers on a word outside
// their arrays, the column readers on an entry outside [0, n).
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
#include <sstream>
#include <string>
#include <vector>

#include "../../rpc_amd/csrc/frames_results.h"

using namespace rpccrc;

namespace {

[[noreturn]] void die(const char *what) {
  fprintf(stderr, "results_emu: %s\n", what);
  abort();
}

const uint64_t kPow10[] = {RPCCRC_POW10_WORDS};
struct Pow {
  uint64_t word(uint32_t i) const {
    if (i >= sizeof(kPow10) / sizeof(kPow10[0])) die("power word read outside the table");
    return kPow10[i];
  }
};

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

struct Staged { // LdsBody of the kernel: word-wise walk, bytes again through at()
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
struct View { // a span of the staged body: the base moved by the span's offset
  const Staged *body;
  Staged operator()(uint32_t off) const { return Staged{body->lds, body->staged, body->base + off}; }
};

struct Pending {
  const std::vector<uint32_t> *m;
  uint32_t method(uint32_t s) const {
    if (s >= m->size()) die("pending method read outside npending");
    return (*m)[s];
  }
};
struct Types {
  const std::vector<uint32_t> *t;
  uint32_t type(uint32_t m) const {
    if (m >= t->size()) die("result type read outside nmethods");
    return (*t)[m];
  }
};
struct Cols {
  const std::vector<uint32_t> *kinds, *slots;
  uint32_t kind(uint32_t e) const {
    if (e >= kinds->size()) die("kind read outside [0, n)");
    return (*kinds)[e];
  }
  uint32_t slot(uint32_t e) const {
    if (e >= slots->size()) die("slot read outside [0, n)");
    return (*slots)[e];
  }
};

std::vector<uint8_t> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot open an input file");
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

} // namespace

int main(int argc, char **argv) {
  if (argc != 7 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: results_emu run stage mis bodies entries schema\n");
    return 2;
  }
  const uint32_t stage = (uint32_t)strtoul(argv[2], nullptr, 10);
  const uint32_t mis = (uint32_t)strtoul(argv[3], nullptr, 10) & 15u;
  if (stage % 16 || stage < kRouteMaxBody + 32) die("stage must be a multiple of 16 that holds any one body");
  const std::vector<uint8_t> buf = slurp(argv[4]);
  std::vector<uint64_t> boff;
  std::vector<uint32_t> blen, kind, slot, roff, rlen, eoff, elen;
  {
    std::ifstream f(argv[5]);
    unsigned long long o, l, k, s, ro, rl, eo, el;
    while (f >> o >> l >> k >> s >> ro >> rl >> eo >> el) {
      boff.push_back(o), blen.push_back((uint32_t)l), kind.push_back((uint32_t)k), slot.push_back((uint32_t)s);
      roff.push_back((uint32_t)ro), rlen.push_back((uint32_t)rl), eoff.push_back((uint32_t)eo), elen.push_back((uint32_t)el);
    }
  }
  std::vector<uint32_t> pending, types, slot_entry;
  {
    std::ifstream f(argv[6]);
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream is(line);
      std::string tag;
      is >> tag;
      unsigned long long v;
      std::vector<uint32_t> *dst = tag == "pending" ? &pending : tag == "types" ? &types : tag == "slot_entry" ? &slot_entry : nullptr;
      if (!dst) die("unknown schema line");
      while (is >> v) dst->push_back((uint32_t)v);
    }
  }
  const uint64_t n = boff.size(), bodies_bytes = buf.size();
  const uint32_t npending = (uint32_t)pending.size(), nmethods = (uint32_t)types.size();
  if (slot_entry.size() != npending) die("slot_entry needs npending words");
  if (npending > kResolveMaxPending || nmethods > kRouteMaxMethods) die("schema over the limits");
  const Bodies src{&buf, mis};
  const Pending pm{&pending};
  const Types ty{&types};

  std::vector<ResultsOut> out(n, ResultsOut{0xEE, 0xEE, 0xDEADBEEFDEADBEEFull, 0x7EEE, 0xDEADBEEFDEADBEEFull});
  struct SlotOut {
    uint32_t status, error_status;
    uint64_t value;
    int32_t error_code;
    uint64_t str_base;
    uint32_t writes;
  };
  std::vector<SlotOut> slots(npending, SlotOut{0xEE, 0xEE, 0xDEADBEEFDEADBEEFull, 0x7EEE, 0xDEADBEEFDEADBEEFull, 0});
  uint32_t ndefer = 0;
  const auto put = [&](uint64_t e, const ResultsOut &o, bool own) {
    out[e] = o;
    if (o.status == kResultsDefer || o.error_status == kResultsDefer) ++ndefer;
    if (!own) return;
    SlotOut &s = slots[slot[e]];
    s = SlotOut{o.status, o.error_status, o.value, o.error_code, boff[e], s.writes + 1};
  };

  // the open-slot pass
  for (uint32_t s = 0; s < npending; ++s) {
    if (results_completes(slot_entry[s], n, Cols{&kind, &slot}, s)) continue;
    slots[s] = SlotOut{0, 0, 0, 0, 0, slots[s].writes + 1};
  }

  const uint64_t nwg = (n + kRouteEntries - 1) / kRouteEntries;
  std::vector<uint8_t> lds(stage);
  FILE *trace = getenv("RPC_EMU_STAGE_TRACE") ? fopen(getenv("RPC_EMU_STAGE_TRACE"), "w") : nullptr;
  for (uint64_t wg = 0; wg < nwg; ++wg) {
    bool pending_lane[kRouteEntries] = {}, own[kRouteEntries] = {};
    uint64_t off[kRouteEntries] = {};
    uint32_t len[kRouteEntries] = {}, type[kRouteEntries] = {};
    for (uint32_t t = 0; t < kRouteEntries; ++t) {
      const uint64_t e = wg * kRouteEntries + t;
      if (e >= n) continue;
      // (only for a MATCHED entry is anything else of the entry looked at)
      const bool m = kind[e] == kResolveMatched;
      if (m) {
        off[t] = boff[e], len[t] = blen[e];
        own[t] = slot[e] < npending && slot_entry[slot[e]] == (uint32_t)e;
      }
      const uint8_t st = results_precheck((uint8_t)kind[e], m ? slot[e] : 0, pm, npending, ty, nmethods, off[t], len[t],
                                          m ? roff[e] : 0, m ? rlen[e] : 0, m ? eoff[e] : 0, m ? elen[e] : 0, bodies_bytes,
                                          &type[t]);
      ResultsOut o = results_plain(st);
      if (st == kResultsWalk) pending_lane[t] = results_unread(len[t], rlen[e], elen[e], &o);
      if (!pending_lane[t]) put(e, o, own[t]);
    }
    for (;;) {
      uint32_t first = 0xFFFFFFFFu;
      for (uint32_t t = 0; t < kRouteEntries; ++t)
        if (pending_lane[t]) first = std::min(first, t);
      if (first == 0xFFFFFFFFu) break;
      const uint64_t w0 = (off[first] + mis) & ~(uint64_t)15;
      bool mine[kRouteEntries] = {};
      uint32_t end = 0;
      for (uint32_t t = 0; t < kRouteEntries; ++t) {
        if (!pending_lane[t]) continue;
        const uint64_t x0 = off[t] + mis;
        mine[t] = x0 >= w0 && x0 + len[t] <= w0 + stage;
        if (mine[t]) end = std::max(end, (uint32_t)(x0 + len[t] - w0));
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
      for (uint32_t t = 0; t < kRouteEntries; ++t) {
        if (!mine[t]) continue;
        const uint64_t e = wg * kRouteEntries + t;
        const Staged body{&lds, blocks * 16u, (uint32_t)(off[t] + mis - w0)};
        put(e, results_walk(View{&body}, type[t], roff[e], rlen[e], eoff[e], elen[e], Pow{}), own[t]);
        pending_lane[t] = false;
      }
    }
  }
  for (uint64_t e = 0; e < n; ++e)
    printf("%u %llu %u %d %llu\n", out[e].status, (unsigned long long)out[e].value, out[e].error_status, out[e].error_code,
           (unsigned long long)out[e].error_message);
  for (uint32_t s = 0; s < npending; ++s) {
    if (slots[s].writes != 1) die("a slot written by no pass, or by more than one lane");
    printf("%u %llu %u %d %llu\n", slots[s].status, (unsigned long long)slots[s].value, slots[s].error_status,
           slots[s].error_code, (unsigned long long)slots[s].str_base);
  }
  printf("%u\n", ndefer);
  if (trace) fclose(trace);
  return 0;
}
