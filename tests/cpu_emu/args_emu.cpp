// tests/cpu_emu/args_emu.cpp -- CPU emulation of the frame args
// (rpc_amd/csrc/frames_args.hip) on the shared source of frames_args.h: the
// precheck, the staging rounds of a workgroup over the `params` spans, the
// strict walk over the staged bytes with its key compares and conversions, and
// the slot stores, run as the kernel runs them (one loop iteration per
// workgroup or lane), at the kernel's own staging size or at a small one.
//
//   args_emu run <stage bytes> <mis> <width> <bodies file> <entries file> <schema file>
//   args_emu num <numbers file>
//
// entries file: text, "body_off body_len kind method params_off params_len" per
// line.  schema file: four lines, "first w ...", "types t ...", "noff w ...",
// "names <hex>" (nmethods, nparams and name_bytes are the arrays' sizes).  mis:
// the low four address bits the body buffer pretends to have.  stdout: per
// entry "status reply_status slot ...", width slots.
// num: one JSON number per line; stdout per line the double's 16 hex digits or
// DEFER (args_number alone, over a flat body).
// The body reader aborts on any byte outside [0, bodies_bytes) and on a 16-byte
// load that is not aligned or not wholly inside; the staged reader aborts on a
// byte outside what the round staged; the schema reader on a word or byte
// outside its array; the table reader outside the table.
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

#include "../../rpc_amd/csrc/frames_args.h"

using namespace rpccrc;

namespace {

[[noreturn]] void die(const char *what) {
  fprintf(stderr, "args_emu: %s\n", what);
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

struct Flat { // a number string for args_number
  const std::string *s;
  uint32_t at(uint32_t i) const {
    if (i >= s->size()) die("number byte read outside the string");
    return (uint8_t)(*s)[i];
  }
};

struct Schema {
  std::vector<uint32_t> firsts, types, noff;
  std::vector<uint8_t> names;
  uint32_t first(uint32_t m) const {
    if (m >= firsts.size()) die("CSR word read outside nmethods + 1");
    return firsts[m];
  }
  uint32_t type(uint32_t p) const {
    if (p >= types.size()) die("type read outside nparams");
    return types[p];
  }
  uint32_t name_off(uint32_t p) const {
    if (p >= noff.size()) die("name word read outside nparams + 1");
    return noff[p];
  }
  uint32_t name(uint32_t b) const {
    if (b >= names.size()) die("name byte read outside [0, name_bytes)");
    return names[b];
  }
};

struct Sink {
  std::vector<uint64_t> *slots;
  uint64_t n, e;
  uint32_t width;
  void put(uint32_t k, uint64_t v) const {
    if (k >= width) die("slot stored outside the width");
    (*slots)[(uint64_t)k * n + e] = v;
  }
};

std::vector<uint8_t> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot open an input file");
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int run_numbers(const char *path) {
  std::ifstream f(path);
  if (!f) die("cannot open the numbers file");
  std::string line;
  while (std::getline(f, line)) {
    const Flat body{&line};
    uint64_t bits = 0;
    if (args_number(body, 0, (uint32_t)line.size(), Pow{}, &bits)) printf("%016llx\n", (unsigned long long)bits);
    else printf("DEFER\n");
  }
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "num")) return run_numbers(argv[2]);
  if (argc != 8 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: args_emu run stage mis width bodies entries schema | args_emu num numbers\n");
    return 2;
  }
  const uint32_t stage = (uint32_t)strtoul(argv[2], nullptr, 10);
  const uint32_t mis = (uint32_t)strtoul(argv[3], nullptr, 10) & 15u;
  const uint32_t width = (uint32_t)strtoul(argv[4], nullptr, 10);
  if (stage % 16 || stage < kRouteMaxBody + 32) die("stage must be a multiple of 16 that holds any one span");
  if (width == 0 || width > kArgsMaxParams) die("width outside 1 .. 8");
  const std::vector<uint8_t> buf = slurp(argv[5]);
  std::vector<uint64_t> boff;
  std::vector<uint32_t> blen, kind, method, poff, plen;
  {
    std::ifstream f(argv[6]);
    unsigned long long o, l, k, m, po, pl;
    while (f >> o >> l >> k >> m >> po >> pl) {
      boff.push_back(o), blen.push_back((uint32_t)l), kind.push_back((uint32_t)k), method.push_back((uint32_t)m);
      poff.push_back((uint32_t)po), plen.push_back((uint32_t)pl);
    }
  }
  Schema sc;
  {
    std::ifstream f(argv[7]);
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream is(line);
      std::string tag;
      is >> tag;
      unsigned long long v;
      if (tag == "first") while (is >> v) sc.firsts.push_back((uint32_t)v);
      else if (tag == "types") while (is >> v) sc.types.push_back((uint32_t)v);
      else if (tag == "noff") while (is >> v) sc.noff.push_back((uint32_t)v);
      else if (tag == "names") {
        std::string hex;
        is >> hex;
        for (size_t i = 0; i + 1 < hex.size(); i += 2) sc.names.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
      }
    }
  }
  const uint64_t n = boff.size(), bodies_bytes = buf.size();
  const uint32_t nmethods = sc.firsts.empty() ? 0 : (uint32_t)sc.firsts.size() - 1;
  const uint32_t nparams = (uint32_t)sc.types.size(), name_bytes = (uint32_t)sc.names.size();
  if (nmethods > kRouteMaxMethods || nparams > kArgsMaxSchemaParams || name_bytes > kArgsMaxNameBytes)
    die("schema over the limits");
  const Bodies src{&buf, mis};
  std::vector<uint64_t> slots((uint64_t)width * n, 0xDEADBEEFDEADBEEFull);
  std::vector<uint32_t> status(n, 0xEE);
  std::vector<int32_t> reply(n, 0x7EEE);
  const auto finish = [&](uint64_t e, uint8_t st, uint32_t used) {
    status[e] = st;
    reply[e] = args_reply_status(st);
    for (uint32_t k = st == kArgsOk ? used : 0u; k < width; ++k) slots[(uint64_t)k * n + e] = 0;
  };

  const uint64_t nwg = (n + kRouteEntries - 1) / kRouteEntries;
  std::vector<uint8_t> lds(stage);
  FILE *trace = getenv("RPC_EMU_STAGE_TRACE") ? fopen(getenv("RPC_EMU_STAGE_TRACE"), "w") : nullptr;
  for (uint64_t wg = 0; wg < nwg; ++wg) {
    bool pending[kRouteEntries] = {};
    uint64_t off[kRouteEntries] = {};
    uint32_t len[kRouteEntries] = {}, base[kRouteEntries] = {}, f0[kRouteEntries] = {}, f1[kRouteEntries] = {};
    for (uint32_t t = 0; t < kRouteEntries; ++t) {
      const uint64_t e = wg * kRouteEntries + t;
      if (e >= n) continue;
      // (only for a CALL entry is anything else of the entry looked at)
      const bool call = kind[e] == kRouteCall;
      base[t] = call ? poff[e] : 0, len[t] = call ? plen[e] : 0;
      const uint8_t st = args_precheck((uint8_t)kind[e], call ? method[e] : 0, sc, nmethods, nparams, name_bytes, width,
                                       call ? boff[e] : 0, call ? blen[e] : 0, base[t], len[t], bodies_bytes, &f0[t], &f1[t]);
      pending[t] = st == kArgsWalk;
      if (pending[t]) off[t] = boff[e] + base[t];
      else finish(e, st, 0);
    }
    for (;;) {
      uint32_t first = 0xFFFFFFFFu;
      for (uint32_t t = 0; t < kRouteEntries; ++t)
        if (pending[t]) first = std::min(first, t);
      if (first == 0xFFFFFFFFu) break;
      const uint64_t w0 = (off[first] + mis) & ~(uint64_t)15;
      bool mine[kRouteEntries] = {};
      uint32_t end = 0;
      for (uint32_t t = 0; t < kRouteEntries; ++t) {
        if (!pending[t]) continue;
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
        Staged body{&lds, blocks * 16u, (uint32_t)(off[t] + mis - w0)};
        const Sink sink{&slots, n, e, width};
        const uint8_t st = args_one(body, len[t], base[t], sc, f0[t], f1[t], Pow{}, sink);
        finish(e, st, f1[t] - f0[t]);
        pending[t] = false;
      }
    }
  }
  for (uint64_t e = 0; e < n; ++e) {
    printf("%u %d", status[e], reply[e]);
    for (uint32_t k = 0; k < width; ++k) printf(" %llu", (unsigned long long)slots[(uint64_t)k * n + e]);
    printf("\n");
  }
  if (trace) fclose(trace);
  return 0;
}
