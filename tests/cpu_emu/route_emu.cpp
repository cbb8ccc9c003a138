// tests/cpu_emu/route_emu.cpp -- CPU emulation of the frame route
// (rpc_amd/csrc/frames_route.hip) on the shared source of frames_route.h: the
// precheck, the staging rounds of a workgroup, the strict automaton over the
// staged bytes, the method compare, and the three grouping passes (per-wave
// ranks from ballots, bucket counts per workgroup, exclusive scan, scatter), run
// as the kernels run them (one loop iteration per workgroup, wave or lane), at
// the kernel's own staging size or at a small one.
//
//   route_emu <stage bytes> <mis> <types 0|1> <bodies file> <entries file>
//             <names file> <offsets file>
//
// entries file: text, "offset length type" per line (type ignored with types 0:
// the call without d_reply_types).  offsets file: the table's nmethods + 1
// words, one per line (empty: no methods).  mis: the low four address bits the
// body buffer pretends to have.  stdout: per entry "kind method id params_off
// params_len", then "order i ..." and "first g ...".
// The body reader aborts on any byte outside [0, bodies_bytes) and on a 16-byte
// load that is not aligned or not wholly inside; the staged reader aborts on a
// byte outside what the round staged; the table reader on a byte outside
// [0, method_bytes) or a word outside the table.
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
#include <string>
#include <vector>

#include "../../rpc_amd/csrc/frames_route.h"

using namespace rpccrc;

namespace {

[[noreturn]] void die(const char *what) {
  fprintf(stderr, "route_emu: %s\n", what);
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

struct Tab {
  const std::vector<uint32_t> *offs;
  const std::vector<uint8_t> *names;
  uint32_t off(uint32_t m) const {
    if (m >= offs->size()) die("table word read outside the table");
    return (*offs)[m];
  }
  uint32_t name(uint32_t p) const {
    if (p >= names->size()) die("name byte read outside [0, method_bytes)");
    return (*names)[p];
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
    fprintf(stderr, "usage: route_emu stage mis types bodies entries names offsets\n");
    return 2;
  }
  const uint32_t stage = (uint32_t)strtoul(argv[1], nullptr, 10);
  const uint32_t mis = (uint32_t)strtoul(argv[2], nullptr, 10) & 15u;
  const bool has_type = atoi(argv[3]) != 0;
  if (stage % 16 || stage < kRouteMaxBody + 32) die("stage must be a multiple of 16 that holds any one body");
  const std::vector<uint8_t> buf = slurp(argv[4]), names = slurp(argv[6]);
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, type, moff;
  {
    std::ifstream f(argv[5]);
    unsigned long long o, l, t;
    while (f >> o >> l >> t) off.push_back(o), len.push_back((uint32_t)l), type.push_back((uint32_t)t);
    std::ifstream g(argv[7]);
    while (g >> o) moff.push_back((uint32_t)o);
  }
  const uint64_t n = off.size(), bodies_bytes = buf.size();
  const uint32_t nmethods = moff.empty() ? 0 : (uint32_t)moff.size() - 1;
  const uint32_t method_bytes = (uint32_t)names.size();
  if (nmethods > kRouteMaxMethods || method_bytes > kRouteMaxMethodBytes) die("table over the limits");
  const Bodies src{&buf, mis};
  const Tab tab{&moff, &names};
  std::vector<RouteOut> out(n);
  std::vector<uint32_t> bucket(n);

  // ---- route kernel: one workgroup per kRouteEntries entries ----------------
  const uint64_t nwg = (n + kRouteEntries - 1) / kRouteEntries;
  std::vector<uint8_t> lds(stage);
  FILE *trace = getenv("RPC_EMU_STAGE_TRACE") ? fopen(getenv("RPC_EMU_STAGE_TRACE"), "w") : nullptr;
  for (uint64_t wg = 0; wg < nwg; ++wg) {
    bool pending[kRouteEntries] = {};
    for (uint32_t t = 0; t < kRouteEntries; ++t) {
      const uint64_t e = wg * kRouteEntries + t;
      if (e >= n) continue;
      // (the offset and the length are looked at only for a DATA entry)
      const bool data = !has_type || type[e] == kRouteTypeData;
      pending[t] = route_precheck(has_type, type[e], data ? off[e] : 0, data ? len[e] : 0, bodies_bytes, &out[e]);
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
      for (uint32_t t = 0; t < kRouteEntries; ++t) {
        if (!mine[t]) continue;
        const uint64_t e = wg * kRouteEntries + t;
        Staged body{&lds, blocks * 16u, (uint32_t)(off[e] + mis - w0)};
        out[e] = route_one(body, len[e], tab, nmethods, method_bytes);
        pending[t] = false;
      }
    }
  }
  for (uint64_t e = 0; e < n; ++e) {
    bucket[e] = route_bucket(out[e].kind, out[e].method, nmethods);
    printf("%u %u %u %u %u\n", out[e].kind, out[e].method, out[e].id, out[e].params_off, out[e].params_len);
  }

  // ---- groups: count, exclusive scan, scatter ----------------------------------
  const uint32_t nb = route_buckets(nmethods), waves = kRouteEntries / 64;
  std::vector<uint64_t> counts((uint64_t)nb * nwg, 0), offs((uint64_t)nb * nwg + 1, 0);
  std::vector<uint32_t> rank(n, 0);
  for (uint64_t wg = 0; wg < nwg; ++wg) {
    std::vector<std::vector<uint32_t>> s_cnt(waves, std::vector<uint32_t>(nb, 0));
    auto bucket_of = [&](uint32_t t) {
      const uint64_t e = wg * kRouteEntries + t;
      return e < n ? bucket[e] : kRouteNoBucket;
    };
    for (uint32_t wave = 0; wave < waves; ++wave) {
      uint64_t left = 0; // the ballot of the lanes with a bucket
      for (uint32_t l = 0; l < 64; ++l)
        if (bucket_of(wave * 64 + l) != kRouteNoBucket) left |= 1ull << l;
      while (left) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(left), b0 = bucket_of(wave * 64 + leader);
        uint64_t same = 0;
        for (uint32_t l = 0; l < 64; ++l)
          if (bucket_of(wave * 64 + l) == b0) same |= 1ull << l;
        for (uint32_t l = 0; l < 64; ++l)
          if ((same >> l) & 1u) rank[wg * kRouteEntries + wave * 64 + l] = route_wave_rank(same, l);
        s_cnt[wave][b0] = route_popc64(same);
        left &= ~same;
      }
    }
    for (uint32_t t = 0; t < kRouteEntries; ++t) {
      const uint32_t b = bucket_of(t);
      if (b == kRouteNoBucket) continue;
      for (uint32_t w = 0; w < t / 64; ++w) rank[wg * kRouteEntries + t] += s_cnt[w][b];
    }
    for (uint32_t k = 0; k < nb; ++k)
      for (uint32_t w = 0; w < waves; ++w) counts[(uint64_t)k * nwg + wg] += s_cnt[w][k];
  }
  for (uint64_t i = 0; i < counts.size(); ++i) offs[i + 1] = offs[i] + counts[i];
  const uint64_t total = offs[counts.size()];
  if (total > n) die("more grouped entries than entries");
  std::vector<int64_t> order(total, -1);
  for (uint64_t e = 0; e < n; ++e) {
    if (bucket[e] == kRouteNoBucket) continue;
    const uint64_t at = offs[(uint64_t)bucket[e] * nwg + e / kRouteEntries] + rank[e];
    if (at >= total) die("scatter outside the order");
    if (order[at] != -1) die("order slot written twice");
    order[at] = (int64_t)e;
  }
  printf("order");
  for (uint64_t i = 0; i < total; ++i) {
    if (order[i] < 0) die("order slot left out");
    printf(" %lld", (long long)order[i]);
  }
  printf("\nfirst");
  for (uint32_t k = 0; k <= nb; ++k) printf(" %llu", (unsigned long long)(nwg ? offs[(uint64_t)k * nwg] : 0));
  printf("\n");
  if (trace) fclose(trace);
  return 0;
}
