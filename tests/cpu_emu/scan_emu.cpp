// tests/cpu_emu/scan_emu.cpp -- CPU emulation of the frame scan
// (rpc_amd/csrc/frames_scan.hip) on the shared source of frames_scan.h: the
// one-header step, the tile maps, up-sweep, down-sweep, count and emit, run
// stage by stage as the kernels run them (one loop iteration per workgroup or
// lane), at the kernels' own T and G or at a small instantiation that makes a
// ~1 MiB connection need four or more levels.
//
//   scan_emu <T> <G> <flags> <tiled_min> <tile_cap> <stream file> <conns file>
//
// conns file: text, "off len" per line.  Output: "levels L", then per
// connection "state consumed n off_0 ... off_{n-1}" (absolute offsets).
// The tile reader aborts on any byte read outside the tile and its 7-byte halo
// or outside the connection.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../rpc_amd/csrc/frames_scan.h"

using namespace rpccrc;

namespace {

[[noreturn]] void die(const char *what) {
  fprintf(stderr, "scan_emu: %s\n", what);
  abort();
}

struct ConnRd { // the serial walk's reader: the connection's bytes, nothing else
  const uint8_t *b;
  uint64_t len;
  uint8_t operator()(uint64_t q) const {
    if (q >= len) die("walk read outside the connection");
    return b[q];
  }
};
struct TileRd { // the tile pass's LDS image: the tile and its halo
  const uint8_t *b;
  uint64_t len, t0, span;
  uint8_t operator()(uint64_t q) const {
    if (q < t0 || q - t0 >= span || q >= len) die("tile pass read outside the tile and its halo");
    return b[q];
  }
};
struct VecSink {
  std::vector<uint64_t> *out;
  uint64_t base, conn_off;
  void operator()(uint64_t k, uint64_t q) const { (*out)[base + k] = conn_off + q; }
};

std::vector<uint64_t> excl_scan(const std::vector<uint64_t> &in) {
  std::vector<uint64_t> out(in.size() + 1, 0);
  for (size_t i = 0; i < in.size(); ++i) out[i + 1] = out[i] + in[i];
  return out;
}

template <uint32_t T, uint32_t G>
int run(int flags, uint64_t tiled_min, uint64_t tile_cap, const std::vector<uint8_t> &stream,
        const std::vector<uint64_t> &coff, const std::vector<uint64_t> &clen) {
  static_assert(T >= kScanEntries, "an exit must land inside the next tile");
  const uint64_t nconn = coff.size(), sb = stream.size();
  auto inside = [&](uint64_t c) { return coff[c] <= sb && clen[c] <= sb - coff[c]; };
  if (flags & kScanLiftCap) tile_cap = 0; // (the API's rule)
  // classify, tile bases, live tiles
  std::vector<uint64_t> want(nconn, 0);
  for (uint64_t c = 0; c < nconn; ++c)
    if (tile_cap && inside(c) && clen[c] > tiled_min) want[c] = std::min(scan_tiles_of<T>(clen[c]), tile_cap + 1);
  const std::vector<uint64_t> tbase = excl_scan(want);
  auto tiled = [&](uint64_t c) { return tile_cap != 0 && want[c] != 0 && tbase[c + 1] <= tile_cap; };
  uint64_t nt = 0;
  for (uint64_t c = 0; c < nconn; ++c)
    if (tiled(c)) nt = std::max(nt, tbase[c + 1]);
  int L = 1;
  while (scan_level_count<G>(tile_cap, (uint32_t)L) > 1) ++L;
  // tile pass
  std::vector<std::vector<uint16_t>> maps(L), entry(L);
  for (int l = 0; l < L; ++l) {
    maps[l].assign(scan_level_count<G>(tile_cap, (uint32_t)l) * kScanMapLen, 0xDEAD);
    entry[l].assign(scan_level_count<G>(tile_cap, (uint32_t)l), 0xDEAD);
  }
  std::vector<uint32_t> tconn(tile_cap, 0);
  for (uint64_t j = 0; j < nt; ++j) {
    const uint64_t c = scan_find_conn(tbase.data(), nconn, j);
    tconn[j] = (uint32_t)c;
    if (!(tbase[c] <= j && j < tbase[c + 1])) die("scan_find_conn");
    const uint64_t k = j - tbase[c], t0 = k * T;
    const TileRd rd{stream.data() + coff[c], clen[c], t0, (uint64_t)T + kScanHalo};
    uint16_t *m = &maps[0][j * kScanMapLen];
    if (k == 0) {
      const uint16_t x = scan_tile_exit<T>(rd, t0, 0, clen[c], flags);
      for (uint32_t e = 0; e < kScanMapLen; ++e) m[e] = x;
    } else {
      for (uint32_t e = 0; e < kScanEntries; ++e) m[e] = scan_tile_exit<T>(rd, t0, e, clen[c], flags);
      m[kScanStop] = (uint16_t)kScanStop;
    }
  }
  // up-sweep
  for (int l = 1; l < L; ++l) {
    const uint64_t n_below = scan_level_count<G>(nt, (uint32_t)l - 1);
    for (uint64_t g = 0; g * G < n_below; ++g) {
      const uint32_t count = (uint32_t)std::min<uint64_t>(G, n_below - g * G);
      for (uint32_t e = 0; e < kScanMapLen; ++e)
        maps[l][g * kScanMapLen + e] = scan_compose(&maps[l - 1][g * G * kScanMapLen], count, e);
    }
  }
  // down-sweep
  for (int l = L - 1; l >= 0; --l) {
    const uint64_t n_here = scan_level_count<G>(nt, (uint32_t)l);
    for (uint64_t g = 0; g * G < n_here; ++g) {
      const uint32_t count = (uint32_t)std::min<uint64_t>(G, n_here - g * G);
      const uint32_t e = (l + 1 == L) ? kScanStop : entry[l + 1][g];
      if (e > kScanStop) die("unresolved entry");
      scan_resolve(&maps[l][g * G * kScanMapLen], count, e, &entry[l][g * G]);
    }
  }
  // count
  std::vector<uint64_t> conn_cnt(nconn, 0), consumed(nconn, ~0ull), tile_cnt(tile_cap, 0);
  std::vector<int> state(nconn, -1), stops(nconn, 0);
  for (uint64_t c = 0; c < nconn; ++c) {
    if (!inside(c)) {
      consumed[c] = 0;
      state[c] = 1;
      continue;
    }
    if (tiled(c)) continue;
    const ScanWalk w = scan_walk(ConnRd{stream.data() + coff[c], clen[c]}, 0, ~0ull, clen[c], flags, ScanNoSink{});
    conn_cnt[c] = w.count;
    consumed[c] = w.p;
    state[c] = (int)w.closed;
  }
  for (uint64_t j = 0; j < nt; ++j) {
    const uint64_t c = tconn[j], k = j - tbase[c];
    const uint32_t e = k == 0 ? 0u : entry[0][j];
    if (e == kScanStop) continue;
    const uint64_t t0 = k * T;
    const ScanWalk w =
        scan_walk(ConnRd{stream.data() + coff[c], clen[c]}, t0 + e, t0 + T, clen[c], flags, ScanNoSink{});
    tile_cnt[j] = w.count;
    if (w.stopped) {
      consumed[c] = w.p;
      state[c] = (int)w.closed;
      stops[c] += 1;
    }
  }
  const std::vector<uint64_t> tpre = excl_scan(tile_cnt);
  for (uint64_t c = 0; c < nconn; ++c)
    if (tiled(c)) {
      if (stops[c] != 1) die("a tiled connection's stop was met by other than one tile");
      conn_cnt[c] = tpre[tbase[c + 1]] - tpre[tbase[c]];
    }
  const std::vector<uint64_t> first = excl_scan(conn_cnt);
  // emit
  std::vector<uint64_t> offs(first[nconn], ~0ull);
  for (uint64_t c = 0; c < nconn; ++c) {
    if (!inside(c) || tiled(c)) continue;
    (void)scan_walk(ConnRd{stream.data() + coff[c], clen[c]}, 0, ~0ull, clen[c], flags,
                    VecSink{&offs, first[c], coff[c]});
  }
  for (uint64_t j = 0; j < nt; ++j) {
    const uint64_t c = tconn[j], k = j - tbase[c];
    const uint32_t e = k == 0 ? 0u : entry[0][j];
    if (e == kScanStop) continue;
    const uint64_t t0 = k * T, base = first[c] + (tpre[j] - tpre[tbase[c]]);
    (void)scan_walk(ConnRd{stream.data() + coff[c], clen[c]}, t0 + e, t0 + T, clen[c], flags,
                    VecSink{&offs, base, coff[c]});
  }
  printf("levels %d tiles %llu\n", L, (unsigned long long)nt);
  for (uint64_t c = 0; c < nconn; ++c) {
    printf("%d %llu %llu", state[c], (unsigned long long)consumed[c], (unsigned long long)conn_cnt[c]);
    for (uint64_t i = first[c]; i < first[c + 1]; ++i) printf(" %llu", (unsigned long long)offs[i]);
    printf("\n");
  }
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc != 8) die("usage: scan_emu T G flags tiled_min tile_cap stream conns");
  const uint32_t T = (uint32_t)strtoul(argv[1], nullptr, 10), G = (uint32_t)strtoul(argv[2], nullptr, 10);
  const int flags = atoi(argv[3]);
  const uint64_t tiled_min = strtoull(argv[4], nullptr, 10), tile_cap = strtoull(argv[5], nullptr, 10);
  std::ifstream sf(argv[6], std::ios::binary);
  const std::vector<uint8_t> stream((std::istreambuf_iterator<char>(sf)), std::istreambuf_iterator<char>());
  std::vector<uint64_t> coff, clen;
  std::ifstream cf(argv[7]);
  for (uint64_t o, l; cf >> o >> l;) {
    coff.push_back(o);
    clen.push_back(l);
  }
  if (T == kScanTile && G == kScanGroup) return run<kScanTile, kScanGroup>(flags, tiled_min, tile_cap, stream, coff, clen);
  if (T == 2048 && G == 4) return run<2048, 4>(flags, tiled_min, tile_cap, stream, coff, clen);
  if (T == kScanEntries && G == 2) return run<kScanEntries, 2>(flags, tiled_min, tile_cap, stream, coff, clen);
  die("no such instantiation");
}
