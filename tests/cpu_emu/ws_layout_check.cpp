// tests/cpu_emu/ws_layout_check.cpp -- the workspace carver (rpc_amd/csrc/workspace.h)
// on the host: a layout of five arrays, one per element size, at every combination of
// the counts below.  Measuring and carving agree; the arrays are 256-aligned, in order,
// disjoint and inside the block; one byte less is refused for good; a count that
// overflows size_t is refused without wrapping; rest() is what is left.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rpc_amd/csrc/workspace.h"

using rpccrc::WsLayout;
using rpccrc::align256;

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

struct E16 {
  uint64_t a, b;
};
static_assert(sizeof(E16) == 16, "a 16-byte element");

struct Arrays {
  uint8_t *p[5];
};
static const size_t kSize[5] = {1, 2, 4, 8, 16};

static void layout(WsLayout &w, const size_t cnt[5], Arrays *a) {
  a->p[0] = w.take<uint8_t>(cnt[0]);
  a->p[1] = reinterpret_cast<uint8_t *>(w.take<uint16_t>(cnt[1]));
  a->p[2] = reinterpret_cast<uint8_t *>(w.take<uint32_t>(cnt[2]));
  a->p[3] = reinterpret_cast<uint8_t *>(w.take<uint64_t>(cnt[3]));
  a->p[4] = reinterpret_cast<uint8_t *>(w.take<E16>(cnt[4]));
}

template <class T> static void overflow_check(uint8_t *base) {
  for (size_t back = 0; back < 3; ++back) {
    const size_t huge = SIZE_MAX / sizeof(T) - back;
    WsLayout m; // measuring: no cap, only size_t itself is in the way
    CHECK(m.take<T>(1) == nullptr && m.ok() && m.used() == 256);
    CHECK(m.take<T>(huge) == nullptr && !m.ok());
    CHECK(m.used() == 256); // (did not wrap, did not move)
    CHECK(m.take<T>(1) == nullptr && !m.ok() && m.used() == 256);
    WsLayout w(base, 1024);
    CHECK(w.take<T>(huge) == nullptr && !w.ok() && w.used() == 0);
    CHECK(w.take<T>(1) == nullptr && !w.ok());
  }
}

int main() {
  const size_t counts[] = {0, 1, 63, 64, 65, 4095, (size_t)1 << 20};
  const size_t nc = sizeof counts / sizeof counts[0];
  const size_t max_bytes = 5 * 256 + ((size_t)1 << 20) * (1 + 2 + 4 + 8 + 16);
  std::vector<uint8_t> block(max_bytes + 256);
  uint8_t *base = block.data(); // (alignment is relative to base)
  size_t idx[5] = {0, 0, 0, 0, 0};
  long layouts = 0;
  for (;;) {
    size_t cnt[5];
    for (int k = 0; k < 5; ++k) cnt[k] = counts[idx[k]];
    Arrays ma, ca;
    WsLayout m;
    layout(m, cnt, &ma);
    CHECK(m.ok());
    const size_t total = m.used();
    size_t want = 0;
    for (int k = 0; k < 5; ++k) {
      CHECK(ma.p[k] == nullptr); // measuring only counts
      want += align256(cnt[k] * kSize[k]);
    }
    CHECK(total == want && total <= max_bytes);
    size_t left = 1;
    CHECK(m.rest(&left) == nullptr && left == 0);

    WsLayout w(base, total); // a block of exactly used() bytes
    layout(w, cnt, &ca);
    CHECK(w.ok() && w.used() == total);
    size_t off = 0;
    for (int k = 0; k < 5; ++k) {
      const size_t at = (size_t)(ca.p[k] - base);
      CHECK(at == off);      // the measuring pass's offsets (its running sum)
      CHECK(at % 256 == 0);
      const size_t end = at + cnt[k] * kSize[k];
      CHECK(end <= total);   // inside the block, the last one too
      off += align256(cnt[k] * kSize[k]);
      CHECK(end <= off);     // ... and below the next array
      if (cnt[k]) ca.p[k][0] = ca.p[k][cnt[k] * kSize[k] - 1] = (uint8_t)k; // (the sanitizer's view of it)
    }
    CHECK(w.rest(&left) == base + total && left == 0);
    CHECK(w.take<uint32_t>(0) == reinterpret_cast<uint32_t *>(base + total) && w.ok() && w.used() == total);

    WsLayout slack(base, total + 77); // rest(): the remainder, not rounded
    layout(slack, cnt, &ca);
    CHECK(slack.ok() && slack.rest(&left) == base + total && left == 77);

    if (total > 0) { // one byte less: refused, and stays refused
      WsLayout s(base, total - 1);
      layout(s, cnt, &ca);
      CHECK(!s.ok() && s.used() <= total - 1);
      const size_t used = s.used();
      CHECK(s.take<uint8_t>(0) == nullptr && s.take<uint8_t>(1) == nullptr && !s.ok() && s.used() == used);
      CHECK(s.rest(&left) == nullptr && left == 0);
    }
    ++layouts;
    int k = 0;
    while (k < 5 && ++idx[k] == nc) idx[k++] = 0;
    if (k == 5) break;
  }
  overflow_check<uint8_t>(base);
  overflow_check<uint16_t>(base);
  overflow_check<uint32_t>(base);
  overflow_check<uint64_t>(base);
  overflow_check<E16>(base);
  { // the running sum, not one count, overflows
    WsLayout m;
    const size_t half = SIZE_MAX / 2 - 255; // 2^63 - 256
    CHECK(m.take<uint8_t>(half) == nullptr && m.ok());
    CHECK(m.take<uint8_t>(half) == nullptr && m.ok());
    CHECK(m.take<uint8_t>(256) == nullptr && m.ok() && m.used() == SIZE_MAX - 255);
    CHECK(m.take<uint8_t>(1) == nullptr && !m.ok() && m.used() == SIZE_MAX - 255);
  }
  printf("ok %ld layouts\n", layouts);
  return 0;
}
