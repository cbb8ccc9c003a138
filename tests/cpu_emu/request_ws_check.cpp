// tests/cpu_emu/request_ws_check.cpp -- the frame request's workspace layout
// (request_ws_layout of rpc_amd/csrc/frames_request.h) over the carver of
// rpc_amd/csrc/workspace.h, on the host: at each n the measuring pass and the
// carving pass agree, the six arrays are 256-aligned, in order, disjoint, inside
// the block and as long as the kernels index them, and a block one byte short is
// refused.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rpc_amd/csrc/frames_request.h"
#include "../../rpc_amd/csrc/workspace.h"

using namespace rpccrc;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

int main() {
  const uint64_t counts[] = {1, 2, 31, 32, 33, 257, 4095, 4096, 100000};
  long layouts = 0;
  for (uint64_t n : counts) {
    for (size_t tmp : {(size_t)0, (size_t)1, (size_t)513}) {
      WsLayout m;
      const RequestWs mw = request_ws_layout(m, n, tmp);
      CHECK(m.ok() && mw.sizes == nullptr && mw.name_word == nullptr);
      const size_t total = m.used();
      std::vector<uint8_t> block(total + 256);
      uint8_t *base = block.data();
      WsLayout w(base, total);
      const RequestWs r = request_ws_layout(w, n, tmp);
      CHECK(w.ok() && w.used() == total);
      // the arrays in the order they are taken, with the bytes the kernels index
      const struct {
        const void *p;
        size_t bytes;
      } a[6] = {{r.sizes, n * 8},        {r.src_off, n * 8}, {r.offs, (n + 1) * 8},
                {r.scan_tmp, tmp * 8},   {r.meta, n * 4},    {r.name_word, (size_t)kRequestMaxMethods * 4}};
      size_t off = 0;
      for (int k = 0; k < 6; ++k) {
        const size_t at = (size_t)(static_cast<const uint8_t *>(a[k].p) - base);
        CHECK(at == off && at % 256 == 0);
        CHECK(at + a[k].bytes <= total);
        off += align256(a[k].bytes);
        CHECK(at + a[k].bytes <= off);
        if (a[k].bytes) base[at] = base[at + a[k].bytes - 1] = (uint8_t)k; // (the sanitizer's view of it)
      }
      CHECK(off == total);
      WsLayout s(base, total - 1);
      request_ws_layout(s, n, tmp);
      CHECK(!s.ok());
      ++layouts;
    }
  }
  printf("ok %ld layouts\n", layouts);
  return 0;
}
