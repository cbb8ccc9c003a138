/* tools/scan_walk_host.c -- the frame walk of rpc_frames_scan_device on one host
 * thread (tools/scan_bench.py leg (b): the baseline a receive loop has today).
 * Same rules as rpc_amd/csrc/frames_scan.h scan_step; flags as RPC_FRAMES_*. */
#include <stdint.h>

uint64_t scan_walk_host(const uint8_t *b, uint64_t len, int flags, uint64_t *out, uint64_t cap, uint64_t *consumed,
                        uint8_t *state) {
  const uint32_t control = (flags & 1) ? 1u : 2u;
  uint64_t p = 0, n = 0;
  *state = 0;
  while (len - p >= 12) {
    const uint32_t type = ((uint32_t)b[p + 2] << 8) | b[p + 3];
    const uint32_t bl = ((uint32_t)b[p + 4] << 24) | ((uint32_t)b[p + 5] << 16) | ((uint32_t)b[p + 6] << 8) | b[p + 7];
    uint64_t adv = 12;
    int close = 0;
    if (type != control) {
      if ((bl > 1024 && !(flags & 4)) || (bl == 0 && (flags & 2)))
        close = 1;
      else if (len - (p + 12) < bl)
        break;
      else
        adv += bl;
    }
    if (n < cap) out[n] = p;
    n += 1;
    p += adv;
    if (close) {
      *state = 1;
      break;
    }
  }
  *consumed = p;
  return n;
}
