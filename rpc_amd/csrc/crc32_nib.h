// rpc_amd/csrc/crc32_nib.h -- A_n(v) from the nibble shift maps (device code).
//
// A_n(v) for n = sum of 2^k bytes, applied map by map from the nibble tables
// NIB[k][i][j] = A_{2^k}(j << 4i) (64 maps x 8 nibble positions x 16, in LDS;
// kShiftNibWords, built by init_device): 8 lookups per set bit of n, instead of
// a bit-serial gf2_mulmod for x^(8n) and another for the product (~30 of those
// per thread for C4's shifts).  Used by the chunk combine (crc32_kernels.hip)
// and the gather fold (crc32_gather.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rpccrc {

__device__ __forceinline__ uint32_t nib_apply(const uint32_t *nib, uint32_t k, uint32_t v) {
  const uint32_t *m = nib + k * 128u;
  uint32_t r = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) r ^= m[i * 16u + ((v >> (4u * i)) & 15u)];
  return r;
}
__device__ __forceinline__ uint32_t nib_shift(const uint32_t *nib, uint64_t nbytes, uint32_t v) {
  while (nbytes) {
    const uint32_t k = (uint32_t)__builtin_ctzll(nbytes);
    v = nib_apply(nib, k, v);
    nbytes &= nbytes - 1;
  }
  return v;
}

} // namespace rpccrc
