// rpc_amd/csrc/excl_scan.h -- the device-wide exclusive scan over uint64 words
// (defined in frames_scan.hip; used by the frame scan and the frame pack).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rpccrc {

// Words of `tmp` an exclusive scan over n words needs.
uint64_t scan_tmp_words(uint64_t n);
// out[i] = in[0] + ... + in[i - 1] for i <= n (out holds n + 1 words: out[n] is
// the total).  Enqueued on s; in and out are different arrays.
hipError_t excl_scan(const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *tmp, hipStream_t s);

} // namespace rpccrc
