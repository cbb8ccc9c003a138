// rpc_amd/csrc/frames_results.hip -- device-side frame results
// (rpc_frames_results_device; the rules, the walk and the conversions:
// frames_results.h).
//
//   [open-slot pass ->] results kernel
#include "../../include/rpccrc.h"
#include "frames_results.h"
#include "frames_stage.h"

namespace rpccrc {

static_assert(kResultsNone == RPC_RESULTS_NONE && kResultsOk == RPC_RESULTS_OK && kResultsAbsent == RPC_RESULTS_ABSENT &&
                  kResultsMismatch == RPC_RESULTS_MISMATCH && kResultsDefer == RPC_RESULTS_DEFER &&
                  kResultsRange == RPC_RESULTS_RANGE && kResultsBadSchema == RPC_RESULTS_BAD_SCHEMA,
              "frames_results.h restates the statuses");

namespace {

constexpr int kResultsThreads = (int)kRouteEntries;

// The powers of five stay in global memory, as the args keep theirs.
__device__ const uint64_t g_results_pow10[2 * (kPow10Max - kPow10Min + 1)] = {RPCCRC_POW10_WORDS};
struct DevPow {
  __device__ __forceinline__ uint64_t word(uint32_t i) const { return g_results_pow10[i]; }
};
struct DevPending {
  const uint16_t *methods;
  __device__ __forceinline__ uint32_t method(uint32_t s) const { return methods[s]; }
};
struct DevTypes {
  const uint8_t *types;
  __device__ __forceinline__ uint32_t type(uint32_t m) const { return types[m]; }
};
struct DevCols {
  const uint8_t *kinds;
  const uint32_t *slots;
  __device__ __forceinline__ uint32_t kind(uint32_t e) const { return kinds[e]; }
  __device__ __forceinline__ uint32_t slot(uint32_t e) const { return slots[e]; }
};

// A span of the staged body: the same words, the base moved by the span's offset.
struct DevView {
  const LdsBody *body;
  __device__ __forceinline__ LdsBody operator()(uint32_t off) const { return LdsBody(body->lds, body->base + off); }
};

// The entry's outputs, each column's store beside its neighbours'; and, for the
// entry that completes a slot (`own`), that slot's.
__device__ __forceinline__ void put(const ResultsArgs &a, uint64_t e, const ResultsOut &o, bool own, uint32_t slot,
                                    uint64_t body_off) {
  if (a.status) a.status[e] = o.status;
  if (a.value) a.value[e] = o.value;
  if (a.error_status) a.error_status[e] = o.error_status;
  if (a.error_code) a.error_code[e] = o.error_code;
  if (a.error_message) a.error_message[e] = o.error_message;
  if (!own) return;
  if (a.slot_status) a.slot_status[slot] = o.status;
  if (a.slot_value) a.slot_value[slot] = o.value;
  if (a.slot_error_status) a.slot_error_status[slot] = o.error_status;
  if (a.slot_error_code) a.slot_error_code[slot] = o.error_code;
  if (a.slot_str_base) a.slot_str_base[slot] = body_off;
}

// One workgroup per kRouteEntries consecutive entries, one lane per entry; the
// bodies of the MATCHED entries that have a member to read are staged in LDS in
// rounds (stage_rounds, frames_stage.h), once, and each lane walks its two
// spans there.
__global__ __launch_bounds__(kResultsThreads) void results_kernel(ResultsArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kRouteEntries + threadIdx.x;
  uint64_t body_off = 0;
  uint32_t body_len = 0, slot = 0, type = 0, r_off = 0, r_len = 0, e_off = 0, e_len = 0;
  bool pending = false, own = false, defer = false;
  if (e < a.n) {
    const uint8_t kind = a.kind[e];
    if (kind == kResolveMatched) { // (only then is anything else of the entry looked at)
      slot = a.slot[e];
      body_off = a.body_off[e], body_len = a.body_len[e];
      r_off = a.result_off[e], r_len = a.result_len[e];
      e_off = a.error_off[e], e_len = a.error_len[e];
      own = a.slot_entry && slot < a.npending && a.slot_entry[slot] == (uint32_t)e;
    }
    const uint8_t st = results_precheck(kind, slot, DevPending{a.pending_method}, a.npending, DevTypes{a.result_types},
                                        a.nmethods, body_off, body_len, r_off, r_len, e_off, e_len, a.bodies_bytes, &type);
    ResultsOut o = results_plain(st);
    if (st == kResultsWalk) pending = results_unread(body_len, r_len, e_len, &o);
    if (!pending) {
      defer = o.status == kResultsDefer || o.error_status == kResultsDefer;
      put(a, e, o, own, slot, body_off);
    }
  }
  stage_rounds(a.bodies, a.bodies_bytes, body_off, body_len, pending, [&](LdsBody &body) {
    const ResultsOut o = results_walk(DevView{&body}, type, r_off, r_len, e_off, e_len, DevPow{});
    defer = o.status == kResultsDefer || o.error_status == kResultsDefer;
    put(a, e, o, own, slot, body_off);
  });
  if (a.ndefer) { // one atomic per wavefront that has any
    const uint64_t d = __ballot(defer);
    if (d && (threadIdx.x & 63u) == 0) atomicAdd(a.ndefer, (uint32_t)__popcll(d));
  }
}

// One lane per slot: a slot that no entry completes reads 0 in every column.
// (The slot an entry completes is that entry's lane's, above: the two passes
// write disjoint slots and read no output, so their order does not matter.)
__global__ __launch_bounds__(kResultsThreads) void results_open_kernel(ResultsArgs a) {
  const uint32_t s = blockIdx.x * kResultsThreads + threadIdx.x;
  if (s >= a.npending) return;
  if (results_completes(a.slot_entry[s], a.n, DevCols{a.kind, a.slot}, s)) return;
  if (a.slot_status) a.slot_status[s] = 0;
  if (a.slot_value) a.slot_value[s] = 0;
  if (a.slot_error_status) a.slot_error_status[s] = 0;
  if (a.slot_error_code) a.slot_error_code[s] = 0;
  if (a.slot_str_base) a.slot_str_base[s] = 0;
}

unsigned blocks_for(uint64_t items) { return (unsigned)((items + kResultsThreads - 1) / kResultsThreads); }

} // namespace

hipError_t launch_frames_results(const ResultsArgs &a, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (a.ndefer && (e = hipMemsetAsync(a.ndefer, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
  const bool per_slot = a.slot_status || a.slot_value || a.slot_error_status || a.slot_error_code || a.slot_str_base;
  if (per_slot && a.npending) {
    hipLaunchKernelGGL(results_open_kernel, dim3(blocks_for(a.npending)), dim3(kResultsThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.n) {
    hipLaunchKernelGGL(results_kernel, dim3(blocks_for(a.n)), dim3(kResultsThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace rpccrc
