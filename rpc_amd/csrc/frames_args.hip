// rpc_amd/csrc/frames_args.hip -- device-side frame args
// (rpc_frames_args_device; the rules, the walk and the conversions:
// frames_args.h).
#include "../../include/rpccrc.h"
#include "frames_args.h"
#include "frames_stage.h"

namespace rpccrc {

static_assert(kArgsNone == RPC_ARGS_NONE && kArgsOk == RPC_ARGS_OK && kArgsInvalid == RPC_ARGS_INVALID &&
                  kArgsDefer == RPC_ARGS_DEFER && kArgsRange == RPC_ARGS_RANGE && kArgsBadSchema == RPC_ARGS_BAD_SCHEMA,
              "frames_args.h restates the statuses");
static_assert(kArgI32 == RPC_ARG_I32 && kArgI64 == RPC_ARG_I64 && kArgF64 == RPC_ARG_F64 && kArgBool == RPC_ARG_BOOL &&
                  kArgStr == RPC_ARG_STR,
              "the types");
static_assert(kArgsMaxParams == RPC_ARGS_MAX_PARAMS && kArgsMaxSchemaParams == RPC_ARGS_MAX_SCHEMA_PARAMS &&
                  kArgsMaxNameBytes == RPC_ARGS_MAX_NAME_BYTES,
              "and the limits");

namespace {

constexpr int kArgsThreads = (int)kRouteEntries;

// The powers of five stay in global memory: a lookup is per lane and far rarer
// than a step of the walk, and 10 KiB more of LDS would cost a workgroup per CU.
__device__ const uint64_t g_pow10[2 * (kPow10Max - kPow10Min + 1)] = {RPCCRC_POW10_WORDS};
struct DevPow {
  __device__ __forceinline__ uint64_t word(uint32_t i) const { return g_pow10[i]; }
};

// The schema is read where it lies: a method's few words and names are shared
// by every entry of that method and stay in the caches.
struct DevSchema {
  const uint32_t *firsts;
  const uint8_t *types;
  const uint32_t *name_offs;
  const uint8_t *names;
  __device__ __forceinline__ uint32_t first(uint32_t m) const { return firsts[m]; }
  __device__ __forceinline__ uint32_t type(uint32_t p) const { return types[p]; }
  __device__ __forceinline__ uint32_t name_off(uint32_t p) const { return name_offs[p]; }
  __device__ __forceinline__ uint32_t name(uint32_t b) const { return names[b]; }
};

// Slot k of entry e is at k * n + e: a lane's store joins its neighbours'.
struct DevSink {
  uint64_t *slots;
  uint64_t n, e;
  __device__ __forceinline__ void put(uint32_t k, uint64_t v) const {
    if (slots) slots[(uint64_t)k * n + e] = v;
  }
};

// The entry's outputs but the slots args_one() handed over: for OK the slots
// behind the method's `used` parameters read 0, for every other status all do.
__device__ __forceinline__ void finish(const ArgsArgs &a, uint64_t e, uint8_t status, uint32_t used) {
  if (a.status) a.status[e] = status;
  if (a.reply_status) a.reply_status[e] = args_reply_status(status);
  if (a.slots)
    for (uint32_t k = status == kArgsOk ? used : 0u; k < a.width; ++k) a.slots[(uint64_t)k * a.n + e] = 0;
}

// One workgroup per kRouteEntries consecutive entries, one lane per entry; the
// `params` spans are staged in LDS in rounds (stage_rounds, frames_stage.h) and
// each lane walks its own there.
__global__ __launch_bounds__(kArgsThreads) void args_kernel(ArgsArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kRouteEntries + threadIdx.x;
  const DevSchema sc{a.param_first, a.param_types, a.param_name_off, a.param_names};
  uint64_t off = 0;
  uint32_t len = 0, base = 0, f0 = 0, f1 = 0;
  bool pending = false;
  if (e < a.n) {
    const uint8_t kind = a.kind[e];
    uint64_t body_off = 0;
    uint32_t body_len = 0, method = 0;
    if (kind == kRouteCall) { // (only then is anything else of the entry looked at)
      method = a.method[e];
      body_off = a.body_off[e], body_len = a.body_len[e];
      base = a.params_off[e], len = a.params_len[e];
    }
    const uint8_t st = args_precheck(kind, method, sc, a.nmethods, a.nparams, a.name_bytes, a.width, body_off, body_len,
                                     base, len, a.bodies_bytes, &f0, &f1);
    pending = st == kArgsWalk;
    if (pending) off = body_off + base;
    else finish(a, e, st, 0); // (OK here is a method without parameters)
  }
  stage_rounds(a.bodies, a.bodies_bytes, off, len, pending, [&](LdsBody &body) {
    const DevSink sink{a.slots, a.n, e};
    const uint8_t st = args_one(body, len, base, sc, f0, f1, DevPow{}, sink);
    finish(a, e, st, f1 - f0);
  });
}

} // namespace

hipError_t launch_frames_args(const ArgsArgs &a, hipStream_t s) {
  const uint64_t nwg = (a.n + kRouteEntries - 1) / kRouteEntries;
  hipLaunchKernelGGL(args_kernel, dim3((unsigned)nwg), dim3(kArgsThreads), 0, s, a);
  return hipGetLastError();
}

} // namespace rpccrc
