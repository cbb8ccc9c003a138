// rpc_amd/csrc/frames_resolve.hip -- device-side frame resolve
// (rpc_frames_resolve_device; the rules, the key policy and the join's table:
// frames_resolve.h).
//
//   [table pass ->] resolve kernel -> finish pass [-> exclusive scan -> compaction]
#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_resolve.h"
#include "frames_stage.h"

namespace rpccrc {

static_assert(kResolveNone == RPC_RESOLVE_NONE && kResolveMatched == RPC_RESOLVE_MATCHED &&
                  kResolveUnknown == RPC_RESOLVE_UNKNOWN && kResolveDuplicate == RPC_RESOLVE_DUPLICATE &&
                  kResolveInvalid == RPC_RESOLVE_INVALID && kResolveDefer == RPC_RESOLVE_DEFER &&
                  kResolveRange == RPC_RESOLVE_RANGE && kResolveNoSlot == RPC_RESOLVE_NO_SLOT &&
                  kResolveMaxPending == RPC_RESOLVE_MAX_PENDING,
              "frames_resolve.h restates the kinds and the limit");

namespace {

constexpr int kResolveThreads = (int)kRouteEntries;

// ---- the table pass: every slot into the (emptied) table --------------------
struct GlobalCas {
  uint32_t *cells;
  __device__ __forceinline__ uint32_t operator()(uint32_t c, uint32_t expect, uint32_t value) {
    return atomicCAS(&cells[c], expect, value);
  }
};
__global__ __launch_bounds__(kResolveThreads) void resolve_table_kernel(ResolveArgs a) {
  const uint32_t s = blockIdx.x * kResolveThreads + threadIdx.x;
  if (s >= a.npending) return;
  GlobalCas cas{a.cells};
  resolve_insert(cas, s, a.pending[s], a.bits);
}

struct GlobalCells {
  const uint32_t *cells;
  __device__ __forceinline__ uint32_t cell(uint32_t c) const { return cells[c]; }
};
struct GlobalIds {
  const uint32_t *ids;
  __device__ __forceinline__ uint32_t id(uint32_t s) const { return ids[s]; }
};

__device__ __forceinline__ void put(const ResolveArgs &a, uint64_t e, ResolveOut o) {
  uint32_t slot = kResolveNoSlot;
  if (o.kind == kResolveUnknown && a.npending) {
    slot = resolve_probe(GlobalCells{a.cells}, GlobalIds{a.pending}, o.id, a.bits);
    if (slot != kResolveNoSlot) {
      atomicMin(&a.slot_entry[slot], (uint32_t)e);
      o.kind = kResolveMatched; // (until the finish pass has seen who took the slot)
    }
  }
  if (a.kind) a.kind[e] = o.kind;
  if (a.id) a.id[e] = o.id;
  if (a.result_off) a.result_off[e] = o.result_off;
  if (a.result_len) a.result_len[e] = o.result_len;
  if (a.error_off) a.error_off[e] = o.error_off;
  if (a.error_len) a.error_len[e] = o.error_len;
  if (a.slot) a.slot[e] = slot;
}

// One workgroup per kRouteEntries consecutive entries, one lane per entry, the
// bodies staged in LDS in rounds: the route kernel's shape (frames_stage.h).
// After its walk a lane probes the table and claims its slot.
__global__ __launch_bounds__(kResolveThreads) void resolve_kernel(ResolveArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kRouteEntries + threadIdx.x;
  uint64_t off = 0;
  uint32_t len = 0;
  bool pending = false;
  if (e < a.n) {
    ResolveOut o;
    const bool has_type = a.types != nullptr;
    const uint32_t type = has_type ? a.types[e] : 0u;
    if (!has_type || type == kRouteTypeData) { // (only then are the offset and the length looked at)
      off = a.body_off[e];
      len = a.body_len[e];
    }
    pending = resolve_precheck(has_type, type, off, len, a.bodies_bytes, &o);
    if (!pending) put(a, e, o);
  }
  stage_rounds(a.bodies, a.bodies_bytes, off, len, pending, [&](LdsBody &body) { put(a, e, resolve_one(body, len)); });
}

// ---- the finish pass ---------------------------------------------------------
// An entry that named a slot reads off slot_entry whether it took it; a slot
// that nobody took is flagged open.
__global__ __launch_bounds__(kResolveThreads) void resolve_finish_kernel(ResolveArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kResolveThreads + threadIdx.x;
  if (i < a.n && a.kind && a.npending) {
    const uint32_t slot = a.slot[i];
    if (slot != kResolveNoSlot) a.kind[i] = resolve_final(a.slot_entry[slot], (uint32_t)i);
  }
  if (i < a.npending && a.flags) a.flags[i] = a.slot_entry[i] == kResolveNoSlot ? 1u : 0u;
}

__global__ __launch_bounds__(kResolveThreads) void resolve_open_kernel(ResolveArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kResolveThreads + threadIdx.x;
  if (s < a.npending && a.flags[s]) a.open[a.offs[s]] = (uint32_t)s;
  if (s == 0) *a.nopen = (uint32_t)a.offs[a.npending];
}

unsigned blocks_for(uint64_t items) { return (unsigned)((items + kResolveThreads - 1) / kResolveThreads); }

} // namespace

hipError_t launch_frames_resolve(const ResolveArgs &a, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (a.npending) {
    if ((e = hipMemsetAsync(a.cells, 0xFF, sizeof(uint32_t) << a.bits, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.slot_entry, 0xFF, sizeof(uint32_t) * (size_t)a.npending, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(resolve_table_kernel, dim3(blocks_for(a.npending)), dim3(kResolveThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.n) {
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks_for(a.n)), dim3(kResolveThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!a.npending) // nothing to finish: no slot is open
    return a.nopen ? hipMemsetAsync(a.nopen, 0, sizeof(uint32_t), s) : hipSuccess;
  if ((a.n && a.kind) || a.flags) {
    const uint64_t items = a.n > a.npending ? a.n : a.npending;
    hipLaunchKernelGGL(resolve_finish_kernel, dim3(blocks_for(items)), dim3(kResolveThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!a.open) return hipSuccess;
  if ((e = excl_scan(a.flags, a.offs, a.npending, a.scan_tmp, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(resolve_open_kernel, dim3(blocks_for(a.npending)), dim3(kResolveThreads), 0, s, a);
  return hipGetLastError();
}

} // namespace rpccrc
