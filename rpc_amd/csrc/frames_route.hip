// rpc_amd/csrc/frames_route.hip -- device-side frame route
// (rpc_frames_route_device; the rules, the automaton and the method compare:
// frames_route.h).
//
//   route kernel [-> bucket counts -> exclusive scan -> scatter]
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_route.h"
#include "frames_stage.h"

namespace rpccrc {

static_assert(kRouteNone == RPC_ROUTE_NONE && kRouteCall == RPC_ROUTE_CALL && kRouteNotFound == RPC_ROUTE_NOT_FOUND &&
                  kRouteInvalid == RPC_ROUTE_INVALID && kRouteDefer == RPC_ROUTE_DEFER && kRouteRange == RPC_ROUTE_RANGE &&
                  kRouteNoMethod == RPC_ROUTE_NO_METHOD,
              "frames_route.h restates the kinds");
static_assert(kRouteMaxBody == RPC_ROUTE_MAX_BODY && kRouteMaxDepth == RPC_ROUTE_MAX_DEPTH &&
                  kRouteMaxTokens == RPC_ROUTE_MAX_TOKENS && kRouteMaxMethods == RPC_ROUTE_MAX_METHODS &&
                  kRouteMaxMethodBytes == RPC_ROUTE_MAX_METHOD_BYTES && kRouteTypeData == RPC_FRAME_TYPE_DATA,
              "and the limits");

namespace {

constexpr int kRouteThreads = (int)kRouteEntries;
constexpr uint32_t kRouteWaves = kRouteEntries / 64;

struct LdsTab {
  const uint32_t *offs;
  const uint8_t *names;
  __device__ __forceinline__ uint32_t off(uint32_t m) const { return offs[m]; }
  __device__ __forceinline__ uint32_t name(uint32_t p) const { return names[p]; }
};

__device__ __forceinline__ void put(const RouteArgs &a, uint64_t e, const RouteOut &o) {
  if (a.kind) a.kind[e] = o.kind;
  if (a.method) a.method[e] = o.method;
  if (a.id) a.id[e] = o.id;
  if (a.params_off) a.params_off[e] = o.params_off;
  if (a.params_len) a.params_len[e] = o.params_len;
  if (a.bucket) a.bucket[e] = (uint16_t)route_bucket(o.kind, o.method, a.nmethods);
}

// One workgroup per kRouteEntries consecutive entries, one lane per entry; the
// bodies are staged in LDS in rounds (stage_rounds, frames_stage.h) and each
// lane walks its own there.
__global__ __launch_bounds__(kRouteThreads) void route_kernel(RouteArgs a) {
  __shared__ uint32_t s_moff[kRouteMaxMethods + 1];
  __shared__ uint4 s_names[kRouteMaxMethodBytes / 16];
  const uint32_t t = threadIdx.x;
  const uint64_t e = (uint64_t)blockIdx.x * kRouteEntries + t;

  if (a.nmethods) // (an empty table may come without its one offset word)
    for (uint32_t i = t; i <= a.nmethods; i += kRouteThreads) s_moff[i] = a.method_off[i];
  {
    uint8_t *nb = reinterpret_cast<uint8_t *>(s_names);
    for (uint32_t i = t; i < a.method_bytes; i += kRouteThreads) nb[i] = a.names[i];
  }
  uint64_t off = 0;
  uint32_t len = 0;
  bool pending = false;
  if (e < a.n) {
    RouteOut o;
    const bool has_type = a.types != nullptr;
    const uint32_t type = has_type ? a.types[e] : 0u;
    if (!has_type || type == kRouteTypeData) { // (only then are the offset and the length looked at)
      off = a.body_off[e];
      len = a.body_len[e];
    }
    pending = route_precheck(has_type, type, off, len, a.bodies_bytes, &o);
    if (!pending) put(a, e, o);
  }
  const LdsTab tab{s_moff, reinterpret_cast<const uint8_t *>(s_names)};
  stage_rounds(a.bodies, a.bodies_bytes, off, len, pending,
               [&](LdsBody &body) { put(a, e, route_one(body, len, tab, a.nmethods, a.method_bytes)); });
}

// ---- groups: a stable counting sort over buckets x workgroups -------------------
// A lane's rank inside its workgroup among the entries of its bucket, and (for
// the count pass) the workgroup's count per bucket in s_cnt[wave][bucket]:
// inside a wave from ballots over the distinct buckets present, across the
// waves from the per-wave counts.
__device__ __forceinline__ uint32_t group_rank(uint32_t b, uint32_t nb, uint32_t (*s_cnt)[kRouteMaxMethods + 3]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  for (uint32_t i = t; i < kRouteWaves * (kRouteMaxMethods + 3); i += kRouteThreads)
    s_cnt[i / (kRouteMaxMethods + 3)][i % (kRouteMaxMethods + 3)] = 0;
  __syncthreads();
  uint32_t rank = 0;
  uint64_t left = __ballot(b != kRouteNoBucket);
  while (left) {
    const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
    const uint32_t b0 = (uint32_t)__shfl((int)b, (int)leader, 64);
    const uint64_t same = __ballot(b == b0);
    if (b == b0) {
      rank = route_wave_rank(same, lane);
      if (lane == leader) s_cnt[wave][b0] = (uint32_t)__popcll(same);
    }
    left &= ~same;
  }
  __syncthreads();
  if (b != kRouteNoBucket)
    for (uint32_t w = 0; w < wave; ++w) rank += s_cnt[w][b];
  return rank;
}

__global__ __launch_bounds__(kRouteThreads) void route_count_kernel(RouteArgs a, uint64_t nwg) {
  __shared__ uint32_t s_cnt[kRouteWaves][kRouteMaxMethods + 3];
  const uint64_t e = (uint64_t)blockIdx.x * kRouteEntries + threadIdx.x;
  const uint32_t nb = route_buckets(a.nmethods);
  const uint32_t b = e < a.n ? a.bucket[e] : kRouteNoBucket;
  (void)group_rank(b, nb, s_cnt);
  for (uint32_t k = threadIdx.x; k < nb; k += kRouteThreads) {
    uint32_t c = 0;
    for (uint32_t w = 0; w < kRouteWaves; ++w) c += s_cnt[w][k];
    a.counts[(uint64_t)k * nwg + blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kRouteThreads) void route_scatter_kernel(RouteArgs a, uint64_t nwg) {
  __shared__ uint32_t s_cnt[kRouteWaves][kRouteMaxMethods + 3];
  const uint64_t e = (uint64_t)blockIdx.x * kRouteEntries + threadIdx.x;
  const uint32_t nb = route_buckets(a.nmethods);
  const uint32_t b = e < a.n ? a.bucket[e] : kRouteNoBucket;
  const uint32_t rank = group_rank(b, nb, s_cnt);
  if (b != kRouteNoBucket) a.order[a.offs[(uint64_t)b * nwg + blockIdx.x] + rank] = (uint32_t)e;
  if (blockIdx.x == 0)
    for (uint32_t k = threadIdx.x; k <= nb; k += kRouteThreads) a.group_first[k] = (uint32_t)a.offs[(uint64_t)k * nwg];
}

} // namespace

hipError_t launch_frames_route(const RouteArgs &a, hipStream_t s) {
  const uint64_t nwg = route_workgroups(a.n);
  hipLaunchKernelGGL(route_kernel, dim3((unsigned)nwg), dim3(kRouteThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.order) return e;
  hipLaunchKernelGGL(route_count_kernel, dim3((unsigned)nwg), dim3(kRouteThreads), 0, s, a, nwg);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = excl_scan(a.counts, a.offs, route_buckets(a.nmethods) * nwg, a.scan_tmp, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(route_scatter_kernel, dim3((unsigned)nwg), dim3(kRouteThreads), 0, s, a, nwg);
  return hipGetLastError();
}

} // namespace rpccrc
