// rpc_amd/csrc/frames_route.hip -- device-side frame route
// (rpc_frames_route_device; the rules, the automaton and the method compare:
// frames_route.h).
//
//   route kernel [-> bucket counts -> exclusive scan -> scatter]
#include <algorithm>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames_route.h"

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
constexpr uint32_t kNone32 = 0xFFFFFFFFu;

// A staged body: the lane walks it word by word (one aligned LDS read per four
// bytes; a byte read per byte at 64 unrelated addresses would be four times the
// LDS instructions and their bank conflicts).
struct LdsBody {
  const uint32_t *lds;
  uint32_t base; // byte offset of the body in the staging area
  uint32_t pos = 0, w = 0;
  __device__ __forceinline__ LdsBody(const uint32_t *l, uint32_t b) : lds(l), base(b) {}
  __device__ __forceinline__ uint32_t next() {
    const uint32_t p = base + pos;
    if ((p & 3u) == 0 || pos == 0) w = lds[p >> 2];
    ++pos;
    return (w >> (8 * (p & 3u))) & 0xFFu;
  }
  __device__ __forceinline__ bool aligned() const { return ((base + pos) & 3u) == 0; }
  __device__ __forceinline__ uint32_t word() const { return lds[(base + pos) >> 2]; }
  __device__ __forceinline__ void skip4() { pos += 4; }
  __device__ __forceinline__ uint32_t at(uint32_t i) const {
    const uint32_t p = base + i;
    return (lds[p >> 2] >> (8 * (p & 3u))) & 0xFFu;
  }
};
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

// One workgroup per kRouteEntries consecutive entries, one lane per entry.  The
// bodies are staged in LDS in rounds: a round's window starts at the 16-byte
// address step at or below the first pending body and takes every pending body
// that lies inside its kRouteStage bytes (the unpack's bodies are back to back:
// a run of consecutive entries; any other order still ends, a body per round at
// the least).  Whole 16-byte blocks inside the buffer come with aligned
// 16-byte loads, the edges that would leave [bodies, bodies + bodies_bytes)
// bytewise.  Then each lane of the round walks its own body in LDS.
__global__ __launch_bounds__(kRouteThreads) void route_kernel(RouteArgs a) {
  __shared__ uint4 s_stage[kRouteStage / 16];
  __shared__ uint32_t s_moff[kRouteMaxMethods + 1];
  __shared__ uint4 s_names[kRouteMaxMethodBytes / 16];
  __shared__ uint64_t s_off[kRouteEntries];
  __shared__ uint32_t s_first, s_end;
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
  s_off[t] = off;
  const uint64_t base_addr = (uint64_t)reinterpret_cast<uintptr_t>(a.bodies);
  const uint32_t mis = (uint32_t)(base_addr & 15u);
  const LdsTab tab{s_moff, reinterpret_cast<const uint8_t *>(s_names)};
  const uint32_t *stage32 = reinterpret_cast<const uint32_t *>(s_stage);

  for (;;) {
    if (t == 0) s_first = kNone32, s_end = 0;
    __syncthreads(); // (also: s_off and the table are written; the last round's walks are over)
    if (pending) atomicMin(&s_first, t);
    __syncthreads();
    const uint32_t first = s_first;
    if (first == kNone32) break;
    // the window in "aligned space": offsets from bodies - mis, so that a multiple
    // of 16 there is a 16-byte address step
    const uint64_t w0 = (s_off[first] + mis) & ~(uint64_t)15;
    const uint64_t x0 = off + mis;
    const bool mine = pending && x0 >= w0 && x0 + len <= w0 + kRouteStage;
    if (mine) atomicMax(&s_end, (uint32_t)(x0 + len - w0));
    __syncthreads();
    const uint32_t blocks = (s_end + 15u) / 16u; // >= 1: the first pending body is in
    const uint64_t lim = a.bodies_bytes + mis;   // the buffer is [mis, lim) in aligned space
    for (uint32_t k = t; k < blocks; k += kRouteThreads) {
      const uint64_t x = w0 + (uint64_t)k * 16u;
      if (x >= mis && x + 16u <= lim) {
        s_stage[k] = *reinterpret_cast<const uint4 *>(a.bodies + (x - mis));
      } else { // the buffer's first or last block: only its bytes inside the buffer
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t b = 0; b < 16; ++b)
          if (x + b >= mis && x + b < lim) w[b >> 2] |= (uint32_t)a.bodies[x + b - mis] << (8 * (b & 3u));
        s_stage[k] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    __syncthreads();
    if (mine) {
      LdsBody body(stage32, (uint32_t)(x0 - w0));
      put(a, e, route_one(body, len, tab, a.nmethods, a.method_bytes));
      pending = false;
    }
  }
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
