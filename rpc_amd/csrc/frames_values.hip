// rpc_amd/csrc/frames_values.hip -- device-side frame values
// (rpc_frames_values_device; the rules, the number formatting, the generated
// bytes and the splice policy: frames_values.h; the piece resolver, the tile
// function and the launch sequence's tail: frames_splice.h; the tile driver:
// frames_tile.h).
//
//   size pass (-> the grid's scan of very long strings) -> exclusive scan (the layout)
//   -> values kernel -> finish pass
#include "../../include/rpccrc.h"
#include "frames_values.h"

namespace rpccrc {

static_assert(kValuesNone == RPC_VALUES_NONE && kValuesOk == RPC_VALUES_OK && kValuesText == RPC_VALUES_TEXT &&
                  kValuesDefer == RPC_VALUES_DEFER && kValuesRange == RPC_VALUES_RANGE &&
                  kValuesBadSchema == RPC_VALUES_BAD_SCHEMA && kValuesNoRoom == RPC_VALUES_NO_ROOM,
              "frames_values.h restates the statuses");
static_assert(kValuesModeNone == RPC_VALUES_MODE_NONE && kValuesModeEncode == RPC_VALUES_MODE_ENCODE &&
                  kValuesModeText == RPC_VALUES_MODE_TEXT && kValuesFormResult == RPC_VALUES_FORM_RESULT &&
                  kValuesFormParams == RPC_VALUES_FORM_PARAMS,
              "the modes and the forms");

namespace {

constexpr int kValuesThreads = 256; // the size pass and the scan of very long strings
// A string up to this long is scanned by its entry's lane; a longer one by the
// whole workgroup, sixteen bytes per lane and round.
constexpr uint32_t kLaneScan = 256;
constexpr uint32_t kLongQueue = 64; // long strings a workgroup queues; further ones are scanned by their lane
// A string longer than this goes on the call's work list and is scanned by the
// whole grid, a chunk of this size per workgroup and round (values_long_kernel).
constexpr uint32_t kGridScan = 65536;
constexpr unsigned kLongGrid = 2048, kFixGrid = 64;

// The powers of five, as frames_args.hip keeps them: in global memory.
__device__ const uint64_t g_values_pow10[2 * (kPow10Max - kPow10Min + 1)] = {RPCCRC_POW10_WORDS};
struct DevPow {
  __device__ __forceinline__ uint64_t word(uint32_t i) const { return g_values_pow10[i]; }
};

struct DevSchema {
  const ValuesArgs &a;
  __device__ __forceinline__ uint32_t first(uint32_t m) const { return a.param_first[m]; }
  __device__ __forceinline__ uint32_t type(uint32_t p) const { return a.param_types[p]; }
  __device__ __forceinline__ uint32_t name_off(uint32_t p) const { return a.param_name_off[p]; }
  __device__ __forceinline__ uint32_t name(uint32_t b) const { return a.param_names[b]; }
  __device__ __forceinline__ uint32_t result_type(uint32_t m) const { return a.result_types[m]; }
};
struct DevIn {
  const ValuesArgs &a;
  uint64_t i;
  __device__ __forceinline__ uint8_t mode() const { return a.mode ? a.mode[i] : kValuesModeEncode; }
  __device__ __forceinline__ int32_t status() const { return a.status ? a.status[i] : 0; }
  __device__ __forceinline__ uint32_t method() const { return a.method[i]; }
  __device__ __forceinline__ uint64_t slot(uint32_t k) const { return a.slots[(uint64_t)k * a.n + i]; }
  __device__ __forceinline__ uint64_t str_base() const { return a.str_base ? a.str_base[i] : 0; }
  __device__ __forceinline__ bool has_text() const { return a.text_off && a.text_len; }
  __device__ __forceinline__ uint64_t text_off() const { return a.text_off[i]; }
  __device__ __forceinline__ uint32_t text_len() const { return a.text_len[i]; }
};

// No byte of strings[off, off + len) needs an escape: the bytes in front of the
// first aligned word, whole aligned words, the bytes behind the last.  (Only
// bytes of the span are read.)
__device__ __forceinline__ bool scan_clean(const uint8_t *strings, uint64_t off, uint64_t len) {
  const uint8_t *p = strings + off, *const end = p + len;
  while (p < end && (reinterpret_cast<uintptr_t>(p) & 3u)) {
    if (values_needs_escape(*p)) return false;
    ++p;
  }
  for (; end - p >= 4; p += 4)
    if (!route_plain4(*reinterpret_cast<const uint32_t *>(p))) return false;
  for (; p < end; ++p)
    if (values_needs_escape(*p)) return false;
  return true;
}
// This lane's share of strings[off, off + len) scanned by the whole workgroup:
// the unaligned head and tail bytewise by lanes 0 and 1, the aligned sixteen
// bytes between them by all.  False: this lane met a byte that needs an escape.
__device__ __forceinline__ bool wg_scan_clean(const uint8_t *strings, uint64_t off, uint64_t len) {
  const uint8_t *const p = strings + off;
  const uint64_t to16 = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u;
  const uint64_t head = len < to16 ? len : to16;
  const uint64_t blocks = (len - head) / 16, tail_at = head + blocks * 16;
  bool bad = false;
  if (threadIdx.x == 0) bad = !scan_clean(strings, off, head);
  if (threadIdx.x == 1) bad = !scan_clean(strings, off + tail_at, len - tail_at);
  for (uint64_t b = threadIdx.x; b < blocks && !bad; b += blockDim.x) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p + head + b * 16);
    bad = !(route_plain4(v.x) && route_plain4(v.y) && route_plain4(v.z) && route_plain4(v.w));
  }
  return !bad;
}
// The strings of one lane's entry: a short one is scanned here, a long one is
// queued for the workgroup (and counts as clean until it has been scanned).
struct DevStr {
  const ValuesArgs &a;
  uint64_t entry;
  const uint8_t *strings;
  uint32_t *q_count;
  uint64_t *q_off;
  uint32_t *q_len, *q_lane;
  __device__ __forceinline__ bool clean(uint64_t off, uint32_t len) const {
    if (len > kGridScan) { // (one record per STR item at the most: the list holds `items`)
      const uint32_t w = atomicAdd(a.long_count, 1u);
      a.long_off[w] = off, a.long_len[w] = len, a.long_entry[w] = (uint32_t)entry, a.long_bad[w] = 0;
      return true;
    }
    if (len > kLaneScan) {
      const uint32_t at = atomicAdd(q_count, 1u);
      if (at < kLongQueue) {
        q_off[at] = off, q_len[at] = len, q_lane[at] = threadIdx.x;
        return true;
      }
    }
    return scan_clean(strings, off, len);
  }
};
struct DevSink {
  const ValuesArgs &a;
  uint64_t base;
  __device__ __forceinline__ void item(uint32_t k, uint64_t size, uint64_t src, uint32_t meta) const {
    a.sizes[base + k] = size, a.src_off[base + k] = src, a.meta[base + k] = meta;
  }
  __device__ __forceinline__ void text(uint32_t k, const ValText &t) const {
    a.text0[base + k] = t.w0, a.text1[base + k] = t.w1, a.text2[base + k] = t.w2;
  }
};

// ---- size pass: one lane per entry, the workgroup for the long strings ---------
__global__ __launch_bounds__(kValuesThreads) void values_size_kernel(ValuesArgs a) {
  __shared__ uint32_t s_count, s_len[kLongQueue], s_lane[kLongQueue], s_bad[kValuesThreads];
  __shared__ uint64_t s_off[kLongQueue];
  if (threadIdx.x == 0) s_count = 0;
  s_bad[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kValuesThreads + threadIdx.x;
  uint8_t st = kValuesNone;
  uint32_t used = 0;
  if (i < a.n) {
    DevSink sink{a, i * a.unit};
    st = values_entry(DevIn{a, i}, a.form, DevSchema{a}, a.nmethods, a.nparams, a.name_bytes, a.width, a.strings_bytes,
                      a.texts_bytes, DevPow{}, DevStr{a, i, a.strings, &s_count, s_off, s_len, s_lane}, sink, &used);
  }
  __syncthreads();
  const uint32_t queued = s_count < kLongQueue ? s_count : kLongQueue;
  for (uint32_t q = 0; q < queued; ++q) { // (uniform: every lane of the workgroup takes part)
    const bool bad = !wg_scan_clean(a.strings, s_off[q], s_len[q]);
    if (bad) s_bad[s_lane[q]] = 1; // (every writer stores the same word)
  }
  __syncthreads();
  if (i < a.n) {
    if (st == kValuesOk && s_bad[threadIdx.x]) st = kValuesDefer;
    a.pre[i] = st;
    for (uint32_t k = (st == kValuesOk || st == kValuesText) ? used : 0u; k < a.unit; ++k) a.sizes[i * a.unit + k] = 0;
  }
}

// ---- the work list of very long strings: the whole grid scans, then the entries are set right ----
__global__ __launch_bounds__(kValuesThreads) void values_long_kernel(ValuesArgs a) {
  const uint32_t count = *a.long_count;
  for (uint32_t w = 0; w < count; ++w) {
    const uint64_t off = a.long_off[w], len = a.long_len[w];
    // string w's chunk c goes to workgroup (c + w) mod the grid: many strings of a
    // few chunks each spread over the grid as a few strings of many chunks do
    const uint64_t first = (blockIdx.x + gridDim.x - w % gridDim.x) % gridDim.x;
    for (uint64_t at = first * kGridScan; at < len; at += (uint64_t)gridDim.x * kGridScan) {
      const uint64_t part = len - at < kGridScan ? len - at : kGridScan;
      if (!wg_scan_clean(a.strings, off + at, part)) a.long_bad[w] = 1; // (every writer stores the same word)
    }
  }
}
__global__ __launch_bounds__(256) void values_fix_kernel(ValuesArgs a) {
  const uint32_t count = *a.long_count;
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < count; w += gridDim.x * blockDim.x) {
    if (!a.long_bad[w]) continue;
    const uint64_t e = a.long_entry[w];
    if (a.pre[e] != kValuesOk && a.pre[e] != kValuesDefer) continue;
    a.pre[e] = kValuesDefer; // (two strings of one entry store the same words)
    for (uint32_t k = 0; k < a.unit; ++k) a.sizes[e * a.unit + k] = 0;
  }
}

// ---- values kernel -------------------------------------------------------------------
struct DevEnt {
  const ValuesArgs &a;
  bool all_fit; // the total lies inside out_cap: every entry is written
  __device__ __forceinline__ uint32_t meta(uint64_t u) const { return a.meta[u]; }
  __device__ __forceinline__ uint64_t text(uint64_t u, uint32_t j) const {
    return j == 0 ? a.text0[u] : j == 1 ? a.text1[u] : a.text2[u];
  }
  __device__ __forceinline__ bool written(uint64_t u) const {
    return all_fit || a.offs[(u / a.unit + 1) * a.unit] <= a.out_cap;
  }
};

// One workgroup per tile of kPackTile output bytes (striding when the grid is
// smaller), as the reply kernel, over the items in place of the entries.
__global__ __launch_bounds__(kSpliceThreads) void values_kernel(ValuesArgs a) {
  __shared__ uint64_t s_range[2];
  __shared__ uint64_t s_off[kTileLdsEntries], s_src[kTileLdsEntries];
  const DevSrc strings{a.strings, a.strings_bytes}, texts{a.texts, a.texts_bytes};
  const DevEnt ent{a, a.offs[a.items] <= a.out_cap};
  const DevSchema sc{a};
  const ValuesSplice<DevEnt, DevSchema, DevSrc> pol{ent, sc, strings, texts};
  // (the walker's loads are relative to the strings)
  tile_drive<kSpliceThreads>(a.offs, a.src_off, a.items, a.out, a.out_cap, s_range, s_off, s_src,
                             [&](const auto off, const auto src_of, auto... tile) {
                               splice_tile(pol, a.strings, off, src_of, tile...);
                             });
}

// ---- finish: statuses, the reply's status words, layout, the DEFER count, total ----
__global__ __launch_bounds__(256) void values_finish_kernel(ValuesArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && a.total) *a.total = a.offs[a.items];
  bool defer = false;
  if (i < a.n) {
    const uint64_t at = a.offs[i * a.unit], size = a.offs[(i + 1) * a.unit] - at;
    const uint8_t st = values_final_status(a.pre[i], at, size, a.out_cap);
    defer = st == kValuesDefer;
    if (a.value_off) a.value_off[i] = at;
    if (a.value_len) a.value_len[i] = (uint32_t)size;
    if (a.values_status) a.values_status[i] = st;
    if (a.reply_status) a.reply_status[i] = values_reply_status(st, a.status ? a.status[i] : 0);
  }
  if (a.ndefer) { // one add per wave that has any
    const uint64_t votes = __ballot(defer);
    if (votes && (threadIdx.x & 63u) == 0) atomicAdd(a.ndefer, (uint32_t)__popcll(votes));
  }
}

} // namespace

hipError_t launch_frames_values(const ValuesArgs &a, hipStream_t s) {
  hipError_t e;
  if (a.ndefer && (e = hipMemsetAsync(a.ndefer, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.long_count, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(values_size_kernel, grid_of(a.n, kValuesThreads), dim3(kValuesThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.strings_bytes > kGridScan) { // (only then can a string be on the work list)
    hipLaunchKernelGGL(values_long_kernel, dim3(kLongGrid), dim3(kValuesThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(values_fix_kernel, dim3(kFixGrid), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return splice_launch_tail(a, a.items, a.n, values_kernel, values_finish_kernel, s);
}

} // namespace rpccrc
