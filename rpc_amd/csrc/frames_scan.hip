// rpc_amd/csrc/frames_scan.hip -- device-side frame scan (rpc_frames_scan_device;
// the rules and the tiled route's algebra: frames_scan.h).
//
// Every stage is count -> exclusive scan -> emit over work units: a unit is a
// connection on the serial route or a tile of a tiled connection.  The units
// count their frames, a device-wide exclusive scan gives the emit bases,
// d_conn_first and d_nframes, and the units walk again and write.
#include "../../include/rpccrc.h"
#include "frames_scan.h"
#include "frames_tile.h" // grid_of

namespace rpccrc {

static_assert(kScanServer == RPC_FRAMES_SERVER && kScanClient == RPC_FRAMES_CLIENT &&
                  kScanLiftCap == RPC_FRAMES_LIFT_CAP,
              "frames_scan.h restates the flag bits");
static_assert(kScanTypePing == RPC_FRAME_TYPE_PING && kScanTypePong == RPC_FRAME_TYPE_PONG, "and the type codes");
static_assert(kScanMaxBody == RPC_MAX_BODY_LEN, "and the cap");

namespace {

constexpr uint32_t T = kScanTile;
constexpr uint32_t G = kScanGroup;
constexpr int kUnitThreads = 64;   // one wave per workgroup: the walks spread over every CU
constexpr int kTileThreads = 256;
constexpr uint32_t kChunk = 2048;  // words per workgroup of the exclusive scan: 256 threads x 8

// ---- exclusive scan over uint64 words ---------------------------------------
// out[i] = in[0] + ... + in[i-1] within the workgroup's chunk.  sums != nullptr:
// sums[block] = the chunk's total.  sums == nullptr (one workgroup): out[n] = total.
__global__ __launch_bounds__(256) void excl_scan_kernel(const uint64_t *in, uint64_t *out, uint64_t n,
                                                        uint64_t *sums) {
  __shared__ uint64_t part[256];
  const uint32_t t = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * kChunk + (uint64_t)t * 8;
  uint64_t v[8], own = 0;
  for (int i = 0; i < 8; ++i) {
    v[i] = base + i < n ? in[base + i] : 0;
    own += v[i];
  }
  part[t] = own;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) { // Hillis-Steele over the 256 thread sums
    const uint64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  uint64_t run = part[t] - own;
  for (int i = 0; i < 8; ++i) {
    if (base + i < n) out[base + i] = run;
    run += v[i];
  }
  if (t == 255) {
    if (sums)
      sums[blockIdx.x] = part[255];
    else
      out[n] = part[255];
  }
}
// out[i] += chunk_base[i / kChunk]; out[n] = chunk_base[nb].
__global__ __launch_bounds__(256) void scan_add_kernel(uint64_t *out, uint64_t n, const uint64_t *chunk_base,
                                                       uint64_t nb) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] += chunk_base[i / kChunk];
  if (i == 0) out[n] = chunk_base[nb];
}
} // namespace

// (declared in excl_scan.h: the frame pack scans its sizes with it too)
hipError_t excl_scan(const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *tmp, hipStream_t s) {
  const uint64_t nb = (n + kChunk - 1) / kChunk;
  if (nb <= 1) {
    hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(256), 0, s, in, out, n, (uint64_t *)nullptr);
    return hipGetLastError();
  }
  uint64_t *sums = tmp, *scanned = tmp + nb, *rest = tmp + 2 * nb + 1;
  hipLaunchKernelGGL(excl_scan_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, out, n, sums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = excl_scan(sums, scanned, nb, rest, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, scanned, nb);
  return hipGetLastError();
}

namespace {
// ---- the routes ---------------------------------------------------------------
struct GlobalRd { // byte q of a connection, straight from global memory
  const uint8_t *b;
  __device__ __forceinline__ uint8_t operator()(uint64_t q) const { return b[q]; }
};
struct LdsRd { // byte q of a connection whose bytes from t0 on are in LDS at `b`
  const uint8_t *b;
  uint64_t t0;
  __device__ __forceinline__ uint8_t operator()(uint64_t q) const { return b[(uint32_t)(q - t0)]; }
};
struct EmitSink { // frame k of this walk at connection offset q
  uint64_t *frame_off;
  uint32_t *frame_conn;
  uint64_t frame_cap, base, conn_off;
  uint32_t conn;
  __device__ __forceinline__ void operator()(uint64_t k, uint64_t q) const {
    const uint64_t i = base + k;
    if (i >= frame_cap) return; // nothing is ever written at index >= frame_cap
    if (frame_off) frame_off[i] = conn_off + q;
    if (frame_conn) frame_conn[i] = conn;
  }
};

__device__ __forceinline__ bool conn_inside(const ScanArgs &a, uint64_t off, uint64_t len) {
  return off <= a.stream_bytes && len <= a.stream_bytes - off;
}
// (after the tile-count scan) does connection c take the tiled route?
__device__ __forceinline__ bool conn_tiled(const ScanArgs &a, uint64_t c) {
  return a.tile_cap != 0 && a.conn_tiles[c] != 0 && a.tbase[c + 1] <= a.tile_cap;
}

// Tiles each connection wants: 0 for the serial route.
__global__ __launch_bounds__(256) void scan_classify_kernel(ScanArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) *a.nt_live = 0;
  if (c >= a.nconn) return;
  const uint64_t off = a.conn_off[c], len = a.conn_len[c];
  uint64_t want = 0;
  if (conn_inside(a, off, len) && len > a.tiled_min) {
    want = scan_tiles_of<T>(len);
    if (want > a.tile_cap) want = a.tile_cap + 1; // cannot fit (and the sum cannot overflow)
  }
  a.conn_tiles[c] = want;
}
// tbase is monotone, so the connections whose tiles fit are a prefix of those
// that want tiles: the live tiles are [0, the largest fitting tbase[c + 1]).
__global__ __launch_bounds__(256) void scan_live_kernel(ScanArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nconn) return;
  if (conn_tiled(a, c)) atomicMax(reinterpret_cast<unsigned long long *>(a.nt_live), (unsigned long long)a.tbase[c + 1]);
}

// Tile pass: one workgroup per tile.  The tile and its 7-byte halo go to LDS
// through aligned 16-byte loads (a 16-byte block that holds one byte of the
// stream lies in the stream's pages); one thread per entry walks its chain in
// LDS (kTileThreads threads, entries dealt round-robin).
__global__ __launch_bounds__(kTileThreads) void scan_tile_kernel(ScanArgs a) {
  __shared__ uint4 lds4[(T + 32) / 16];
  __shared__ uint32_t s_conn;
  __shared__ uint16_t s_first;
  const uint64_t j = blockIdx.x;
  if (j >= *a.nt_live) return;
  if (threadIdx.x == 0) {
    const uint32_t c = (uint32_t)scan_find_conn(a.tbase, a.nconn, j);
    s_conn = c;
    a.tconn[j] = c;
  }
  __syncthreads();
  const uint64_t c = s_conn;
  const uint64_t k = j - a.tbase[c], len = a.conn_len[c];
  const uint64_t t0 = k * T; // <= len
  const uint8_t *src = a.stream + a.conn_off[c] + t0;
  const uint64_t left = len - t0;
  const uint32_t nbytes = (uint32_t)(left < (uint64_t)T + kScanHalo ? left : (uint64_t)T + kScanHalo);
  const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint32_t nvec = nbytes ? (shift + nbytes + 15) / 16 : 0; // <= T / 16 + 2
  const uint4 *src4 = reinterpret_cast<const uint4 *>(src - shift);
  for (uint32_t v = threadIdx.x; v < nvec; v += kTileThreads) lds4[v] = src4[v];
  __syncthreads();
  const LdsRd rd{reinterpret_cast<const uint8_t *>(lds4) + shift, t0};
  uint16_t *m = a.maps[0] + j * kScanMapLen;
  if (k == 0) { // a connection's first tile: the constant map (frames_scan.h)
    if (threadIdx.x == 0) s_first = scan_tile_exit<T>(rd, t0, 0, len, a.flags);
    __syncthreads();
    const uint16_t x = s_first;
    for (uint32_t e = threadIdx.x; e < kScanMapLen; e += kTileThreads) m[e] = x;
    return;
  }
  for (uint32_t e = threadIdx.x; e < kScanEntries; e += kTileThreads) m[e] = scan_tile_exit<T>(rd, t0, e, len, a.flags);
  if (threadIdx.x == 0) m[kScanStop] = (uint16_t)kScanStop;
}

// Up-sweep, level `level` >= 1: map g is the composition of maps g*G .. of the
// level below, held in LDS.
__global__ __launch_bounds__(256) void scan_up_kernel(ScanArgs a, int level) {
  __shared__ uint16_t lm[G * kScanMapLen];
  const uint64_t g = blockIdx.x;
  const uint64_t n_below = scan_level_count<G>(*a.nt_live, (uint32_t)level - 1);
  if (g * G >= n_below) return;
  const uint32_t count = (uint32_t)(n_below - g * G < G ? n_below - g * G : G);
  const uint16_t *below = a.maps[level - 1] + g * G * kScanMapLen;
  for (uint32_t i = threadIdx.x; i < count * kScanMapLen; i += 256) lm[i] = below[i];
  __syncthreads();
  uint16_t *m = a.maps[level] + g * kScanMapLen;
  for (uint32_t e = threadIdx.x; e < kScanMapLen; e += 256) m[e] = scan_compose(lm, count, e);
}
// Down-sweep to level `level` (from a.levels - 1 down to 0): one lane per group.
// The one group of the top level is entered "stopped": its first map is a
// connection's first tile (or a composition that starts with one), which
// ignores its entry.
__global__ __launch_bounds__(kUnitThreads) void scan_down_kernel(ScanArgs a, int level) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n_here = scan_level_count<G>(*a.nt_live, (uint32_t)level);
  if (g * G >= n_here) return;
  const uint32_t count = (uint32_t)(n_here - g * G < G ? n_here - g * G : G);
  const uint32_t e = (level + 1 == a.levels) ? kScanStop : a.entry[level + 1][g];
  scan_resolve(a.maps[level] + g * G * kScanMapLen, count, e, a.entry[level] + g * G);
}

// Count (EMIT = false) and emit (EMIT = true): unit u < nconn is connection u
// (its serial walk, if it takes that route), unit nconn + j is tile j.
template <bool EMIT>
__global__ __launch_bounds__(kUnitThreads) void scan_units_kernel(ScanArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u < a.nconn) {
    const uint64_t c = u, off = a.conn_off[c], len = a.conn_len[c];
    if (!conn_inside(a, off, len)) { // not inside the stream: closed, nothing consumed
      if (!EMIT) {
        a.conn_cnt[c] = 0;
        a.consumed[c] = 0;
        a.state[c] = RPC_CONN_CLOSED;
      }
      return;
    }
    if (conn_tiled(a, c)) return; // (its tiles do the work; scan_conn_total_kernel sums them)
    const GlobalRd rd{a.stream + off};
    if (!EMIT) {
      const ScanWalk w = scan_walk(rd, 0, ~0ull, len, a.flags, ScanNoSink{});
      a.conn_cnt[c] = w.count;
      a.consumed[c] = w.p;
      a.state[c] = w.closed ? RPC_CONN_CLOSED : RPC_CONN_OPEN;
    } else {
      const EmitSink sink{a.frame_off, a.frame_conn, a.frame_cap, a.conn_first[c], off, (uint32_t)c};
      (void)scan_walk(rd, 0, ~0ull, len, a.flags, sink);
    }
    return;
  }
  const uint64_t j = u - a.nconn;
  if (j >= a.tile_cap) return;
  uint64_t cnt = 0;
  if (j < *a.nt_live) {
    const uint64_t c = a.tconn[j];
    const uint64_t k = j - a.tbase[c];
    const uint32_t e = k == 0 ? 0u : a.entry[0][j];
    if (e != kScanStop) { // the true chain reaches this tile
      const uint64_t off = a.conn_off[c], len = a.conn_len[c], t0 = k * T;
      const GlobalRd rd{a.stream + off};
      if (!EMIT) {
        const ScanWalk w = scan_walk(rd, t0 + e, t0 + T, len, a.flags, ScanNoSink{});
        cnt = w.count;
        if (w.stopped) { // exactly one tile of a connection meets its stop
          a.consumed[c] = w.p;
          a.state[c] = w.closed ? RPC_CONN_CLOSED : RPC_CONN_OPEN;
        }
      } else {
        const uint64_t base = a.conn_first[c] + (a.tpre[j] - a.tpre[a.tbase[c]]);
        const EmitSink sink{a.frame_off, a.frame_conn, a.frame_cap, base, off, (uint32_t)c};
        (void)scan_walk(rd, t0 + e, t0 + T, len, a.flags, sink);
      }
    }
  }
  if (!EMIT) a.tile_cnt[j] = cnt;
}
// A tiled connection's frames: the sum over its tiles.
__global__ __launch_bounds__(256) void scan_conn_total_kernel(ScanArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nconn) return;
  if (conn_tiled(a, c)) a.conn_cnt[c] = a.tpre[a.tbase[c + 1]] - a.tpre[a.tbase[c]];
}
// *nframes, and the padding behind the frames found: offset stream_bytes (which
// rpc_frames_verify_device calls MALFORMED with no body read), connection ~0.
__global__ __launch_bounds__(256) void scan_finish_kernel(ScanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nf = a.conn_first[a.nconn];
  if (i == 0) *a.nframes = nf;
  if (i >= nf && i < a.frame_cap) {
    if (a.frame_off) a.frame_off[i] = a.stream_bytes;
    if (a.frame_conn) a.frame_conn[i] = 0xFFFFFFFFu;
  }
}

// ---- reach pass -----------------------------------------------------------------
__global__ __launch_bounds__(256) void reach_init_kernel(uint64_t *first_close, uint64_t nconn) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nconn) first_close[c] = ~0ull;
}
__device__ __forceinline__ bool closes(uint8_t v) {
  return v == RPC_FRAME_BAD_CRC || v == RPC_FRAME_TOO_LARGE || v == RPC_FRAME_RECV_ERR;
}
__global__ __launch_bounds__(256) void reach_min_kernel(const uint32_t *frame_conn, uint64_t frame_cap,
                                                        const uint64_t *nframes, const uint8_t *verdict,
                                                        uint64_t *first_close) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= frame_cap || i >= *nframes) return;
  if (closes(verdict[i]))
    atomicMin(reinterpret_cast<unsigned long long *>(first_close + frame_conn[i]), (unsigned long long)i);
}
__global__ __launch_bounds__(256) void reach_rewrite_kernel(const uint32_t *frame_conn, uint64_t frame_cap,
                                                            const uint64_t *nframes, const uint64_t *first_close,
                                                            uint8_t *verdict, uint32_t *crc, uint8_t *state) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= frame_cap || i >= *nframes) return;
  const uint32_t c = frame_conn[i];
  const uint64_t f = first_close[c];
  if (i > f) {
    verdict[i] = RPC_FRAME_NOT_REACHED;
    if (crc) crc[i] = 0;
  } else if (i == f && verdict[i] == RPC_FRAME_BAD_CRC) {
    state[c] = RPC_CONN_CLOSED;
  }
}

#define SCAN_LAUNCH(kernel, grid, block, ...)                      \
  do {                                                             \
    hipLaunchKernelGGL(kernel, grid, block, 0, s, __VA_ARGS__);    \
    const hipError_t _e = hipGetLastError();                       \
    if (_e != hipSuccess) return _e;                               \
  } while (0)

} // namespace

uint64_t scan_tmp_words(uint64_t n) {
  const uint64_t nb = (n + kChunk - 1) / kChunk;
  return nb <= 1 ? 1 : 2 * nb + 1 + scan_tmp_words(nb);
}

int scan_levels_for(uint64_t tile_cap) {
  int L = 1;
  while (scan_level_count<G>(tile_cap, (uint32_t)L) > 1) ++L;
  return L;
}

hipError_t launch_frames_scan(const ScanArgs &a, hipStream_t s) {
  hipError_t e;
  if (a.tile_cap) {
    SCAN_LAUNCH(scan_classify_kernel, grid_of(a.nconn, 256), dim3(256), a);
    if ((e = excl_scan(a.conn_tiles, a.tbase, a.nconn, a.scan_tmp, s)) != hipSuccess) return e;
    SCAN_LAUNCH(scan_live_kernel, grid_of(a.nconn, 256), dim3(256), a);
    SCAN_LAUNCH(scan_tile_kernel, dim3((unsigned)a.tile_cap), dim3(kTileThreads), a);
    for (int l = 1; l < a.levels; ++l)
      SCAN_LAUNCH(scan_up_kernel, dim3((unsigned)scan_level_count<G>(a.tile_cap, (uint32_t)l)), dim3(256), a, l);
    for (int l = a.levels - 1; l >= 0; --l)
      SCAN_LAUNCH(scan_down_kernel, grid_of(scan_level_count<G>(a.tile_cap, (uint32_t)l + 1), kUnitThreads),
                  dim3(kUnitThreads), a, l);
  }
  const uint64_t units = a.nconn + a.tile_cap;
  SCAN_LAUNCH(scan_units_kernel<false>, grid_of(units, kUnitThreads), dim3(kUnitThreads), a);
  if (a.tile_cap) {
    if ((e = excl_scan(a.tile_cnt, a.tpre, a.tile_cap, a.scan_tmp, s)) != hipSuccess) return e;
    SCAN_LAUNCH(scan_conn_total_kernel, grid_of(a.nconn, 256), dim3(256), a);
  }
  if ((e = excl_scan(a.conn_cnt, a.conn_first, a.nconn, a.scan_tmp, s)) != hipSuccess) return e;
  if (a.frame_cap) SCAN_LAUNCH(scan_units_kernel<true>, grid_of(units, kUnitThreads), dim3(kUnitThreads), a);
  SCAN_LAUNCH(scan_finish_kernel, grid_of(a.frame_cap ? a.frame_cap : 1, 256), dim3(256), a);
  return hipSuccess;
}

hipError_t launch_frames_reach(const uint32_t *frame_conn, uint64_t frame_cap, const uint64_t *nframes, uint64_t nconn,
                               uint64_t *first_close, uint8_t *verdict, uint32_t *crc, uint8_t *state, hipStream_t s) {
  SCAN_LAUNCH(reach_init_kernel, grid_of(nconn, 256), dim3(256), first_close, nconn);
  SCAN_LAUNCH(reach_min_kernel, grid_of(frame_cap, 256), dim3(256), frame_conn, frame_cap, nframes, verdict,
              first_close);
  SCAN_LAUNCH(reach_rewrite_kernel, grid_of(frame_cap, 256), dim3(256), frame_conn, frame_cap, nframes, first_close,
              verdict, crc, state);
  return hipSuccess;
}

} // namespace rpccrc
