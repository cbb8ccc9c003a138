// rpc_amd/csrc/frames_api.cpp -- the rpc_frames_* entry points of librpccrc
// (include/rpccrc.h): the frame stages' host side.  Each entry point reads top
// to bottom as: its own argument checks, which need no device; the "nothing to
// do" return; open the context; the empty batch; the workspace, carved by the
// stage's layout function (beside its Args, in its header) out of one leased
// block; fill the Args; launch.  Reads no test hook: one object serves the
// product library and the test build.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../include/rpccrc.h"
#include "excl_scan.h"
#include "frames.h"
#include "frames_args.h"
#include "frames_carry.h"
#include "frames_pack.h"
#include "frames_reply.h"
#include "frames_request.h"
#include "frames_resolve.h"
#include "frames_results.h"
#include "frames_route.h"
#include "frames_scan.h"
#include "frames_unpack.h"
#include "frames_values.h"
#include "host_core.h"

namespace rpccrc {
namespace {

std::atomic<int> g_scan_path{RPCCRC_SCAN_AUTO}; // rpc_frames_set_scan_path

// What every entry point does between its argument checks and its first
// launch: the calling thread's device (RPCCRC_EIO while its error word is set)
// and the stream, then one leased block for the arrays that layout(WsLayout &)
// takes, returned when the call has enqueued its work.
struct FramesCall {
  DeviceCtx *c = nullptr;
  hipStream_t s = nullptr;
  Lease ws;
  int open(void *stream) {
    s = static_cast<hipStream_t>(stream);
    return get_async_ctx(&c);
  }
  template <class F> int workspace(F &&layout, size_t slack = 0) { return ws.get(ws_pool(*c), s, layout, slack); }
};

bool frames_flags_ok(int flags) {
  const int role = flags & (RPC_FRAMES_SERVER | RPC_FRAMES_CLIENT);
  return (flags & ~(RPC_FRAMES_SERVER | RPC_FRAMES_CLIENT | RPC_FRAMES_LIFT_CAP)) == 0 &&
         (role == RPC_FRAMES_SERVER || role == RPC_FRAMES_CLIENT);
}

// What rpc_frames_pack_device and rpc_frames_unpack_device ask of the arguments
// they have in common.
bool frames_layout_args_ok(uint64_t n, const uint8_t *d_out, uint64_t out_cap, const uint64_t *d_conn_first,
                           uint64_t nconn, const uint64_t *d_conn_bytes_first) {
  if (n >= 0xFFFFFFFFull) return false;
  if (out_cap > 0 && !d_out) return false;
  if (d_conn_bytes_first && !d_conn_first) return false;
  return nconn == 0 || d_conn_first;
}

// Their empty batch: every offset is 0.
int frames_layout_empty(uint64_t *d_total, uint64_t *d_conn_bytes_first, uint64_t nconn, hipStream_t s) {
  if (d_total) RPCCRC_TRY(hipMemsetAsync(d_total, 0, 8, s));
  if (d_conn_bytes_first) RPCCRC_TRY(hipMemsetAsync(d_conn_bytes_first, 0, (nconn + 1) * 8, s));
  return RPCCRC_OK;
}

} // namespace
} // namespace rpccrc

using namespace rpccrc;

// rpc_frames_scan_device, and with d_verdict the fused scan + verify + reach pass.
static int frames_scan_common(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_conn_off,
                              const uint64_t *d_conn_len, uint64_t nconn, int flags, uint64_t *d_frame_offsets,
                              uint32_t *d_frame_conn, uint64_t frame_cap, uint64_t *d_conn_first,
                              uint64_t *d_conn_consumed, uint8_t *d_conn_state, uint64_t *d_nframes, uint8_t *d_verdict,
                              uint32_t *d_crc, bool fused, void *stream) {
  if (!frames_flags_ok(flags)) return RPCCRC_EINVAL;
  if (!d_nframes || !d_conn_first || nconn >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (frame_cap != 0 && !d_frame_offsets) return RPCCRC_EINVAL;
  if (nconn != 0 && (!d_stream || !d_conn_off || !d_conn_len || !d_conn_consumed || !d_conn_state))
    return RPCCRC_EINVAL;
  if (fused && frame_cap != 0 && (!d_verdict || !d_stream || frame_cap >= 0xFFFFFFFFull)) return RPCCRC_EINVAL;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  const bool reach = fused && frame_cap != 0 && nconn != 0;

  ScanArgs a;
  a.stream = d_stream;
  a.stream_bytes = stream_bytes;
  a.conn_off = d_conn_off;
  a.conn_len = d_conn_len;
  a.nconn = nconn;
  a.flags = flags;
  a.frame_off = d_frame_offsets;
  a.frame_conn = d_frame_conn;
  a.frame_cap = frame_cap;
  a.conn_first = d_conn_first;
  a.consumed = d_conn_consumed;
  a.state = d_conn_state;
  a.nframes = d_nframes;

  // The tiled route: cap in force only, for connections longer than tiled_min.
  // Connections inside the stream that do not overlap need at most
  // stream_bytes / T + (one more per tiled connection) tiles; what does not
  // fit the workspace walks serially.
  const int path = g_scan_path.load(std::memory_order_relaxed);
  a.tiled_min = path == RPCCRC_SCAN_TILED ? kScanTile : kScanTiledMin;
  if (nconn != 0 && path != RPCCRC_SCAN_SERIAL && !(flags & RPC_FRAMES_LIFT_CAP) && stream_bytes > a.tiled_min) {
    uint64_t max_tiles = 1;
    for (uint32_t i = 0; i <= kScanMaxLevels; ++i) max_tiles *= kScanGroup;
    a.tile_cap = stream_bytes / kScanTile + std::min<uint64_t>(nconn, stream_bytes / a.tiled_min) + 1;
    a.tile_cap = std::min(a.tile_cap, max_tiles);
    a.levels = scan_levels_for(a.tile_cap);
    if (f.workspace([&](WsLayout &w) { scan_tiled_ws_layout(w, a); }) != RPCCRC_OK) {
      a.tile_cap = 0; // no workspace: every connection walks serially (results identical)
      a.levels = 0;
      (void)hipGetLastError(); // (the failed allocation's error is not the next launch's)
    }
  }

  Lease base; // (beside the tiled route's block, which f holds)
  const size_t tmp_words = scan_tmp_words(std::max(nconn, a.tile_cap));
  const bool own_conn = reach && !d_frame_conn;
  uint64_t *first_close = nullptr;
  // (nconn == 0 runs the same launches: no unit finds work, *d_nframes = 0,
  // every entry of d_frame_offsets is padding)
  const auto layout = [&](WsLayout &w) { scan_ws_layout(w, a, tmp_words, reach, own_conn, first_close); };
  if ((rc = base.get(ws_pool(*f.c), f.s, layout, 256))) return rc;
  if ((rc = map_hip(launch_frames_scan(a, f.s)))) return rc;
  if (!fused || frame_cap == 0) return RPCCRC_OK;
  if ((rc = rpc_frames_verify_device(d_stream, stream_bytes, d_frame_offsets, frame_cap, flags, d_verdict, d_crc,
                                     stream)))
    return rc;
  if (!reach) return RPCCRC_OK;
  return map_hip(launch_frames_reach(a.frame_conn, frame_cap, d_nframes, nconn, first_close, d_verdict, d_crc,
                                     d_conn_state, f.s));
}

extern "C" {

int rpc_frames_verify_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_frame_offsets,
                             uint64_t n, int flags, uint8_t *d_verdict, uint32_t *d_crc, void *stream) {
  if (!frames_flags_ok(flags)) return RPCCRC_EINVAL;
  if (n == 0) return RPCCRC_OK;
  if (!d_stream || !d_frame_offsets || !d_verdict || n >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  FramesParse fp; // (launched by ragged(), or fused into the route's plan)
  uint32_t *bcrc = nullptr;
  if ((rc = f.workspace([&](WsLayout &w) { verify_ws_layout(w, fp, bcrc, n); }))) return rc;
  if (d_crc) bcrc = d_crc;
  fp.stream = d_stream;
  fp.stream_bytes = stream_bytes;
  fp.frame_off = d_frame_offsets;
  fp.flags = flags;
  const FramesCmp cmp{fp.hdr_crc, fp.pre, d_verdict};
  RaggedCall q{d_stream, fp.body_off, fp.body_len, n, bcrc};
  q.small_bodies = true;
  q.route = (flags & RPC_FRAMES_LIFT_CAP) != 0;
  q.span_bytes = stream_bytes;
  q.cmp = &cmp;
  q.parse = &fp;
  if ((rc = ragged(*f.c, q, f.s))) return rc;
  if (q.compared) return RPCCRC_OK; // (route-all: the fold wrote the verdicts)
  return map_hip(launch_frames_compare(bcrc, fp.hdr_crc, fp.pre, n, d_verdict, f.s));
}

int rpc_frames_stamp_device(uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_frame_offsets,
                            const uint32_t *d_body_lens, uint64_t n, uint16_t version, uint16_t type, int flags,
                            uint8_t *d_verdict, void *stream) {
  if ((flags & ~(RPC_FRAMES_SERVER | RPC_FRAMES_CLIENT | RPC_FRAMES_LIFT_CAP)) != 0) return RPCCRC_EINVAL;
  if (n == 0) return RPCCRC_OK;
  if (!d_stream || !d_frame_offsets || !d_body_lens || n >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  FramesStamp st; // (the check launched by ragged(), or fused into the route's plan; the headers likewise)
  uint32_t *bcrc = nullptr;
  if ((rc = f.workspace([&](WsLayout &w) { stamp_ws_layout(w, st, bcrc, n); }))) return rc;
  if (d_verdict) st.pre = d_verdict;
  st.stream = d_stream;
  st.stream_bytes = stream_bytes;
  st.frame_off = d_frame_offsets;
  st.body_len = d_body_lens;
  st.flags = flags;
  st.version = version;
  st.type = type;
  RaggedCall q{d_stream, st.body_off, st.len_eff, n, bcrc};
  q.small_bodies = true;
  q.route = (flags & RPC_FRAMES_LIFT_CAP) != 0;
  q.span_bytes = stream_bytes;
  q.stamp = &st;
  if ((rc = ragged(*f.c, q, f.s))) return rc;
  if (q.stamped) return RPCCRC_OK; // (route-all: the fold wrote the headers)
  return map_hip(launch_frames_stamp(st, bcrc, n, f.s));
}

int rpc_frames_pack_device(const uint8_t *d_bodies, uint64_t bodies_bytes, const uint64_t *d_body_offsets,
                           const uint32_t *d_body_lens, uint64_t n, const uint16_t *d_types, uint16_t type,
                           const uint16_t *d_versions, uint16_t version, const uint64_t *d_conn_first, uint64_t nconn,
                           int flags, uint8_t *d_out, uint64_t out_cap, uint64_t *d_frame_offsets, uint8_t *d_verdict,
                           uint32_t *d_crc, uint64_t *d_conn_bytes_first, uint64_t *d_total, void *stream) {
  if ((flags & ~(RPC_FRAMES_SERVER | RPC_FRAMES_CLIENT | RPC_FRAMES_LIFT_CAP)) != 0) return RPCCRC_EINVAL;
  if (!frames_layout_args_ok(n, d_out, out_cap, d_conn_first, nconn, d_conn_bytes_first)) return RPCCRC_EINVAL;
  const bool no_data = !d_types && !pack_is_data(type); // heartbeats or nothing: no body is looked at
  if (n > 0 && !no_data && (!d_body_lens || !d_body_offsets)) return RPCCRC_EINVAL;
  if (bodies_bytes > 0 && !d_bodies) return RPCCRC_EINVAL;
  if (n == 0 && !d_total && !d_conn_bytes_first) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (n == 0) return frames_layout_empty(d_total, d_conn_bytes_first, nconn, f.s);
  const size_t tmp_words = scan_tmp_words(n);
  PackArgs a;
  a.n = n;
  if ((rc = f.workspace([&](WsLayout &w) { pack_ws_layout(w, a, tmp_words); }))) return rc;
  if (d_crc) a.crc = d_crc;
  a.bodies = d_bodies;
  a.bodies_bytes = bodies_bytes;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.types = d_types;
  a.versions = d_versions;
  a.type = type;
  a.version = version;
  a.conn_first = d_conn_first;
  a.nconn = nconn;
  a.flags = flags;
  a.out = d_out;
  a.out_cap = out_cap;
  a.frame_off = d_frame_offsets;
  a.verdict = d_verdict;
  a.conn_bytes_first = d_conn_bytes_first;
  a.total = d_total;
  if ((rc = map_hip(launch_frames_pack_layout(a, f.s)))) return rc;
  // The CRCs, over the source bodies: the ragged call stamp makes (the length
  // bound, the lifted-cap route), without its hooks.  A layout-only call that
  // does not ask for them skips the pass; a batch that cannot hold a data
  // frame has no body to read (every CRC is 0).
  if (no_data || !d_bodies) { // (no source buffer: every body the CRC pass would read is empty)
    RPCCRC_TRY(hipMemsetAsync(a.crc, 0, n * 4, f.s));
  } else if (d_out || d_crc) {
    RaggedCall q{d_bodies, a.src_off, a.src_len, n, a.crc};
    q.small_bodies = true;
    q.route = (flags & RPC_FRAMES_LIFT_CAP) != 0;
    q.span_bytes = bodies_bytes;
    if ((rc = ragged(*f.c, q, f.s))) return rc;
  }
  return map_hip(launch_frames_pack_write(a, f.s));
}

int rpc_frames_unpack_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_frame_offsets,
                             const uint8_t *d_verdict, uint64_t n, const uint64_t *d_conn_first, uint64_t nconn,
                             int flags, int nul, uint8_t *d_out, uint64_t out_cap, uint64_t *d_body_offsets,
                             uint32_t *d_body_lens, uint16_t *d_reply_types, uint16_t *d_versions,
                             uint8_t *d_verdict_out, uint64_t *d_conn_bytes_first, uint64_t *d_total, void *stream) {
  if (!frames_flags_ok(flags)) return RPCCRC_EINVAL;
  if (nul != 0 && nul != 1) return RPCCRC_EINVAL;
  if (!frames_layout_args_ok(n, d_out, out_cap, d_conn_first, nconn, d_conn_bytes_first)) return RPCCRC_EINVAL;
  if (n > 0 && (!d_frame_offsets || !d_verdict)) return RPCCRC_EINVAL;
  if (stream_bytes > 0 && !d_stream) return RPCCRC_EINVAL;
  if (n == 0 && !d_total && !d_conn_bytes_first) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (n == 0) return frames_layout_empty(d_total, d_conn_bytes_first, nconn, f.s);
  const size_t tmp_words = scan_tmp_words(n);
  UnpackArgs a;
  a.n = n;
  if ((rc = f.workspace([&](WsLayout &w) { unpack_ws_layout(w, a, tmp_words); }))) return rc;
  a.stream = d_stream;
  a.stream_bytes = stream_bytes;
  a.frame_off = d_frame_offsets;
  a.verdict_in = d_verdict;
  a.conn_first = d_conn_first;
  a.nconn = nconn;
  a.flags = flags;
  a.nul = nul;
  a.out = d_out;
  a.out_cap = out_cap;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.reply_types = d_reply_types;
  a.versions = d_versions;
  a.verdict_out = d_verdict_out;
  a.conn_bytes_first = d_conn_bytes_first;
  a.total = d_total;
  return map_hip(launch_frames_unpack(a, f.s));
}

int rpc_frames_carry_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_conn_off,
                            const uint64_t *d_conn_len, const uint64_t *d_conn_consumed, const uint8_t *d_conn_state,
                            uint64_t nconn, uint8_t *d_next, uint64_t next_bytes, const uint64_t *d_next_at,
                            uint64_t room, const uint64_t *d_new_len, uint64_t *d_next_off, uint64_t *d_next_len,
                            uint8_t *d_status, uint64_t *d_carried, void *stream) {
  if (nconn >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (nconn > 0 && (!d_conn_off || !d_conn_len || !d_conn_consumed || !d_next_at || !d_next_off || !d_next_len))
    return RPCCRC_EINVAL;
  if (stream_bytes > 0 && !d_stream) return RPCCRC_EINVAL;
  if (next_bytes > 0 && !d_next) return RPCCRC_EINVAL;
  if (nconn == 0 && !d_carried) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (d_carried) RPCCRC_TRY(hipMemsetAsync(d_carried, 0, 8, f.s)); // (the kernels add to it)
  if (nconn == 0) return RPCCRC_OK;
  CarryArgs a;
  a.stream = d_stream;
  a.stream_bytes = stream_bytes;
  a.conn_off = d_conn_off;
  a.conn_len = d_conn_len;
  a.conn_consumed = d_conn_consumed;
  a.conn_state = d_conn_state;
  a.nconn = nconn;
  a.next = d_next;
  a.next_bytes = next_bytes;
  a.next_at = d_next_at;
  a.room = room;
  a.new_len = d_new_len;
  a.next_off = d_next_off;
  a.next_len = d_next_len;
  a.status = d_status;
  a.carried = d_carried;
  // No tail can be longer than room: up to the threshold a group of lanes walks
  // a whole tail in one launch, and the long route's passes (plan, scan, chunks)
  // are not launched -- the idea of max_len in rpc_crc32_device_batch_bounded.
  if (room <= kCarryShortRoom) return map_hip(launch_frames_carry_short(a, f.s));
  const size_t tmp_words = scan_tmp_words(nconn);
  if ((rc = f.workspace([&](WsLayout &w) { carry_ws_layout(w, a, tmp_words); }))) return rc;
  return map_hip(launch_frames_carry_long(a, f.s));
}

int rpc_frames_route_device(const uint8_t *d_bodies, uint64_t bodies_bytes, const uint64_t *d_body_offsets,
                            const uint32_t *d_body_lens, const uint16_t *d_reply_types, uint64_t n,
                            const uint8_t *d_method_names, uint32_t method_bytes, const uint32_t *d_method_off,
                            uint32_t nmethods, uint8_t *d_kind, uint16_t *d_method, uint32_t *d_id,
                            uint32_t *d_params_off, uint32_t *d_params_len, uint32_t *d_order,
                            uint32_t *d_group_first, void *stream) {
  if (n >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (nmethods > RPC_ROUTE_MAX_METHODS || method_bytes > RPC_ROUTE_MAX_METHOD_BYTES) return RPCCRC_EINVAL;
  if (n > 0 && (!d_body_offsets || !d_body_lens)) return RPCCRC_EINVAL;
  if (bodies_bytes > 0 && !d_bodies) return RPCCRC_EINVAL;
  if (nmethods > 0 && !d_method_off) return RPCCRC_EINVAL;
  if (method_bytes > 0 && !d_method_names) return RPCCRC_EINVAL;
  if ((d_order == nullptr) != (d_group_first == nullptr)) return RPCCRC_EINVAL;
  if (n == 0 && !d_group_first) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (n == 0) { // no entries: every group is empty
    RPCCRC_TRY(hipMemsetAsync(d_group_first, 0, ((size_t)nmethods + 4) * 4, f.s));
    return RPCCRC_OK;
  }
  RouteArgs a;
  a.n = n;
  a.nmethods = nmethods;
  if (d_order) { // (without the order outputs none of the grouping passes is launched)
    const size_t tmp_words = scan_tmp_words(route_cells(a));
    if ((rc = f.workspace([&](WsLayout &w) { route_ws_layout(w, a, tmp_words); }))) return rc;
  }
  a.bodies = d_bodies;
  a.bodies_bytes = bodies_bytes;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.types = d_reply_types;
  a.names = d_method_names;
  a.method_bytes = method_bytes;
  a.method_off = d_method_off;
  a.kind = d_kind;
  a.method = d_method;
  a.id = d_id;
  a.params_off = d_params_off;
  a.params_len = d_params_len;
  a.order = d_order;
  a.group_first = d_group_first;
  return map_hip(launch_frames_route(a, f.s));
}

int rpc_frames_args_device(const uint8_t *d_bodies, uint64_t bodies_bytes, const uint64_t *d_body_offsets,
                           const uint32_t *d_body_lens, const uint8_t *d_kind, const uint16_t *d_method,
                           const uint32_t *d_params_off, const uint32_t *d_params_len, uint64_t n,
                           const uint32_t *d_param_first, uint32_t nmethods, const uint8_t *d_param_types,
                           const uint32_t *d_param_name_off, uint32_t nparams, const uint8_t *d_param_names,
                           uint32_t name_bytes, uint32_t width, uint64_t *d_slots, uint8_t *d_status,
                           int32_t *d_reply_status, void *stream) {
  if (n >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (nmethods > RPC_ROUTE_MAX_METHODS || nparams > RPC_ARGS_MAX_SCHEMA_PARAMS || name_bytes > RPC_ARGS_MAX_NAME_BYTES)
    return RPCCRC_EINVAL;
  if (width == 0 || width > RPC_ARGS_MAX_PARAMS) return RPCCRC_EINVAL;
  if (n > 0 && (!d_body_offsets || !d_body_lens || !d_kind || !d_method || !d_params_off || !d_params_len))
    return RPCCRC_EINVAL;
  if (bodies_bytes > 0 && !d_bodies) return RPCCRC_EINVAL;
  if (nmethods > 0 && !d_param_first) return RPCCRC_EINVAL;
  if (nparams > 0 && (!d_param_types || !d_param_name_off)) return RPCCRC_EINVAL;
  if (name_bytes > 0 && !d_param_names) return RPCCRC_EINVAL;
  if (n == 0) return RPCCRC_OK;
  FramesCall f;
  const int rc = f.open(stream);
  if (rc) return rc;
  ArgsArgs a; // (no workspace)
  a.bodies = d_bodies;
  a.bodies_bytes = bodies_bytes;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.kind = d_kind;
  a.method = d_method;
  a.params_off = d_params_off;
  a.params_len = d_params_len;
  a.n = n;
  a.param_first = d_param_first;
  a.nmethods = nmethods;
  a.param_types = d_param_types;
  a.param_name_off = d_param_name_off;
  a.nparams = nparams;
  a.param_names = d_param_names;
  a.name_bytes = name_bytes;
  a.width = width;
  a.slots = d_slots;
  a.status = d_status;
  a.reply_status = d_reply_status;
  return map_hip(launch_frames_args(a, f.s));
}

int rpc_frames_results_device(const uint8_t *d_bodies, uint64_t bodies_bytes, const uint64_t *d_body_offsets,
                              const uint32_t *d_body_lens, const uint8_t *d_kind, const uint32_t *d_slot,
                              const uint32_t *d_result_off, const uint32_t *d_result_len, const uint32_t *d_error_off,
                              const uint32_t *d_error_len, const uint32_t *d_slot_entry, uint64_t n,
                              const uint16_t *d_pending_method, uint32_t npending, const uint8_t *d_result_types,
                              uint32_t nmethods, uint8_t *d_status, uint64_t *d_value, uint8_t *d_error_status,
                              int32_t *d_error_code, uint64_t *d_error_message, uint8_t *d_slot_status,
                              uint64_t *d_slot_value, uint8_t *d_slot_error_status, int32_t *d_slot_error_code,
                              uint64_t *d_slot_str_base, uint32_t *d_ndefer, void *stream) {
  if (n >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (npending > RPC_RESOLVE_MAX_PENDING || nmethods > RPC_ROUTE_MAX_METHODS) return RPCCRC_EINVAL;
  if (n > 0 && (!d_body_offsets || !d_body_lens || !d_kind || !d_slot || !d_result_off || !d_result_len ||
                !d_error_off || !d_error_len))
    return RPCCRC_EINVAL;
  if (bodies_bytes > 0 && !d_bodies) return RPCCRC_EINVAL;
  if (npending > 0 && !d_pending_method) return RPCCRC_EINVAL;
  if (nmethods > 0 && !d_result_types) return RPCCRC_EINVAL;
  const bool per_slot = d_slot_status || d_slot_value || d_slot_error_status || d_slot_error_code || d_slot_str_base;
  if (per_slot && !d_slot_entry) return RPCCRC_EINVAL;
  if (n == 0 && !d_ndefer && !(per_slot && npending)) return RPCCRC_OK;
  FramesCall f;
  const int rc = f.open(stream);
  if (rc) return rc;
  ResultsArgs a; // (no workspace; with n == 0 every slot is open and nothing defers)
  a.bodies = d_bodies;
  a.bodies_bytes = bodies_bytes;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.kind = d_kind;
  a.slot = d_slot;
  a.result_off = d_result_off;
  a.result_len = d_result_len;
  a.error_off = d_error_off;
  a.error_len = d_error_len;
  a.slot_entry = d_slot_entry;
  a.n = n;
  a.pending_method = d_pending_method;
  a.npending = npending;
  a.result_types = d_result_types;
  a.nmethods = nmethods;
  a.status = d_status;
  a.value = d_value;
  a.error_status = d_error_status;
  a.error_code = d_error_code;
  a.error_message = d_error_message;
  a.slot_status = d_slot_status;
  a.slot_value = d_slot_value;
  a.slot_error_status = d_slot_error_status;
  a.slot_error_code = d_slot_error_code;
  a.slot_str_base = d_slot_str_base;
  a.ndefer = d_ndefer;
  return map_hip(launch_frames_results(a, f.s));
}

int rpc_frames_reply_device(const uint8_t *d_kind, const uint32_t *d_id, const int32_t *d_status,
                            const uint16_t *d_reply_types, uint64_t n, const uint8_t *d_values, uint64_t values_bytes,
                            const uint64_t *d_value_offsets, const uint32_t *d_value_lens, const uint64_t *d_conn_first,
                            uint64_t nconn, uint8_t *d_out, uint64_t out_cap, uint64_t *d_body_offsets,
                            uint32_t *d_body_lens, uint16_t *d_types_out, uint8_t *d_reply_status,
                            uint64_t *d_conn_bytes_first, uint64_t *d_total, void *stream) {
  if (!frames_layout_args_ok(n, d_out, out_cap, d_conn_first, nconn, d_conn_bytes_first)) return RPCCRC_EINVAL;
  if (n > 0 && (!d_id || !d_value_offsets || !d_value_lens)) return RPCCRC_EINVAL;
  if (values_bytes > 0 && !d_values) return RPCCRC_EINVAL;
  if (n == 0 && !d_total && !d_conn_bytes_first) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (n == 0) return frames_layout_empty(d_total, d_conn_bytes_first, nconn, f.s);
  const size_t tmp_words = scan_tmp_words(n);
  ReplyArgs a;
  a.n = n;
  if ((rc = f.workspace([&](WsLayout &w) { reply_ws_layout(w, a, tmp_words); }))) return rc;
  a.kind = d_kind;
  a.id = d_id;
  a.status = d_status;
  a.reply_types = d_reply_types;
  a.values = d_values;
  a.values_bytes = values_bytes;
  a.value_off = d_value_offsets;
  a.value_len = d_value_lens;
  a.conn_first = d_conn_first;
  a.nconn = nconn;
  a.out = d_out;
  a.out_cap = out_cap;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.types_out = d_types_out;
  a.reply_status = d_reply_status;
  a.conn_bytes_first = d_conn_bytes_first;
  a.total = d_total;
  return map_hip(launch_frames_reply(a, f.s));
}

int rpc_frames_values_device(int form, const uint8_t *d_mode, const int32_t *d_status, const uint16_t *d_method,
                             const uint64_t *d_slots, uint32_t width, uint64_t n, const uint8_t *d_result_types,
                             const uint32_t *d_param_first, uint32_t nmethods, const uint8_t *d_param_types,
                             const uint32_t *d_param_name_off, uint32_t nparams, const uint8_t *d_param_names,
                             uint32_t name_bytes, const uint8_t *d_strings, uint64_t strings_bytes,
                             const uint64_t *d_str_base, const uint8_t *d_texts, uint64_t texts_bytes,
                             const uint64_t *d_text_offsets, const uint32_t *d_text_lens, uint8_t *d_out,
                             uint64_t out_cap, uint64_t *d_value_offsets, uint32_t *d_value_lens,
                             uint8_t *d_values_status, int32_t *d_reply_status, uint32_t *d_ndefer, uint64_t *d_total,
                             void *stream) {
  if (form != RPC_VALUES_FORM_RESULT && form != RPC_VALUES_FORM_PARAMS) return RPCCRC_EINVAL;
  if (!frames_layout_args_ok(n, d_out, out_cap, nullptr, 0, nullptr)) return RPCCRC_EINVAL;
  if (width == 0 || width > RPC_ARGS_MAX_PARAMS) return RPCCRC_EINVAL;
  if (nmethods > RPC_ROUTE_MAX_METHODS) return RPCCRC_EINVAL;
  if (n > 0 && (!d_method || !d_slots)) return RPCCRC_EINVAL;
  const bool params = form == RPC_VALUES_FORM_PARAMS;
  if (params) {
    if (nparams > RPC_ARGS_MAX_SCHEMA_PARAMS || name_bytes > RPC_ARGS_MAX_NAME_BYTES) return RPCCRC_EINVAL;
    if (nmethods > 0 && !d_param_first) return RPCCRC_EINVAL;
    if (nparams > 0 && (!d_param_types || !d_param_name_off)) return RPCCRC_EINVAL;
    if (name_bytes > 0 && !d_param_names) return RPCCRC_EINVAL;
  } else if (nmethods > 0 && !d_result_types) {
    return RPCCRC_EINVAL;
  }
  if (strings_bytes > 0 && !d_strings) return RPCCRC_EINVAL;
  if (texts_bytes > 0 && !d_texts) return RPCCRC_EINVAL;
  const uint32_t unit = params ? width : 1u;
  if (n * unit >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (n == 0 && !d_total && !d_ndefer) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (n == 0) {
    if (d_ndefer) RPCCRC_TRY(hipMemsetAsync(d_ndefer, 0, sizeof(uint32_t), f.s));
    return frames_layout_empty(d_total, nullptr, 0, f.s);
  }
  ValuesArgs a;
  a.n = n;
  a.unit = unit;
  a.items = n * unit;
  const size_t tmp_words = scan_tmp_words(a.items);
  if ((rc = f.workspace([&](WsLayout &w) { values_ws_layout(w, a, tmp_words); }))) return rc;
  a.form = form;
  a.mode = d_mode;
  a.status = d_status;
  a.method = d_method;
  a.slots = d_slots;
  a.width = width;
  a.result_types = d_result_types;
  a.param_first = d_param_first;
  a.nmethods = nmethods;
  a.param_types = d_param_types;
  a.param_name_off = d_param_name_off;
  a.nparams = params ? nparams : 0;
  a.param_names = d_param_names;
  a.name_bytes = params ? name_bytes : 0;
  a.strings = d_strings;
  a.strings_bytes = strings_bytes;
  a.str_base = d_str_base;
  a.texts = d_texts;
  a.texts_bytes = texts_bytes;
  a.text_off = d_text_offsets;
  a.text_len = d_text_lens;
  a.out = d_out;
  a.out_cap = out_cap;
  a.value_off = d_value_offsets;
  a.value_len = d_value_lens;
  a.values_status = d_values_status;
  a.reply_status = d_reply_status;
  a.ndefer = d_ndefer;
  a.total = d_total;
  return map_hip(launch_frames_values(a, f.s));
}

int rpc_frames_request_device(const uint16_t *d_method, const uint32_t *d_id, const uint16_t *d_types, uint64_t n,
                              const uint8_t *d_method_names, uint32_t method_bytes, const uint32_t *d_method_off,
                              uint32_t nmethods, const uint8_t *d_params, uint64_t params_bytes,
                              const uint64_t *d_params_offsets, const uint32_t *d_params_lens,
                              const uint64_t *d_conn_first, uint64_t nconn, uint8_t *d_out, uint64_t out_cap,
                              uint64_t *d_body_offsets, uint32_t *d_body_lens, uint16_t *d_types_out,
                              uint8_t *d_request_status, uint64_t *d_conn_bytes_first, uint64_t *d_total, void *stream) {
  if (!frames_layout_args_ok(n, d_out, out_cap, d_conn_first, nconn, d_conn_bytes_first)) return RPCCRC_EINVAL;
  if (nmethods > RPC_ROUTE_MAX_METHODS || method_bytes > RPC_ROUTE_MAX_METHOD_BYTES) return RPCCRC_EINVAL;
  if (n > 0 && (!d_method || !d_id || !d_params_offsets || !d_params_lens)) return RPCCRC_EINVAL;
  if (params_bytes > 0 && !d_params) return RPCCRC_EINVAL;
  if (nmethods > 0 && !d_method_off) return RPCCRC_EINVAL;
  if (method_bytes > 0 && !d_method_names) return RPCCRC_EINVAL;
  if (n == 0 && !d_total && !d_conn_bytes_first) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  if (n == 0) return frames_layout_empty(d_total, d_conn_bytes_first, nconn, f.s);
  const size_t tmp_words = scan_tmp_words(n);
  RequestArgs a;
  a.n = n;
  if ((rc = f.workspace([&](WsLayout &w) { request_ws_layout(w, a, tmp_words); }))) return rc;
  a.method = d_method;
  a.id = d_id;
  a.types = d_types;
  a.names = d_method_names;
  a.method_bytes = method_bytes;
  a.method_off = d_method_off;
  a.nmethods = nmethods;
  a.params = d_params;
  a.params_bytes = params_bytes;
  a.params_off = d_params_offsets;
  a.params_len = d_params_lens;
  a.conn_first = d_conn_first;
  a.nconn = nconn;
  a.out = d_out;
  a.out_cap = out_cap;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.types_out = d_types_out;
  a.request_status = d_request_status;
  a.conn_bytes_first = d_conn_bytes_first;
  a.total = d_total;
  return map_hip(launch_frames_request(a, f.s));
}

int rpc_frames_resolve_device(const uint8_t *d_bodies, uint64_t bodies_bytes, const uint64_t *d_body_offsets,
                              const uint32_t *d_body_lens, const uint16_t *d_reply_types, uint64_t n,
                              const uint32_t *d_pending_ids, uint32_t npending, uint8_t *d_kind, uint32_t *d_id,
                              uint32_t *d_result_off, uint32_t *d_result_len, uint32_t *d_error_off,
                              uint32_t *d_error_len, uint32_t *d_slot, uint32_t *d_slot_entry, uint32_t *d_open,
                              uint32_t *d_nopen, void *stream) {
  if (n >= 0xFFFFFFFFull) return RPCCRC_EINVAL;
  if (npending > RPC_RESOLVE_MAX_PENDING) return RPCCRC_EINVAL;
  if (n > 0 && (!d_body_offsets || !d_body_lens)) return RPCCRC_EINVAL;
  if (bodies_bytes > 0 && !d_bodies) return RPCCRC_EINVAL;
  if (npending > 0 && !d_pending_ids) return RPCCRC_EINVAL;
  if ((d_open == nullptr) != (d_nopen == nullptr)) return RPCCRC_EINVAL;
  if (n == 0 && !d_slot_entry && !d_nopen) return RPCCRC_OK;
  FramesCall f;
  int rc = f.open(stream);
  if (rc) return rc;
  ResolveArgs a;
  a.n = n;
  a.npending = npending;
  a.open = d_open;
  a.slot = d_slot; // (the caller's, or workspace stands in)
  a.slot_entry = d_slot_entry;
  if (npending) { // (the decode-only call joins nothing)
    a.bits = resolve_table_bits(npending);
    const size_t tmp_words = d_open ? scan_tmp_words(npending) : 0;
    if ((rc = f.workspace([&](WsLayout &w) { resolve_ws_layout(w, a, tmp_words); }))) return rc;
  }
  a.bodies = d_bodies;
  a.bodies_bytes = bodies_bytes;
  a.body_off = d_body_offsets;
  a.body_len = d_body_lens;
  a.types = d_reply_types;
  a.pending = d_pending_ids;
  a.kind = d_kind;
  a.id = d_id;
  a.result_off = d_result_off;
  a.result_len = d_result_len;
  a.error_off = d_error_off;
  a.error_len = d_error_len;
  a.nopen = d_nopen;
  return map_hip(launch_frames_resolve(a, f.s));
}

int rpc_frames_scan_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_conn_off,
                           const uint64_t *d_conn_len, uint64_t nconn, int flags, uint64_t *d_frame_offsets,
                           uint32_t *d_frame_conn, uint64_t frame_cap, uint64_t *d_conn_first, uint64_t *d_conn_consumed,
                           uint8_t *d_conn_state, uint64_t *d_nframes, void *stream) {
  return frames_scan_common(d_stream, stream_bytes, d_conn_off, d_conn_len, nconn, flags, d_frame_offsets, d_frame_conn,
                            frame_cap, d_conn_first, d_conn_consumed, d_conn_state, d_nframes, nullptr, nullptr, false,
                            stream);
}

int rpc_frames_scan_verify_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_conn_off,
                                  const uint64_t *d_conn_len, uint64_t nconn, int flags, uint64_t *d_frame_offsets,
                                  uint32_t *d_frame_conn, uint64_t frame_cap, uint64_t *d_conn_first,
                                  uint64_t *d_conn_consumed, uint8_t *d_conn_state, uint64_t *d_nframes,
                                  uint8_t *d_verdict, uint32_t *d_crc, void *stream) {
  return frames_scan_common(d_stream, stream_bytes, d_conn_off, d_conn_len, nconn, flags, d_frame_offsets, d_frame_conn,
                            frame_cap, d_conn_first, d_conn_consumed, d_conn_state, d_nframes, d_verdict, d_crc, true,
                            stream);
}

int rpc_frames_set_scan_path(int path) {
  if (path != RPCCRC_SCAN_AUTO && path != RPCCRC_SCAN_SERIAL && path != RPCCRC_SCAN_TILED) return RPCCRC_EINVAL;
  g_scan_path.store(path);
  return RPCCRC_OK;
}

} // extern "C"
