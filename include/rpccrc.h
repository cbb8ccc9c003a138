/*
 * include/rpccrc.h -- C-ABI of librpccrc, the MI355X-native body-checksum
 * library that replaces KlinLike/RPC's crc.c.
 *
 * Drop-in part (exact reference signatures, C linkage, no new types):
 *   rpc_crc32         replaces reference crc.c:4-9   (declared crc.h:8)
 *   rpc_crc32_verify  replaces reference crc.c:11-14 (declared crc.h:11)
 * Callers that keep working unchanged: client/rpc_async.c:219,525 and
 * server/rpc_server_main.c:227,249 (and the unbuilt client/rpc_client.c:60,154).
 * Link librpccrc.so in place of crc.c (CMakeLists.txt:14,25).  The library
 * does NOT define zlib's global `crc32`, so it never interposes on -lz.
 *
 * Additive part (SURVEY.md 8b "New (additive) batched ABI"): many-buffer CRC
 * over host or device (HBM-resident) buffers, computed by hand-written HIP
 * kernels for gfx950.  Plain pointers and sizes only; the caller owns every
 * buffer.  `stream` arguments are hipStream_t passed as void* (NULL = the
 * default stream of the calling thread's current HIP device).
 *
 * Semantics are bit-exact to zlib crc32 as called by crc.c:6-7:
 *   CRC-32/ISO-HDLC, poly 0xEDB88320 (reflected), init/xorout 0xFFFFFFFF;
 *   rpc_crc32(NULL, n) == 0; rpc_crc32(p, 0) == 0;
 *   len is reduced modulo 2^32 (zlib's uInt len, crc.c:7 passes size_t).
 *
 * Error convention for the int-returning batched calls: 0 (or a non-negative
 * count where stated) on success, a negative errno-style code on failure
 * (RPCCRC_E*).  The two drop-in calls have no error channel in the reference
 * (crc.h:8,11); if no HIP device is usable they print a diagnostic to stderr and
 * abort() -- they never fall back to a CPU implementation.
 */
#pragma once

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RPCCRC_API __attribute__((visibility("default")))
#else
#define RPCCRC_API
#endif

#define RPCCRC_OK 0
#define RPCCRC_EINVAL (-22) /* bad argument (NULL buffer with n>0, bad size, ...) */
#define RPCCRC_ENODEV (-19) /* no usable HIP device */
#define RPCCRC_ENOMEM (-12) /* device or pinned allocation failed */
#define RPCCRC_EIO (-5)     /* HIP runtime / kernel launch error, or a kernel-reported
                               error (rpc_crc32_device_status) */
#define RPCCRC_EAGAIN (-11) /* receive ring: no free segment yet, poll first */

/* ---- drop-in (reference crc.h) ---------------------------------------- */

/* reference crc.h:8 / crc.c:4-9.  CRC of `len` bytes at `data`. */
RPCCRC_API uint32_t rpc_crc32(const void *data, size_t len);

/* reference crc.h:11 / crc.c:11-14.  expected_crc in host byte order. */
RPCCRC_API bool rpc_crc32_verify(const void *data, size_t len, uint32_t expected_crc);

/* ---- batched, host buffers -------------------------------------------- */

/* out_crc[i] = rpc_crc32(base + offsets[i], lengths[i]) for i < n.  Buffers are
 * host memory (pinned memory is used in place; pageable memory is staged).
 * flags must be 0.  Returns RPCCRC_OK or a negative code. */
RPCCRC_API int rpc_crc32_batch(const uint8_t *base, const uint64_t *offsets, const uint32_t *lengths, size_t n,
                    uint32_t *out_crc, int flags);

/* Batched rpc_crc32_verify: ok[i] = (crc == expected[i]).  Returns the number
 * of mismatching bodies (>= 0) or a negative code. */
RPCCRC_API int64_t rpc_crc32_verify_batch(const uint8_t *base, const uint64_t *offsets, const uint32_t *lengths,
                               const uint32_t *expected, size_t n, uint8_t *ok);

/* ---- batched, device (HBM-resident) buffers ---------------------------- */

/* Ragged batch: body i = d_base[d_offsets[i] .. + d_lengths[i]).  All pointers
 * are device pointers on the current device.  Asynchronous on `stream`.
 * Bodies of >= 256 KiB (>= 16 KiB in batches of <= 16384 bodies) are cut into
 * chunks on the device and folded with the GF(2) combine, so one long body does
 * not serialise the batch on one wave.  A batch of >= 65536 bodies that lie back
 * to back in batch order (each 64 B - 1 MiB; decided on the device) is CRC'd as
 * one stream of 4 KiB blocks and folded per body (dense span mode, DESIGN.md 4.9;
 * RPCCRC_DENSE=0 turns it off).  Same results either way. */
RPCCRC_API int rpc_crc32_device_batch(const uint8_t *d_base, const uint64_t *d_offsets, const uint32_t *d_lengths,
                           uint64_t n, uint32_t *d_out, void *stream);

/* rpc_crc32_device_batch with a length bound the caller knows (e.g. MAX_BODY_LEN,
 * rpc.h:17, or a workload's maximum): max_len >= every d_lengths[i], 0 = none.
 * With a bound below the big-body route threshold the route is never needed
 * and its passes are not launched.  The threshold depends on the batch size:
 * 16 KiB for n <= 16384 bodies, 256 KiB above (RPCCRC_BIG_MIN overrides both).
 * Results never depend on the hint: a body longer than a wrong bound is still
 * CRC'd exactly (by one wavefront, so slowly). */
RPCCRC_API int rpc_crc32_device_batch_bounded(const uint8_t *d_base, const uint64_t *d_offsets,
                                              const uint32_t *d_lengths, uint64_t n, uint32_t max_len,
                                              uint32_t *d_out, void *stream);

/* Equal-length batch: body i = d_base[i*stride .. + body_len). */
RPCCRC_API int rpc_crc32_device_uniform(const uint8_t *d_base, uint64_t n, uint32_t body_len, uint64_t stride,
                             uint32_t *d_out, void *stream);

/* Large bodies (any size): body i = d_base[h_offsets[i] .. + h_lengths[i]),
 * offsets/lengths in HOST memory.  Each body is split into chunk_bytes chunks
 * (multiple of 16; 0 = default: 16 KiB, or 8/4 KiB when that divides every
 * length of back-to-back bodies) processed in parallel and merged with the
 * GF(2) combine (zlib crc32_combine semantics).  Back-to-back bodies whose
 * lengths are chunk multiples run as one uniform batch.  Stream-ordered; the
 * call returns once the work is enqueued. */
RPCCRC_API int rpc_crc32_device_large(const uint8_t *d_base, const uint64_t *h_offsets, const uint64_t *h_lengths,
                           uint64_t n, uint32_t *d_out, uint64_t chunk_bytes, void *stream);

/* ---- gathered and running CRCs ------------------------- */

/* Gathered bodies.  Segment s = d_base[d_seg_offsets[s] .. + d_seg_lengths[s]).
 * Body i is the concatenation, in order, of segments d_seg_first[i] ..
 * d_seg_first[i+1]-1 (CSR: n+1 entries, non-decreasing, d_seg_first[0] == 0,
 * d_seg_first[n] == nseg; this is the caller's contract, like the offsets).
 * d_seed == NULL: d_out[i] = rpc_crc32 of the concatenation.
 * d_seed != NULL: d_out[i] = zlib crc32(d_seed[i], concatenation), i.e.
 *   rpc_crc32_combine(d_seed[i], rpc_crc32(concatenation), total length);
 *   a body with no segments, or only empty ones, yields d_seed[i] (0 without seeds).
 * max_seg_len: bound on the segment lengths, 0 = none (as _device_batch_bounded).
 * A segment may belong to several bodies, segments may overlap and lie in any
 * order in memory.  d_out may be the same pointer as d_seed.  Asynchronous.
 * The segments are CRC'd as one rpc_crc32_device_batch (all its routes), then
 * folded per body on the device with the GF(2) combine: a body's total length is
 * 64-bit (it may exceed 4 GiB), and a body of many segments is folded by a whole
 * workgroup.  n == 0: RPCCRC_OK, nothing touched.  nseg == 0 (d_base,
 * d_seg_offsets, d_seg_lengths may then be NULL): every body is empty. */
RPCCRC_API int rpc_crc32_device_gather(const uint8_t *d_base, const uint64_t *d_seg_offsets,
                                       const uint32_t *d_seg_lengths, uint64_t nseg, uint32_t max_seg_len,
                                       const uint64_t *d_seg_first, uint64_t n, const uint32_t *d_seed,
                                       uint32_t *d_out, void *stream);

/* The same over host memory; synchronous, staged as rpc_crc32_batch stages.  flags must be 0. */
RPCCRC_API int rpc_crc32_batch_gather(const uint8_t *base, const uint64_t *seg_offsets, const uint32_t *seg_lengths,
                                      size_t nseg, const uint64_t *seg_first, size_t n, const uint32_t *seed,
                                      uint32_t *out_crc, int flags);

/* zlib's running form for one buffer: crc32(crc, data, len).  data == NULL -> 0
 * (zlib returns 0 for Z_NULL whatever crc is); len reduced mod 2^32 as rpc_crc32.
 * rpc_crc32 of the buffer (on the GPU, as the drop-in call) combined with crc. */
RPCCRC_API uint32_t rpc_crc32_update(uint32_t crc, const void *data, size_t len);

/* ---- frames (rpc.h:3-8 wire format) ------------------------------------ */

/* Reference wire constants (rpc.h:11-18). */
#define RPC_HEADER_LEN_BYTES 12u /* RPC_HEADER_LEN, rpc.h:15 */
#define RPC_MAX_BODY_LEN 1024u   /* MAX_BODY_LEN, rpc.h:17 */
#define RPC_FRAME_TYPE_DATA 0u   /* RPC_TYPE_DATA, rpc.h:11 */
#define RPC_FRAME_TYPE_PING 1u   /* RPC_TYPE_PING, rpc.h:12 */
#define RPC_FRAME_TYPE_PONG 2u   /* RPC_TYPE_PONG, rpc.h:13 */

/* Per-frame verdict (one byte per frame), in the order the reference decides:
 * type first, then the body-length cap, then the CRC. */
#define RPC_FRAME_BAD_CRC 0u   /* data frame, body CRC != header crc32: the server
                                  closes the connection (rpc_server_main.c:227-233),
                                  the client reports RPC_CRC_ERR (rpc_async.c:219-222) */
#define RPC_FRAME_OK 1u        /* data frame, body CRC == header crc32 */
#define RPC_FRAME_CONTROL 2u   /* heartbeat answered from the header alone, whatever
                                  its crc32 / body_len fields hold: PING at the server
                                  (rpc_server_main.c:172-187), PONG at the client
                                  (rpc_async.c:303-309); no body is read */
#define RPC_FRAME_TOO_LARGE 3u /* body_len > MAX_BODY_LEN with the cap in force: the
                                  peer is dropped before its body is read
                                  (rpc_server_main.c:189-195, rpc_async.c:312) */
#define RPC_FRAME_MALFORMED 4u /* header or body extends past the stream: not read */
#define RPC_FRAME_RECV_ERR 5u  /* client role only: a non-PONG frame with body_len 0.
                                  The reference client's BODY state calls
                                  recv(fd, buf, 0) on its non-blocking socket; once
                                  any further byte (or the peer's FIN) is pending that
                                  returns 0, taken for a closed peer
                                  (rpc_async.c:330-349): the connection is dropped and
                                  the call ends with RPC_RECV_ERR (rpc_types.h:26,
                                  rpc_async.c:377-386).  (On an idle socket recv
                                  returns EAGAIN and the client waits until more
                                  arrives, or the call times out.)  The empty body is
                                  never verified (rpc_async.c:219 is not reached).
                                  The server reads an empty body and verifies it
                                  (rpc_server_main.c:198-227), so a server-role frame
                                  with body_len 0 is OK / BAD_CRC by its crc32 field. */

/* Frame-call flags.  The role picks which heartbeat type is a control frame
 * (the other one is an ordinary data frame, as in the reference). */
#define RPC_FRAMES_SERVER 0x1   /* PING is control (rpc_server_main.c:172) */
#define RPC_FRAMES_CLIENT 0x2   /* PONG is control (rpc_async.c:303) */
#define RPC_FRAMES_LIFT_CAP 0x4 /* no MAX_BODY_LEN cap; bodies of any
                                   size, the large ones chunked + GF(2)-combined */

/* Verify n frames of a device stream of stream_bytes bytes.  Frame i starts at
 * d_stream + d_frame_offsets[i] with a 12-byte big-endian rpc_header_t {u16
 * version, u16 type, u32 body_len, u32 crc32} (rpc.h:3-8, parsed as
 * rpc_server_main.c:165-169) followed by body_len body bytes.  Writes
 * d_verdict[i] (RPC_FRAME_*) and, if d_crc is not NULL, the body CRC (0 for
 * frames whose body is not read).  Nothing outside [d_stream, d_stream +
 * stream_bytes) is read.  flags: exactly one role bit, optionally LIFT_CAP. */
RPCCRC_API int rpc_frames_verify_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_frame_offsets,
                             uint64_t n, int flags, uint8_t *d_verdict, uint32_t *d_crc, void *stream);

/* Stamp headers: for each frame i whose body d_stream[d_frame_offsets[i] + 12
 * .. + d_body_lens[i]) lies inside the stream, write its 12-byte header
 * (version, type, body_len, crc32 big-endian, as rpc_async.c:521-530).
 * Without RPC_FRAMES_LIFT_CAP a body over MAX_BODY_LEN is not stamped (the
 * reference client refuses to send it, rpc_async.c:499-501).  d_verdict
 * (optional): RPC_FRAME_OK (stamped), _TOO_LARGE or _MALFORMED.  Role bits are
 * ignored. */
RPCCRC_API int rpc_frames_stamp_device(uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_frame_offsets,
                            const uint32_t *d_body_lens, uint64_t n, uint16_t version, uint16_t type, int flags,
                            uint8_t *d_verdict, void *stream);

/* ---- frame pack: build wire streams from bodies ---------------------------
 * The mirror image of the scan.  Entry i is a type, a version and a body
 * d_bodies[d_body_offsets[i], + d_body_lens[i]); the call computes the layout,
 * copies the bodies into place, stamps the headers and leaves one contiguous
 * byte run per connection to send().  For entry i, in this order:
 *   1. t = d_types ? d_types[i] : type.  t == RPC_FRAME_TYPE_NONE: 0 bytes,
 *      RPC_FRAME_SKIPPED; its offset and length are not looked at (the verdicts
 *      of a scan can feed a reply batch with no compaction step).
 *   2. t is PING or PONG: a heartbeat as the reference sends one
 *      (conn_pool.c:248-257, rpc_server_main.c:172-187): 12 bytes, body_len 0,
 *      crc32 0, RPC_FRAME_CONTROL; offset and length are not looked at.
 *   3. Any other type is a data frame.  A body that does not lie inside
 *      [0, bodies_bytes): RPC_FRAME_MALFORMED, 0 bytes.
 *   4. len > RPC_MAX_BODY_LEN without RPC_FRAMES_LIFT_CAP: RPC_FRAME_TOO_LARGE,
 *      0 bytes (rpc_async.c:499-501: the client does not send it).
 *   5. Otherwise 12 + len bytes, RPC_FRAME_OK.
 * Layout: d_frame_offsets[i] is the exclusive 64-bit sum of the sizes of
 * entries 0 .. i-1, *d_total the sum of all; with a CSR d_conn_first[nconn + 1]
 * over the entries (as the scan returns it) d_conn_bytes_first[c] is the frame
 * offset of entry d_conn_first[c] and d_conn_bytes_first[nconn] is *d_total:
 * connection c sends d_out[d_conn_bytes_first[c], d_conn_bytes_first[c + 1]).
 * The layout never depends on out_cap.
 * Capacity: an entry of non-zero size that does not end inside out_cap is not
 * written, not even in part, and its verdict becomes RPC_FRAME_MALFORMED.
 * Nothing at or beyond d_out + out_cap is written, and bytes of d_out that
 * belong to no written frame are left untouched.  d_out == NULL with out_cap
 * == 0 is the layout-only call: everything but d_out is written, so the caller
 * can size the buffer from *d_total and call again.
 * A written frame is its 12-byte big-endian header (rpc_async.c:521-530) and
 * the body bytes.  d_crc[i]: the CRC stamped (bit-exact rpc_crc32), 0 for
 * everything that is not a data frame of rule 5.  d_out must not overlap
 * d_bodies.  Nothing outside [d_bodies, d_bodies + bodies_bytes) is read.
 * All pointers are device pointers; d_frame_offsets, d_verdict, d_crc [n],
 * d_conn_bytes_first [nconn + 1] and d_total [1] are optional; the call is
 * asynchronous on `stream`.  flags: RPC_FRAMES_LIFT_CAP; role bits are accepted
 * and ignored, as in stamp.
 * RPCCRC_EINVAL, before any device is touched: unknown flag bits; n >=
 * 0xFFFFFFFF; n > 0 with d_body_lens or d_body_offsets NULL (unless d_types is
 * NULL and `type` is a heartbeat or NONE); bodies_bytes > 0 with d_bodies NULL;
 * out_cap > 0 with d_out NULL; d_conn_bytes_first without d_conn_first; nconn >
 * 0 with d_conn_first NULL.  n == 0 with neither d_total nor
 * d_conn_bytes_first is RPCCRC_OK with no device; with them, *d_total and the
 * nconn + 1 connection words are written as 0. */
#define RPC_FRAME_SKIPPED 7u        /* pack only: the caller asked for no frame here */
#define RPC_FRAME_TYPE_NONE 0xFFFFu /* pack only: type value meaning "emit nothing for this entry" */
RPCCRC_API int rpc_frames_pack_device(const uint8_t *d_bodies, uint64_t bodies_bytes, const uint64_t *d_body_offsets,
                           const uint32_t *d_body_lens, uint64_t n, const uint16_t *d_types, uint16_t type,
                           const uint16_t *d_versions, uint16_t version, const uint64_t *d_conn_first, uint64_t nconn,
                           int flags, uint8_t *d_out, uint64_t out_cap, uint64_t *d_frame_offsets, uint8_t *d_verdict,
                           uint32_t *d_crc, uint64_t *d_conn_bytes_first, uint64_t *d_total, void *stream);

/* ---- frame scan: find the frames in raw connection bytes -----------------
 * A connection is a byte run [d_conn_off[c], + d_conn_len[c]) of the device
 * stream: what recv() has delivered so far, typically tens of pipelined frames
 * and a partial one at the end.  Its frames are found by walking the headers
 * from its first byte, with the reference's stop rules:
 *   - fewer than 12 bytes left, or a body that is not complete yet: stop; the
 *     partial frame is not emitted and not consumed (it is not here yet);
 *   - a control frame (PING at a server, PONG at a client): 12 bytes, go on;
 *   - body_len over MAX_BODY_LEN without LIFT_CAP (rpc_server_main.c:189-195),
 *     or body_len 0 at a client (rpc_async.c:330-349): emitted (its verdict is
 *     TOO_LARGE / RECV_ERR), 12 bytes consumed, the connection is CLOSED and
 *     nothing behind it is looked at;
 *   - otherwise a data frame of 12 + body_len bytes.
 * Outputs (all device pointers; the call is asynchronous on `stream`):
 *   d_frame_offsets[frame_cap]  absolute offsets in d_stream, grouped by
 *       connection in connection order, stream order within a connection.
 *       Only the first frame_cap frames are written, never anything at index
 *       >= frame_cap; entries [*d_nframes, frame_cap) are set to stream_bytes,
 *       which rpc_frames_verify_device calls MALFORMED with no body read, so
 *       the array can go to verify with n = frame_cap and no host round trip.
 *       NULL with frame_cap 0: count only (everything else is still written).
 *   d_frame_conn[frame_cap]     the frame's connection (optional; 0xFFFFFFFF
 *       in the padding entries)
 *   d_conn_first[nconn + 1]     CSR over the frames found (also past frame_cap)
 *   d_conn_consumed[nconn]      bytes of the connection the caller may drop;
 *       the rest is the carry-over for the next recv()
 *   d_conn_state[nconn]         RPC_CONN_OPEN / RPC_CONN_CLOSED
 *   d_nframes[1]                frames found, also when > frame_cap
 * A connection that does not lie inside the stream is CLOSED with no frames
 * and nothing consumed.  nconn == 0 is RPCCRC_OK with *d_nframes = 0.  flags as
 * rpc_frames_verify_device.  Every emitted frame is one rpc_frames_verify_device
 * does not call MALFORMED. */
#define RPC_FRAME_NOT_REACHED 6u /* fused call only: a frame behind one that closed its connection */
#define RPC_CONN_OPEN 0u
#define RPC_CONN_CLOSED 1u
RPCCRC_API int rpc_frames_scan_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_conn_off,
                           const uint64_t *d_conn_len, uint64_t nconn, int flags, uint64_t *d_frame_offsets,
                           uint32_t *d_frame_conn, uint64_t frame_cap, uint64_t *d_conn_first, uint64_t *d_conn_consumed,
                           uint8_t *d_conn_state, uint64_t *d_nframes, void *stream);

/* Scan, then rpc_frames_verify_device on the frame_cap entries (d_verdict and
 * d_crc hold frame_cap entries; d_crc may be NULL; padding entries read
 * MALFORMED with crc 0), then within each connection every frame behind the
 * first one whose verdict is BAD_CRC, TOO_LARGE or RECV_ERR becomes
 * RPC_FRAME_NOT_REACHED with crc 0 -- the reference has closed the connection
 * there (rpc_server_main.c:227-233) -- and a connection with a BAD_CRC becomes
 * RPC_CONN_CLOSED.  d_conn_consumed keeps the scan's value. */
RPCCRC_API int rpc_frames_scan_verify_device(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_conn_off,
                           const uint64_t *d_conn_len, uint64_t nconn, int flags, uint64_t *d_frame_offsets,
                           uint32_t *d_frame_conn, uint64_t frame_cap, uint64_t *d_conn_first, uint64_t *d_conn_consumed,
                           uint8_t *d_conn_state, uint64_t *d_nframes, uint8_t *d_verdict, uint32_t *d_crc,
                           void *stream);

/* Route of the scan (results identical):
 *   RPCCRC_SCAN_AUTO    connections longer than 96 KiB tiled, the rest serial
 *   RPCCRC_SCAN_SERIAL  one lane per connection walks its headers
 *   RPCCRC_SCAN_TILED   every connection of more than one 32 KiB tile is cut
 *                       into tiles whose entry -> exit maps are composed
 * Calls with RPC_FRAMES_LIFT_CAP always walk serially (the tiled route rests on
 * frames of at most 12 + MAX_BODY_LEN bytes). */
#define RPCCRC_SCAN_AUTO 0
#define RPCCRC_SCAN_SERIAL 1
#define RPCCRC_SCAN_TILED 2
RPCCRC_API int rpc_frames_set_scan_path(int path);

/* ---- frame unpack: verified bodies as C strings, and the reply plan -------
 * What sits between the fused scan + verify and the dispatcher.  Inputs are
 * what rpc_frames_scan_verify_device (or scan, then verify) left: the raw
 * stream, d_frame_offsets and d_verdict over n entries (n may be the padded
 * frame_cap), the CSR d_conn_first.  The bodies the reference would dispatch
 * are copied out back to back, each followed by one 0 byte when nul is 1 -- the
 * reference copies a body into its own buffer, sets body[body_len] = '\0' and
 * hands the char * to its dispatcher (rpc_server_main.c:198-238,
 * rpc_async.c:357,454-457) -- and the per-entry arrays are the frame pack's
 * inputs for the replies.  For entry i with v = d_verdict[i], in this order:
 *   1. v is neither RPC_FRAME_OK nor RPC_FRAME_CONTROL: nothing is delivered:
 *      size 0, reply type RPC_FRAME_TYPE_NONE, version 0, length 0, verdict out
 *      v.  The offset is not looked at (padding entries, NOT_REACHED, BAD_CRC
 *      and the rest end here).
 *   2. The 12-byte header does not lie inside [0, stream_bytes): the verdict is
 *      contradicted: size 0, NONE, version 0, length 0, verdict out
 *      RPC_FRAME_MALFORMED.
 *   3. version, type and body_len are read big-endian (rpc_server_main.c:
 *      165-169).  ctl is PING with RPC_FRAMES_SERVER, PONG with _CLIENT.  Every
 *      contradiction below gives the result of rule 2.
 *   4. v == CONTROL: type != ctl is a contradiction; otherwise size 0, length
 *      0, the header's version, verdict out CONTROL, reply type PONG at a server
 *      (rpc_server_main.c:172-187 answers a PING with a PONG of its version) and
 *      NONE at a client, which consumes a PONG (rpc_async.c:303-309).
 *   5. v == OK: type == ctl, body_len over RPC_MAX_BODY_LEN without
 *      RPC_FRAMES_LIFT_CAP, body_len 0 at a client, or a body not inside the
 *      stream is a contradiction; otherwise the entry is delivered: size
 *      body_len + nul, length body_len, the header's version, reply type
 *      RPC_FRAME_TYPE_DATA, verdict out OK.
 * No CRC is computed: OK is trusted as far as rules 2-5 allow.
 * Layout: d_body_offsets[i] is the exclusive 64-bit sum of the sizes of entries
 * 0 .. i-1, *d_total the sum of all; d_conn_bytes_first[c] is the body offset
 * of entry d_conn_first[c], d_conn_bytes_first[nconn] is *d_total (a CSR that
 * runs past n reads as the end).  The layout never depends on out_cap.
 * Output: a delivered entry's body bytes go to d_out + d_body_offsets[i]; with
 * nul one 0 byte follows them, and that address is the string the reference's
 * rpc_server_dispatch takes.
 * Capacity (the pack's rule): an entry of non-zero size that does not end
 * inside out_cap is not written, not even in part; its verdict out becomes
 * RPC_FRAME_MALFORMED and its reply type NONE; its offset, length and version
 * keep the layout's values.  Nothing at or beyond d_out + out_cap is written,
 * and no byte of d_out outside a written entry.  d_out == NULL with out_cap ==
 * 0 is the layout-only call.
 * Nothing outside [d_stream, d_stream + stream_bytes) is read.  d_out must not
 * overlap the stream; d_verdict_out may be d_verdict.
 * The outputs are rpc_frames_pack_device's inputs unchanged: bodies d_out,
 * d_body_offsets, d_body_lens, types d_reply_types, versions d_versions, the
 * same d_conn_first (the pack never looks at the offset or length of a NONE or
 * PONG entry).
 * All pointers are device pointers; every output from d_body_offsets on is
 * optional; the call is asynchronous on `stream`.  flags: exactly one role bit,
 * optionally RPC_FRAMES_LIFT_CAP.  nul: 0 or 1.
 * RPCCRC_EINVAL, before any device is touched: unknown flag bits or not exactly
 * one role bit; nul not 0 or 1; n >= 0xFFFFFFFF; n > 0 with d_frame_offsets or
 * d_verdict NULL; stream_bytes > 0 with d_stream NULL; out_cap > 0 with d_out
 * NULL; d_conn_bytes_first without d_conn_first; nconn > 0 with d_conn_first
 * NULL.  n == 0 with neither d_total nor d_conn_bytes_first is RPCCRC_OK with
 * no device; with them, *d_total and the nconn + 1 connection words are written
 * as 0. */
RPCCRC_API int rpc_frames_unpack_device(const uint8_t *d_stream, uint64_t stream_bytes,
                           const uint64_t *d_frame_offsets, const uint8_t *d_verdict, uint64_t n,
                           const uint64_t *d_conn_first, uint64_t nconn, int flags, int nul,
                           uint8_t *d_out, uint64_t out_cap,
                           uint64_t *d_body_offsets, uint32_t *d_body_lens, uint16_t *d_reply_types,
                           uint16_t *d_versions, uint8_t *d_verdict_out,
                           uint64_t *d_conn_bytes_first, uint64_t *d_total, void *stream);

/* ---- frame carry: partial frames join the next read ------------------------
 * What happens between two rounds of scan -> unpack -> handlers -> pack.  The
 * scan left d_conn_consumed[c]: the rest of connection c, its *tail*, is the
 * start of a frame whose other bytes the next recv() brings.  The caller lands
 * the next round's new bytes in another buffer, d_next, with `room` bytes of
 * headroom in front of each connection's bytes: d_next_at[c] is the offset in
 * d_next at which connection c's new bytes begin (d_new_len[c] of them; they are
 * there already or a copy on another stream is still landing them: the call
 * never looks at them).  The call copies each open connection's tail so that it
 * ends exactly where the new bytes begin, and writes the next round's
 * connections, d_next_off / d_next_len, for the scan over d_next.  Only the
 * tails move: with the cap in force a tail is at most 12 + RPC_MAX_BODY_LEN - 1
 * bytes (the scan stops only inside a header or a body), which
 * RPC_FRAMES_CARRY_ROOM covers.
 * For connection c, in this order:
 *   1. d_conn_state is given and d_conn_state[c] != RPC_CONN_OPEN:
 *      RPC_CARRY_CLOSED, next_off = next_len = 0.  Its offset, length and
 *      consumed are not looked at, and its new bytes are not attached: the
 *      reference reads nothing more from a peer it has dropped
 *      (rpc_server_main.c:189-195, 227-233).  (The scan of the empty connection
 *      reads OPEN again; from then on the slot is the host's to reuse.)
 *   2. The connection does not lie inside [0, stream_bytes), or consumed > len
 *      (computed without 64-bit wrap): RPC_CARRY_INVALID, 0 / 0, nothing read.
 *   3. With tail = len - consumed, at = d_next_at[c], nl = d_new_len ?
 *      d_new_len[c] : 0: tail > room, tail > at, at > next_bytes or nl >
 *      next_bytes - at: RPC_CARRY_NO_ROOM, 0 / 0, nothing written.
 *   4. Otherwise stream bytes [off + consumed, off + len) are copied to d_next
 *      [at - tail, at); next_off = at - tail, next_len = tail + nl,
 *      RPC_CARRY_OK.
 * *d_carried is the sum of the tails written.
 * Nothing outside [d_stream, d_stream + stream_bytes) is read, not even by an
 * aligned load window.  No byte of d_next outside a written tail is written,
 * and none is read and written back: the byte at `at` may be in flight from a
 * copy on another stream.  The regions [at - room, at) of different connections
 * must be disjoint (the caller's contract, not checked), and d_next must not
 * overlap the stream: the caller double-buffers.  d_next_off may be d_conn_off
 * and d_next_len may be d_conn_len: a connection's words are read before any of
 * them is overwritten.
 * room is also the bound that picks the route: up to 4096 one launch does
 * everything; above it (RPC_FRAMES_LIFT_CAP servers, whose partial body can be
 * megabytes) tails are copied in 16 KiB chunks dealt out over the whole device.
 * All pointers are device pointers; d_conn_state, d_new_len, d_status and
 * d_carried are optional; the call is asynchronous on `stream`.
 * RPCCRC_EINVAL, before any device is touched: nconn >= 0xFFFFFFFF; nconn > 0
 * with d_conn_off, d_conn_len, d_conn_consumed, d_next_at, d_next_off or
 * d_next_len NULL; stream_bytes > 0 with d_stream NULL; next_bytes > 0 with
 * d_next NULL.  nconn == 0 without d_carried is RPCCRC_OK with no device; with
 * it, *d_carried is written as 0. */
#define RPC_FRAMES_CARRY_ROOM 1040u /* >= 12 + RPC_MAX_BODY_LEN - 1, rounded up to 16: enough for any tail with the cap in force */
#define RPC_CARRY_OK 0u       /* tail (possibly empty) carried, new bytes attached */
#define RPC_CARRY_CLOSED 1u   /* the connection was closed: nothing carried, nothing attached */
#define RPC_CARRY_INVALID 2u  /* connection not inside the stream, or consumed > len: nothing read */
#define RPC_CARRY_NO_ROOM 3u  /* tail > room, or the next connection would not lie inside d_next: nothing written */
RPCCRC_API int rpc_frames_carry_device(const uint8_t *d_stream, uint64_t stream_bytes,
                           const uint64_t *d_conn_off, const uint64_t *d_conn_len, const uint64_t *d_conn_consumed,
                           const uint8_t *d_conn_state, uint64_t nconn,
                           uint8_t *d_next, uint64_t next_bytes, const uint64_t *d_next_at, uint64_t room,
                           const uint64_t *d_new_len,
                           uint64_t *d_next_off, uint64_t *d_next_len, uint8_t *d_status,
                           uint64_t *d_carried, void *stream);

/* ---- frame route: JSON-RPC envelope, method index, groups --------------------
 * What sits between the unpack and the handlers.  The reference's dispatcher
 * parses each whole body to learn its `method` and `id` and then runs a strcmp
 * chain (rpc_server_skeleton.c:118-160).  This call gives, for every delivered
 * body, the request's id, the index of its method in the server's table and
 * where `params` lies, and groups the entries by method, so that a handler runs
 * once over an array of its requests and the host parses only the `params`
 * span of requests it is going to answer.  It is not a JSON codec: no tree is
 * built and no value converted but a digits-only id.  It accepts a strict
 * subset of what the reference's lenient parser accepts; inside the subset its
 * answer is the reference's, and everything outside it -- every body the
 * reference calls a parse error among them -- reads RPC_ROUTE_DEFER and goes
 * through the full parser on the host as before.
 * d_bodies, d_body_offsets, d_body_lens and d_reply_types are the unpack's
 * outputs unchanged (nul 0 or 1: the NUL is never looked at); d_reply_types ==
 * NULL means every entry is DATA.  The method table is the names back to back
 * in d_method_names; name m is bytes [d_method_off[m], d_method_off[m + 1]).
 * For entry i, in this order:
 *   1. d_reply_types is given and d_reply_types[i] != RPC_FRAME_TYPE_DATA:
 *      RPC_ROUTE_NONE.  The offset and the length are not looked at.
 *   2. The body does not lie inside [0, bodies_bytes) (computed without 64-bit
 *      wrap): RPC_ROUTE_RANGE.  Nothing is read.
 *   3. RPC_ROUTE_DEFER if len == 0 or len > RPC_ROUTE_MAX_BODY, if the body is
 *      not strict, if it nests deeper than RPC_ROUTE_MAX_DEPTH (the root object
 *      is depth 1), or if it has more than RPC_ROUTE_MAX_TOKENS tokens (each of
 *      { } [ ] , : outside strings, each string, each number or literal).
 *      Strict: the whole body is one JSON object per RFC 8259 with only space,
 *      \t, \n, \r as whitespace before it, inside it and after it; numbers
 *      follow the RFC grammar exactly (no leading zero, digits on both sides of
 *      a point, digits in an exponent); literals are exactly true, false, null;
 *      string bytes are >= 0x20 and not '"'; a backslash is followed by one of
 *      " \ / b f n r t -- any \u defers (the reference rejects some surrogates
 *      and accepts \u0000); bytes >= 0x80 pass unchecked, as the reference
 *      copies them.  A 0 byte anywhere defers.
 *   4. RPC_ROUTE_DEFER if a depth-1 key contains a backslash: keys are compared
 *      as raw bytes.
 *   5. The value of the FIRST depth-1 key `id`: absent or not a number: id 0.  A
 *      number written as digits only with value <= 4294967295: that value.
 *      Digits only and larger: RPC_ROUTE_INVALID with id 0
 *      (rpc_server_skeleton.c:131-135).  Any other number form (sign, fraction,
 *      exponent): RPC_ROUTE_DEFER.
 *   6. The first depth-1 key `method`: absent, or its value is not a string:
 *      RPC_ROUTE_INVALID with the id of rule 5.  The string contains a
 *      backslash: RPC_ROUTE_DEFER.
 *   7. The method's raw bytes are compared with the table in table order: the
 *      first equal name gives RPC_ROUTE_CALL and its index, none gives
 *      RPC_ROUTE_NOT_FOUND.  A table word that is not monotone (off[m] >
 *      off[m + 1]) or that leaves method_bytes makes that name match nothing.
 *      The empty name is legal and matches "method":"".
 *   8. For RPC_ROUTE_CALL, d_params_off / d_params_len are the span, relative
 *      to the body's first byte, of the first depth-1 `params` value, from its
 *      first byte to one past its last; 0 / 0 when absent (the reference
 *      substitutes {}).
 *
 *   kind                  d_method             d_id                 d_params_off / _len
 *   NONE, RANGE, DEFER    RPC_ROUTE_NO_METHOD  0                    0 / 0
 *   INVALID, NOT_FOUND    RPC_ROUTE_NO_METHOD  rule 5 (0 when rule  0 / 0
 *                                              5 reads INVALID)
 *   CALL                  table index          rule 5               rule 8
 *
 * Every body in the strict subset parses under the reference's parser to the
 * tree an RFC parser builds (its nesting limit is 1000), so inside the subset
 * rules 5-8 are rpc_server_skeleton.c:129-160 and 162-260.
 * Groups: when d_order and d_group_first are given (both or neither),
 * d_group_first is a CSR of nmethods + 4 words over nmethods + 3 groups: CALL
 * by method index, then NOT_FOUND, INVALID, DEFER.  d_order lists the entry
 * indices group by group, ascending inside each group (a stable counting sort);
 * NONE and RANGE entries are in no group, and only d_order[0 ..
 * d_group_first[nmethods + 3]) is written (so n words always suffice).
 * Nothing outside [d_bodies, d_bodies + bodies_bytes) and the two table arrays
 * is read, not even by an aligned load window.  All pointers are device
 * pointers; every output is optional; the call is asynchronous on `stream`.
 * RPCCRC_EINVAL, before any device is touched: n >= 0xFFFFFFFF; nmethods >
 * RPC_ROUTE_MAX_METHODS; method_bytes > RPC_ROUTE_MAX_METHOD_BYTES; n > 0 with
 * d_body_offsets or d_body_lens NULL; bodies_bytes > 0 with d_bodies NULL;
 * nmethods > 0 with d_method_off NULL; method_bytes > 0 with d_method_names
 * NULL; exactly one of d_order / d_group_first given.  n == 0 writes the
 * nmethods + 4 words of d_group_first as 0 when it is given and is otherwise
 * RPCCRC_OK with no device touched. */
#define RPC_ROUTE_NONE 0u      /* not a DATA entry: nothing to route */
#define RPC_ROUTE_CALL 1u      /* a request for method d_method[i] */
#define RPC_ROUTE_NOT_FOUND 2u /* a request for a method the table does not hold (-32601 from d_id[i]) */
#define RPC_ROUTE_INVALID 3u   /* no string `method`, or an id above 4294967295 (-32600 from d_id[i]) */
#define RPC_ROUTE_DEFER 4u     /* outside the strict subset: the host's full parser decides */
#define RPC_ROUTE_RANGE 5u     /* the body does not lie inside d_bodies: nothing read */
#define RPC_ROUTE_NO_METHOD 0xFFFFu
#define RPC_ROUTE_MAX_BODY 1024u /* = RPC_MAX_BODY_LEN */
#define RPC_ROUTE_MAX_DEPTH 32u
#define RPC_ROUTE_MAX_TOKENS 256u
#define RPC_ROUTE_MAX_METHODS 256u
#define RPC_ROUTE_MAX_METHOD_BYTES 4096u
RPCCRC_API int rpc_frames_route_device(const uint8_t *d_bodies, uint64_t bodies_bytes,
                           const uint64_t *d_body_offsets, const uint32_t *d_body_lens,
                           const uint16_t *d_reply_types, uint64_t n,
                           const uint8_t *d_method_names, uint32_t method_bytes,
                           const uint32_t *d_method_off, uint32_t nmethods,
                           uint8_t *d_kind, uint16_t *d_method, uint32_t *d_id,
                           uint32_t *d_params_off, uint32_t *d_params_len,
                           uint32_t *d_order, uint32_t *d_group_first, void *stream);

/* ---- frame reply: JSON-RPC reply bodies built from id + value ----------------
 * What sits between the handlers and the pack.  Every reply the reference's
 * dispatcher sends has one of two fixed forms around a variable part
 * (rpc_server_helpers.c:10-54, printed by cJSON_PrintUnformatted):
 *   {"jsonrpc":"2.0","id":<id>,"result":<value>}
 *   {"jsonrpc":"2.0","id":<id>,"error":{"code":<code>,"message":"<message>"}}
 * with <id> a uint32_t and <code> an int in plain decimal, and it only ever
 * sends five messages: Parse error (-32700), Invalid Request (-32600), Method
 * not found (-32601), Invalid params (-32602), Internal error (-32603)
 * (rpc_server_skeleton.c:118-260).  So a handler hands back only the value
 * text, and this call wraps it with the id the route left on the device,
 * answers the NOT_FOUND and INVALID groups without the host seeing them, lays
 * the bodies out back to back and leaves the pack's inputs ready.
 * d_kind and d_id are the route's outputs unchanged; d_kind == NULL means every
 * DATA entry is a CALL.  d_reply_types is the unpack's output unchanged; NULL
 * means every entry is DATA.  d_status[i] is the handler's verdict for a CALL: 0
 * a result, anything else the JSON-RPC error code; NULL means all 0.  Entry i's
 * value is d_values [d_value_offsets[i], + d_value_lens[i]).
 * For entry i, in this order:
 *   1. d_reply_types is given and d_reply_types[i] != RPC_FRAME_TYPE_DATA: size
 *      0, type out d_reply_types[i] (a PONG stays a PONG for the pack, NONE stays
 *      NONE), RPC_REPLY_NONE.  Nothing else of the entry is looked at.
 *   2. Kind RPC_ROUTE_NONE, RPC_ROUTE_RANGE or any value above it: size 0, type
 *      out RPC_FRAME_TYPE_NONE, RPC_REPLY_NONE.
 *   3. Kind NOT_FOUND: the error form with code -32601 and d_id[i]; kind
 *      INVALID: with code -32600 (the route has set d_id to 0 where the
 *      reference answers with id 0).  Neither d_status nor the value is looked
 *      at.  RPC_REPLY_ERROR.
 *   4. Kind CALL, with s = d_status ? d_status[i] : 0:
 *      s == 0: the result form around the value bytes, copied verbatim -- they
 *        are the caller's JSON text; nothing is validated or escaped -- and an
 *        empty value is written as null (this call's choice: the reference
 *        never has an empty result).  RPC_REPLY_RESULT.
 *      s one of the five codes above: the error form with that code and its
 *        fixed message; the value is not looked at.  RPC_REPLY_ERROR.
 *      any other s: the error form with code s printed as %d and the value
 *        bytes verbatim as the message (the caller has escaped them); an empty
 *        value gives the message `error`, the reference's default for a NULL
 *        message (rpc_server_helpers.c:29).  RPC_REPLY_ERROR.
 *   5. Kind DEFER: the host ran the full parser and built the whole reply: the
 *      body is the value bytes verbatim, RPC_REPLY_RAW.  An empty value means
 *      the host sends nothing: size 0, type NONE, RPC_REPLY_NONE.  d_status is
 *      not looked at.
 *   6. A value that rules 4-5 look at and that does not lie inside [0,
 *      values_bytes) (offset <= values_bytes and length <= values_bytes -
 *      offset, computed without 64-bit wrap; an empty value is held to it too),
 *      or a body whose length would not fit 32 bits: size 0, type NONE,
 *      RPC_REPLY_RANGE.  Nothing is read.
 * Layout: d_body_offsets[i] is the exclusive 64-bit sum of the sizes of entries
 * 0 .. i-1, d_body_lens[i] the size, *d_total the sum of all;
 * d_conn_bytes_first[c] is the body offset of entry d_conn_first[c],
 * d_conn_bytes_first[nconn] is *d_total (a CSR that runs past n reads as the
 * end).  The layout never depends on out_cap.
 * Capacity (the pack's rule): an entry of non-zero size that does not end
 * inside out_cap is not written, not even in part; it reads RPC_REPLY_NO_ROOM
 * with type NONE; its offset and length keep the layout's values.  No byte of
 * d_out outside a written entry is written.  d_out == NULL with out_cap == 0 is
 * the layout-only call.
 * Nothing outside [d_values, d_values + values_bytes) is read, not even by an
 * aligned load window.  d_out must not overlap d_values; d_types_out may be
 * d_reply_types.
 * The outputs are rpc_frames_pack_device's inputs unchanged: bodies d_out,
 * d_body_offsets, d_body_lens, types d_types_out (with the unpack's versions and
 * the same d_conn_first).  The length cap stays the pack's business (TOO_LARGE
 * there).
 * All pointers are device pointers; every output from d_body_offsets on is
 * optional; the call is asynchronous on `stream`.
 * RPCCRC_EINVAL, before any device is touched: n >= 0xFFFFFFFF; n > 0 with
 * d_id, d_value_offsets or d_value_lens NULL; values_bytes > 0 with d_values
 * NULL; out_cap > 0 with d_out NULL; d_conn_bytes_first without d_conn_first;
 * nconn > 0 with d_conn_first NULL.  n == 0 with neither d_total nor
 * d_conn_bytes_first is RPCCRC_OK with no device; with them, *d_total and the
 * nconn + 1 connection words are written as 0. */
#define RPC_REPLY_NONE 0u    /* nothing to send for this entry */
#define RPC_REPLY_RESULT 1u  /* the result form */
#define RPC_REPLY_ERROR 2u   /* the error form */
#define RPC_REPLY_RAW 3u     /* a deferred entry: the host's whole reply, verbatim */
#define RPC_REPLY_RANGE 4u   /* the value does not lie inside d_values, or the body is over 32 bits: nothing read */
#define RPC_REPLY_NO_ROOM 5u /* the entry does not end inside out_cap: nothing written */
RPCCRC_API int rpc_frames_reply_device(const uint8_t *d_kind, const uint32_t *d_id, const int32_t *d_status,
                           const uint16_t *d_reply_types, uint64_t n,
                           const uint8_t *d_values, uint64_t values_bytes,
                           const uint64_t *d_value_offsets, const uint32_t *d_value_lens,
                           const uint64_t *d_conn_first, uint64_t nconn,
                           uint8_t *d_out, uint64_t out_cap,
                           uint64_t *d_body_offsets, uint32_t *d_body_lens, uint16_t *d_types_out,
                           uint8_t *d_reply_status, uint64_t *d_conn_bytes_first, uint64_t *d_total,
                           void *stream);

/* ---- frame request: JSON-RPC request bodies built from method + params + id ----
 * The reply's mirror image: what sits in front of a client's pack.  Everything
 * the reference client sends is one function (client/rpc_codec.c:6-20, printed
 * by cJSON_PrintUnformatted):
 *   {"jsonrpc":"2.0","method":"<name>","params":<params>,"id":<id>}
 *   {"jsonrpc":"2.0","method":"<name>","id":<id>}                   (params == NULL)
 * with <id> a uint32_t in plain decimal and the name through cJSON's string
 * printer.  So a caller hands over a method index, the JSON text of its params
 * and an id, and this call writes the envelope, lays the bodies out back to
 * back and leaves the pack's inputs ready; the ids are
 * rpc_frames_resolve_device's d_pending_ids.
 * The method table is rpc_frames_route_device's (d_method_names, method_bytes,
 * d_method_off, nmethods, with its two limits), so a client and a server share
 * one table: d_method[i] is what the route would give back as the method index.
 * d_types are the pack's types; NULL means every entry is DATA.  Entry i's
 * value is d_params [d_params_offsets[i], + d_params_lens[i]).
 * For entry i, in this order:
 *   1. d_types is given and d_types[i] != RPC_FRAME_TYPE_DATA: size 0, type out
 *      d_types[i] (a client's PING stays a PING for the pack, NONE stays NONE),
 *      RPC_REQUEST_NONE.  Nothing else of the entry is looked at.
 *   2. d_method[i] == RPC_ROUTE_NO_METHOD: the host built the whole request (a
 *      notification without id, a name that needs escaping, anything outside
 *      the form): the body is the value bytes verbatim, RPC_REQUEST_RAW.  An
 *      empty value sends nothing: size 0, type NONE, RPC_REQUEST_NONE.  d_id is
 *      not looked at.
 *   3. RPC_REQUEST_BAD_METHOD, with size 0 and type NONE, if d_method[i] >=
 *      nmethods; if the name's table word is not monotone (off[m] > off[m + 1])
 *      or leaves method_bytes (rule 7 of the route: such a name matches nothing
 *      there); or if the name holds a byte below 0x20, `"` or `\`: the
 *      reference would print an escape there and the route compares raw bytes,
 *      so such a name could not round-trip.  Bytes >= 0x80 are copied as they
 *      are, as the reference does.  The empty name is legal.  Neither d_id nor
 *      the value is looked at.
 *   4. A value that rules 2 and 5 look at and that does not lie inside [0,
 *      params_bytes) (offset <= params_bytes and length <= params_bytes -
 *      offset, computed without 64-bit wrap; an empty value is held to it too),
 *      or a body whose length would not fit 32 bits: size 0, type NONE,
 *      RPC_REQUEST_RANGE.  Nothing is read.
 *   5. Otherwise RPC_REQUEST_CALL.  With a non-empty value the first form above
 *      around the value bytes, copied verbatim -- they are the caller's JSON
 *      text; nothing is validated or escaped -- of 45 + name + value + digits
 *      bytes.  With an empty value the second form, of 35 + name + digits bytes
 *      (the reference's answer for params == NULL).  Id 0 is written like any
 *      other (the reference's rpc_async_call refuses it; its server accepts it).
 * Layout: d_body_offsets[i] is the exclusive 64-bit sum of the sizes of entries
 * 0 .. i-1, d_body_lens[i] the size, *d_total the sum of all;
 * d_conn_bytes_first[c] is the body offset of entry d_conn_first[c],
 * d_conn_bytes_first[nconn] is *d_total (a CSR that runs past n reads as the
 * end).  The layout never depends on out_cap.
 * Capacity (the pack's rule): an entry of non-zero size that does not end
 * inside out_cap is not written, not even in part; it reads RPC_REQUEST_NO_ROOM
 * with type NONE; its offset and length keep the layout's values.  No byte of
 * d_out outside a written entry is written.  d_out == NULL with out_cap == 0 is
 * the layout-only call.
 * Nothing outside [d_params, d_params + params_bytes) and the two table arrays
 * is read, not even by an aligned load window.  d_out must not overlap
 * d_params; d_types_out may be d_types.
 * The outputs are rpc_frames_pack_device's inputs unchanged: bodies d_out,
 * d_body_offsets, d_body_lens, types d_types_out (with the same d_conn_first).
 * The length cap stays the pack's business (TOO_LARGE there).
 * All pointers are device pointers; every output from d_body_offsets on is
 * optional; the call is asynchronous on `stream`.
 * RPCCRC_EINVAL, before any device is touched: n >= 0xFFFFFFFF; nmethods >
 * RPC_ROUTE_MAX_METHODS; method_bytes > RPC_ROUTE_MAX_METHOD_BYTES; n > 0 with
 * d_method, d_id, d_params_offsets or d_params_lens NULL; params_bytes > 0 with
 * d_params NULL; nmethods > 0 with d_method_off NULL; method_bytes > 0 with
 * d_method_names NULL; out_cap > 0 with d_out NULL; d_conn_bytes_first without
 * d_conn_first; nconn > 0 with d_conn_first NULL.  n == 0 with neither d_total
 * nor d_conn_bytes_first is RPCCRC_OK with no device; with them, *d_total and
 * the nconn + 1 connection words are written as 0. */
#define RPC_REQUEST_NONE 0u       /* nothing to send for this entry */
#define RPC_REQUEST_CALL 1u       /* one of the two request forms */
#define RPC_REQUEST_RAW 2u        /* the host's whole request, verbatim */
#define RPC_REQUEST_BAD_METHOD 3u /* no such method, a broken table word, or a name that needs escaping */
#define RPC_REQUEST_RANGE 4u      /* the value does not lie inside d_params, or the body is over 32 bits: nothing read */
#define RPC_REQUEST_NO_ROOM 5u    /* the entry does not end inside out_cap: nothing written */
RPCCRC_API int rpc_frames_request_device(const uint16_t *d_method, const uint32_t *d_id, const uint16_t *d_types,
                           uint64_t n,
                           const uint8_t *d_method_names, uint32_t method_bytes,
                           const uint32_t *d_method_off, uint32_t nmethods,
                           const uint8_t *d_params, uint64_t params_bytes,
                           const uint64_t *d_params_offsets, const uint32_t *d_params_lens,
                           const uint64_t *d_conn_first, uint64_t nconn,
                           uint8_t *d_out, uint64_t out_cap,
                           uint64_t *d_body_offsets, uint32_t *d_body_lens, uint16_t *d_types_out,
                           uint8_t *d_request_status, uint64_t *d_conn_bytes_first, uint64_t *d_total,
                           void *stream);

/* ---- frame resolve: reply envelopes matched to pending ids -------------------
 * What sits between a client's unpack and its completions.  The reference
 * client parses each whole reply to learn its `id` and whether `result` or
 * `error` is there (client/rpc_codec.c:22-52) and completes the one call in
 * flight on the connection; a client that keeps many calls in flight has to
 * find the call by id.  This call gives, for every delivered body, the reply's
 * id, where its `result` and `error` values lie, and which of the caller's
 * pending slots it answers -- so that the host parses only the spans of calls
 * it completes.  Like the route it is not a JSON codec and accepts the same
 * strict subset; everything outside reads RPC_RESOLVE_DEFER and goes through
 * the full parser on the host as before.
 * d_bodies, d_body_offsets, d_body_lens and d_reply_types are the unpack's
 * outputs unchanged (nul 0 or 1: the NUL is never looked at); d_reply_types ==
 * NULL means every entry is DATA.  d_pending_ids[s] is the id of the call in
 * the caller's slot s.  For entry i, in this order:
 *   1. d_reply_types is given and d_reply_types[i] != RPC_FRAME_TYPE_DATA:
 *      RPC_RESOLVE_NONE.  The offset and the length are not looked at.
 *   2. The body does not lie inside [0, bodies_bytes) (computed without 64-bit
 *      wrap): RPC_RESOLVE_RANGE.  Nothing is read.
 *   3. RPC_RESOLVE_DEFER if the body is outside the route's strict subset: rule
 *      3 of rpc_frames_route_device word for word, with its three limits
 *      (RPC_ROUTE_MAX_BODY, RPC_ROUTE_MAX_DEPTH, RPC_ROUTE_MAX_TOKENS).
 *   4. RPC_RESOLVE_DEFER if a depth-1 key contains a backslash.
 *   5. Depth-1 keys are compared with `id`, `result` and `error` ignoring ASCII
 *      letter case, and the FIRST key that matches a name is that name's member
 *      (cJSON_GetObjectItem; the server's lookup is case-sensitive, so this
 *      differs from the route).  "ID":"x","id":5 has a string id.
 *   6. `id` is absent or not a number: RPC_RESOLVE_INVALID (the reference
 *      returns -1).  A number written as digits only with value <= 4294967295:
 *      that value.  Any other number form (sign, fraction, exponent), or digits
 *      only and larger: RPC_RESOLVE_DEFER (the reference casts a double).
 *   7. d_result_off / d_result_len and d_error_off / d_error_len are the spans
 *      of the two members' values, relative to the body's first byte, from the
 *      value's first byte to one past its last; 0 / 0 when absent.  A null
 *      value is present.  Both, one or neither may be there (the reference
 *      returns 0 in all four cases).
 *   8. A decoded entry whose id no slot holds: RPC_RESOLVE_UNKNOWN with
 *      d_slot[i] = RPC_RESOLVE_NO_SLOT.  Otherwise d_slot[i] is the LOWEST slot
 *      index holding that id (a table that holds an id twice never matches the
 *      later slots), and among the entries that name one slot the lowest entry
 *      index reads RPC_RESOLVE_MATCHED and every other RPC_RESOLVE_DUPLICATE:
 *      pending_take() called in arrival order, whose second take finds nothing.
 *   9. d_slot_entry[s] is the matched entry's index, or 0xFFFFFFFF while slot s
 *      stays open.  d_open lists the open slots in ascending order and *d_nopen
 *      is their count (both or neither; npending words always suffice).
 *
 *   kind                        d_id    spans     d_slot
 *   NONE, RANGE, DEFER, INVALID 0       0 / 0     RPC_RESOLVE_NO_SLOT
 *   UNKNOWN                     rule 6  rule 7    RPC_RESOLVE_NO_SLOT
 *   MATCHED, DUPLICATE          rule 6  rule 7    rule 8
 *
 * The result does not depend on the order in which lanes or workgroups run.
 * npending == 0 is the decode-only call: every decoded entry reads UNKNOWN.
 * Nothing outside [d_bodies, d_bodies + bodies_bytes) and d_pending_ids[0 ..
 * npending) is read, not even by an aligned load window.  All pointers are
 * device pointers; every output is optional; the call is asynchronous on
 * `stream`.
 * RPCCRC_EINVAL, before any device is touched: n >= 0xFFFFFFFF; npending >
 * RPC_RESOLVE_MAX_PENDING; n > 0 with d_body_offsets or d_body_lens NULL;
 * bodies_bytes > 0 with d_bodies NULL; npending > 0 with d_pending_ids NULL;
 * exactly one of d_open / d_nopen given.  n == 0 still writes d_slot_entry,
 * d_open and *d_nopen (every slot open) when they are given and is otherwise
 * RPCCRC_OK with no device touched. */
#define RPC_RESOLVE_NONE 0u      /* not a DATA entry: nothing to resolve */
#define RPC_RESOLVE_MATCHED 1u   /* the reply that completes slot d_slot[i] */
#define RPC_RESOLVE_UNKNOWN 2u   /* a reply whose id no slot holds */
#define RPC_RESOLVE_DUPLICATE 3u /* a reply to slot d_slot[i] behind the one that took it */
#define RPC_RESOLVE_INVALID 4u   /* no numeric `id` (the reference's -1) */
#define RPC_RESOLVE_DEFER 5u     /* outside the strict subset: the host's full parser decides */
#define RPC_RESOLVE_RANGE 6u     /* the body does not lie inside d_bodies: nothing read */
#define RPC_RESOLVE_NO_SLOT 0xFFFFFFFFu
#define RPC_RESOLVE_MAX_PENDING (1u << 24)
RPCCRC_API int rpc_frames_resolve_device(const uint8_t *d_bodies, uint64_t bodies_bytes,
                           const uint64_t *d_body_offsets, const uint32_t *d_body_lens,
                           const uint16_t *d_reply_types, uint64_t n,
                           const uint32_t *d_pending_ids, uint32_t npending,
                           uint8_t *d_kind, uint32_t *d_id,
                           uint32_t *d_result_off, uint32_t *d_result_len,
                           uint32_t *d_error_off, uint32_t *d_error_len,
                           uint32_t *d_slot, uint32_t *d_slot_entry,
                           uint32_t *d_open, uint32_t *d_nopen, void *stream);

/* ---- frame args: typed params decoded per method schema ----------------------
 * What sits between the route and the handlers.  The reference's generated
 * rpc_parse_params_<method> functions (rpc_server_skeleton.c:13-116,
 * rpc_parse_i64_value in rpc_server_helpers.c:56-75) look a fixed list of
 * (name, type) up in the flat `params` object by case-sensitive name; there
 * are five types.  This call does that for every CALL entry of a route: it
 * decodes the method's declared parameters into typed 64-bit slots, column by
 * column, so that a handler runs once over arrays of numbers and the -32602
 * answers are decided without the host seeing them.  Like the route it is not
 * a JSON codec: it accepts a strict subset, inside the subset its answer is
 * the reference's, and everything else reads RPC_ARGS_DEFER and goes through
 * the host's parser on the span as before.
 * d_bodies, d_body_offsets, d_body_lens are the unpack's outputs; d_kind,
 * d_method, d_params_off, d_params_len the route's, all unchanged.  The schema:
 * method m declares parameters [d_param_first[m], d_param_first[m + 1]) (a CSR
 * of nmethods + 1 words, in the order of the route's table); parameter p has
 * type d_param_types[p] (RPC_ARG_*) and the name bytes [d_param_name_off[p],
 * d_param_name_off[p + 1]) of d_param_names.  `width` is the slots per entry.
 * For entry i, in this order:
 *   1. d_kind[i] != RPC_ROUTE_CALL: RPC_ARGS_NONE.  Nothing else of the entry
 *      is looked at.
 *   2. RPC_ARGS_BAD_SCHEMA, with no body byte read, if d_method[i] >= nmethods;
 *      if the method's two CSR words are not monotone or leave nparams; if the
 *      method has more than `width` parameters; if one of its parameters has an
 *      unknown type code or name words that are not monotone or leave
 *      name_bytes.  (Only the entry's own method is looked at.)
 *   3. RPC_ARGS_RANGE, with nothing read, if the body does not lie inside
 *      [0, bodies_bytes) or the span does not lie inside the body (both
 *      computed without wrap).
 *   4. The method declares no parameters: RPC_ARGS_OK, and the span is not
 *      read (the reference's `ping` takes any params, absent ones included).
 *   5. d_params_len[i] == 0: RPC_ARGS_INVALID (the reference substitutes {} and
 *      every lookup fails).
 *   6. RPC_ARGS_DEFER unless the span is one strict JSON value -- an object,
 *      array, string, number or literal by the grammar of the route's rule 3,
 *      with no byte, whitespace included, before or after the value -- of at
 *      most RPC_ROUTE_MAX_BODY bytes, nested no deeper than
 *      RPC_ROUTE_MAX_DEPTH - 1 (the span's outermost container is depth 1) and
 *      with at most RPC_ROUTE_MAX_TOKENS tokens, counted as the route counts.
 *   7. A strict value that is not an object: RPC_ARGS_INVALID ([1,2] and null
 *      answer -32602 in the reference).
 *   8. RPC_ARGS_DEFER if a depth-1 key of the object contains a backslash.
 *      Keys are compared as raw bytes, case-sensitively, and the FIRST equal
 *      key wins: {"a":1,"a":5} reads 1, {"A":1,"a":3} reads 3.  Other keys and
 *      anything nested are skipped.  Two parameters of one name read the same
 *      value; the empty name is legal.
 *   9. RPC_ARGS_INVALID if a declared parameter is absent or its value is of a
 *      JSON type its declared type does not take, judged from the value's
 *      first byte alone, before any conversion (so INVALID wins over DEFER, as
 *      in the reference): a number takes I32, I64, F64; true / false takes
 *      BOOL only; a string takes STR and I64; null, an object and an array
 *      take none.
 *  10. Otherwise each parameter is converted; RPC_ARGS_DEFER if a conversion
 *      leaves the subset, else RPC_ARGS_OK:
 *      F64   the bit pattern of the double strtod gives, correctly rounded.
 *            In the subset: at most 19 significant digits once leading zeros
 *            are stripped (trailing zeros count), and a result that is zero
 *            because every digit is 0 (the sign is kept: -0.0 is
 *            0x8000000000000000) or a normal double.  DEFER: more digits, a
 *            non-zero number whose double is zero, subnormal or infinite.
 *      I32   with d the F64 conversion: (int64_t)trunc(d) when -2147483649 < d
 *            < 2147483648 (the reference's (int32_t)valuedouble: 1.9 -> 1,
 *            -1.9 -> -1, 1e3 -> 1000), else DEFER (the cast is undefined there).
 *      I64   from a number: (int64_t)trunc(d) when -2^63 <= d < 2^63, else
 *            DEFER (9007199254740993 reads ...992, through the double, as in
 *            the reference).  From a string, the reference's strtoll path and
 *            what its client sends: -?[0-9]{1,19} with a value inside int64
 *            gives that value; every other string is DEFER (the host runs
 *            strtoll: blanks and '+' are accepted there, "12a" and "" are
 *            -32602, an overflow saturates).
 *      BOOL  1 or 0.
 *      STR   offset | (uint64_t)length << 32 of the bytes between the quotes,
 *            the offset relative to the body's first byte.  A backslash
 *            inside is DEFER: the host unescapes.
 * d_slots (width * n words) holds slot k of entry i at k * n + i, column-major:
 * for OK the method's parameters in declaration order and 0 behind them, for
 * every other status `width` zeros.  d_status is the RPC_ARGS_* above;
 * d_reply_status is 0 for OK, -32602 for INVALID and -32603 for everything
 * else, and goes to rpc_frames_reply_device as its d_status (the host
 * overwrites it for the DEFER entries it handles; an entry nobody handled
 * answers "Internal error", never an empty result).
 * Nothing outside [d_bodies, d_bodies + bodies_bytes) and the schema arrays is
 * read, not even by an aligned load window.  All pointers are device pointers;
 * every output is optional; the call is asynchronous on `stream`.
 * RPCCRC_EINVAL, before any device is touched: n >= 0xFFFFFFFF; nmethods >
 * RPC_ROUTE_MAX_METHODS; nparams > RPC_ARGS_MAX_SCHEMA_PARAMS; name_bytes >
 * RPC_ARGS_MAX_NAME_BYTES; width 0 or > RPC_ARGS_MAX_PARAMS; n > 0 with
 * d_body_offsets, d_body_lens, d_kind, d_method, d_params_off or d_params_len
 * NULL; bodies_bytes > 0 with d_bodies NULL; nmethods > 0 with d_param_first
 * NULL; nparams > 0 with d_param_types or d_param_name_off NULL; name_bytes > 0
 * with d_param_names NULL.  n == 0 is RPCCRC_OK with no device touched. */
#define RPC_ARGS_NONE 0u       /* not a CALL entry: nothing to decode */
#define RPC_ARGS_OK 1u         /* every declared parameter decoded */
#define RPC_ARGS_INVALID 2u    /* a parameter absent or of the wrong JSON type (-32602) */
#define RPC_ARGS_DEFER 3u      /* outside the strict subset: the host's parser decides */
#define RPC_ARGS_RANGE 4u      /* the body or the span lies outside its buffer: nothing read */
#define RPC_ARGS_BAD_SCHEMA 5u /* the method's schema words are broken: no body byte read */
#define RPC_ARG_I32 0u
#define RPC_ARG_I64 1u
#define RPC_ARG_F64 2u
#define RPC_ARG_BOOL 3u
#define RPC_ARG_STR 4u
#define RPC_ARGS_MAX_PARAMS 8u
#define RPC_ARGS_MAX_SCHEMA_PARAMS 1024u
#define RPC_ARGS_MAX_NAME_BYTES 4096u
RPCCRC_API int rpc_frames_args_device(const uint8_t *d_bodies, uint64_t bodies_bytes,
                           const uint64_t *d_body_offsets, const uint32_t *d_body_lens,
                           const uint8_t *d_kind, const uint16_t *d_method,
                           const uint32_t *d_params_off, const uint32_t *d_params_len, uint64_t n,
                           const uint32_t *d_param_first, uint32_t nmethods,
                           const uint8_t *d_param_types, const uint32_t *d_param_name_off, uint32_t nparams,
                           const uint8_t *d_param_names, uint32_t name_bytes, uint32_t width,
                           uint64_t *d_slots, uint8_t *d_status, int32_t *d_reply_status, void *stream);

/* ---- frame results: typed results decoded per pending slot --------------------
 * What sits between a client's resolve and its completions: the args' mirror on
 * the client side.  The reference's generated client stubs
 * (client/gen/rpc_client_gen.c) read the `result` member that
 * rpc_codec_decode_response hands over in one of five fixed shapes, one per IDL
 * result type -- cJSON_IsString -> the string; cJSON_IsString -> strtoll, or
 * cJSON_IsNumber -> (int64_t)valuedouble; cJSON_IsNumber -> (int32_t)valuedouble;
 * cJSON_IsNumber -> valuedouble; cJSON_IsBool -> cJSON_IsTrue -- return their
 * default (0, 0.0, false, NULL) in every other case and never look at `error`.
 * This call does that for every MATCHED entry of a resolve and leaves the
 * completions indexed by pending slot, so that only columns cross to the host.
 * Like the args it is not a JSON codec: inside its strict subset the answer is
 * the reference's, everything else reads RPC_RESULTS_DEFER and goes through the
 * host's parser on the span as before.
 * d_bodies, d_body_offsets, d_body_lens are the unpack's outputs; d_kind,
 * d_slot, d_result_off, d_result_len, d_error_off, d_error_len, d_slot_entry
 * the resolve's, all unchanged.  d_pending_method[s] (npending words) is the
 * method index slot s's request was sent with -- the d_method given to
 * rpc_frames_request_device -- and d_result_types[m] (nmethods bytes, RPC_ARG_*)
 * the array rpc_frames_values_device's RESULT form takes.
 * For entry i, in this order:
 *   1. d_kind[i] != RPC_RESOLVE_MATCHED: RPC_RESULTS_NONE.  Nothing else of the
 *      entry is looked at (pending_take finds nothing for an UNKNOWN or a
 *      DUPLICATE reply: the reference drops it).
 *   2. RPC_RESULTS_BAD_SCHEMA, with no body byte read, if d_slot[i] >= npending;
 *      if d_pending_method[d_slot[i]] >= nmethods; if that method's type is not
 *      an RPC_ARG_*.
 *   3. RPC_RESULTS_RANGE, with nothing read, if the body does not lie inside
 *      [0, bodies_bytes) or one of the two spans does not lie inside the body
 *      (all computed without wrap).  A span of length 0 is not checked.
 *   4. d_result_len[i] == 0: RPC_RESULTS_ABSENT, value 0 (no `result`: the
 *      reference returns the default).
 *   5. RPC_RESULTS_DEFER unless the span is one strict JSON value: rule 6 of
 *      rpc_frames_args_device word for word, with its three limits.  A body
 *      longer than RPC_ROUTE_MAX_BODY defers as well (it is not staged), and so
 *      does an object with a backslash in a depth-1 key (the args' rule 8 rides
 *      along with their walk; the host's answer is the default either way).
 *   6. The value's JSON type, judged from its first byte alone, against the
 *      declared type: a number takes I32, I64, F64; a string takes STR and I64;
 *      true / false takes BOOL; null, an object and an array take none.  A
 *      value the type does not take: RPC_RESULTS_MISMATCH, value 0 -- the
 *      default the reference returns, also for the null its server prints for
 *      a NaN or an infinity.
 *   7. The conversion of rpc_frames_args_device's rule 10 word for word, with
 *      every DEFER class it names: I32, I64, F64 from a number; I64 from a
 *      string; BOOL; STR as offset | (uint64_t)length << 32 of the bytes
 *      between the quotes, the offset relative to the body's first byte, where
 *      a backslash inside is DEFER.  RPC_RESULTS_OK with the value, or
 *      RPC_RESULTS_DEFER with value 0.
 * `error` is decoded independently of the value, with a status of its own in
 * the same codes.  d_error_len[i] == 0: ABSENT.  Else the span goes through
 * rules 6-10 of rpc_frames_args_device as if it were the `params` of a method
 * declaring (code: I32, message: STR): OK there is OK here, with d_error_code[i]
 * and d_error_message[i] (offset | length << 32, relative to the body);
 * INVALID there is MISMATCH, DEFER is DEFER, both with zeros.  (A span inside a
 * body longer than RPC_ROUTE_MAX_BODY: DEFER.)  An entry whose status is NONE,
 * BAD_SCHEMA or RANGE has error status ABSENT and zeros.
 * Per slot s, with e = d_slot_entry[s]: if e < n, d_kind[e] ==
 * RPC_RESOLVE_MATCHED and d_slot[e] == s, then d_slot_status[s],
 * d_slot_value[s], d_slot_error_status[s] and d_slot_error_code[s] are entry
 * e's answers and d_slot_str_base[s] is d_body_offsets[e] -- the d_str_base of
 * rpc_frames_values_device, so that a STR completion can be echoed where it
 * lies.  Otherwise the slot is open and all five read 0.  At most one entry
 * passes that test for a slot, whatever the input (two MATCHED entries naming
 * one slot among them): the answer does not depend on the order in which lanes
 * or workgroups run.
 * *d_ndefer is the number of entries whose status or error status is DEFER,
 * each counted once: non-zero tells the host to parse those spans.
 * Nothing outside [d_bodies, d_bodies + bodies_bytes), the two schema arrays
 * and the listed inputs is read, not even by an aligned load window.  All
 * pointers are device pointers; every output is optional; the call is
 * asynchronous on `stream` and needs no workspace.
 * RPCCRC_EINVAL, before any device is touched: n >= 0xFFFFFFFF; npending >
 * RPC_RESOLVE_MAX_PENDING; nmethods > RPC_ROUTE_MAX_METHODS; n > 0 with
 * d_body_offsets, d_body_lens, d_kind, d_slot, d_result_off, d_result_len,
 * d_error_off or d_error_len NULL; bodies_bytes > 0 with d_bodies NULL;
 * npending > 0 with d_pending_method NULL; nmethods > 0 with d_result_types
 * NULL; a per-slot output given without d_slot_entry.  n == 0 still writes the
 * per-slot outputs (every slot open) and *d_ndefer = 0 when they are given and
 * is otherwise RPCCRC_OK with no device touched. */
#define RPC_RESULTS_NONE 0u       /* not a MATCHED entry; an open slot */
#define RPC_RESULTS_OK 1u         /* the member decoded */
#define RPC_RESULTS_ABSENT 2u     /* the reply has no such member: the default */
#define RPC_RESULTS_MISMATCH 3u   /* a JSON type the declared type does not take: the default */
#define RPC_RESULTS_DEFER 4u      /* outside the strict subset: the host's parser decides */
#define RPC_RESULTS_RANGE 5u      /* the body or a span lies outside its buffer: nothing read */
#define RPC_RESULTS_BAD_SCHEMA 6u /* no such slot, method or type: no body byte read */
RPCCRC_API int rpc_frames_results_device(const uint8_t *d_bodies, uint64_t bodies_bytes,
                           const uint64_t *d_body_offsets, const uint32_t *d_body_lens,
                           const uint8_t *d_kind, const uint32_t *d_slot,
                           const uint32_t *d_result_off, const uint32_t *d_result_len,
                           const uint32_t *d_error_off, const uint32_t *d_error_len,
                           const uint32_t *d_slot_entry, uint64_t n,
                           const uint16_t *d_pending_method, uint32_t npending,
                           const uint8_t *d_result_types, uint32_t nmethods,
                           uint8_t *d_status, uint64_t *d_value, uint8_t *d_error_status,
                           int32_t *d_error_code, uint64_t *d_error_message,
                           uint8_t *d_slot_status, uint64_t *d_slot_value, uint8_t *d_slot_error_status,
                           int32_t *d_slot_error_code, uint64_t *d_slot_str_base,
                           uint32_t *d_ndefer, void *stream);

/* ---- frame values: typed results and params as JSON text ---------------------
 * The args' mirror: what sits between the handlers' typed columns and
 * rpc_frames_reply_device, and between a client's columns and
 * rpc_frames_request_device.  The reference formats one value at a time, by a
 * fixed schema: the server's results are one of five types per method
 * (rpc_server_skeleton.c:162-257), the client's params a fixed list of (name,
 * type) per method (client/gen/rpc_client_gen.c, the cJSON_Add*ToObject
 * lines).  This call formats a whole batch from the slots the args leave, so
 * that only column bytes cross to the host and back.
 * Entry i has a mode d_mode[i] (NULL: RPC_VALUES_MODE_ENCODE for all), the
 * handler's verdict d_status[i] (NULL: 0 for all; it may be the args'
 * d_reply_status with the host's overwrites), a method d_method[i] and `width`
 * slots d_slots[k * n + i], column-major exactly as the args leave them.
 * form RPC_VALUES_FORM_RESULT takes one type per method, d_result_types[m]
 * (RPC_ARG_*), and uses slot 0 only; the four parameter arrays are not looked
 * at.  form RPC_VALUES_FORM_PARAMS takes the args' four schema arrays
 * unchanged; d_result_types is not looked at.  For entry i, in this order:
 *   1. d_status[i] != 0: RPC_VALUES_NONE, size 0 (the reply does not look at
 *      the value of such an entry).  Nothing else of the entry is looked at.
 *   2. mode RPC_VALUES_MODE_TEXT: the entry is the host's text
 *      d_texts[d_text_offsets[i], + d_text_lens[i]), copied verbatim (the
 *      reply's RAW form, the request's verbatim entries, a DEFER entry the host
 *      formatted, anything it chose to format itself): RPC_VALUES_TEXT.
 *      RPC_VALUES_RANGE, with nothing read, if the span does not lie inside
 *      [0, texts_bytes) or d_text_offsets or d_text_lens is NULL.
 *   3. Any mode but RPC_VALUES_MODE_ENCODE: RPC_VALUES_NONE, size 0.
 *   4. RPC_VALUES_BAD_SCHEMA, with no string byte read, if d_method[i] >=
 *      nmethods; RESULT: if the method's type is not an RPC_ARG_*; PARAMS: if
 *      the method's two CSR words are not monotone or leave nparams, if it has
 *      more than `width` parameters, if one of its parameters has an unknown
 *      type or name words that are not monotone or leave name_bytes (the args'
 *      rule 2), or a name with a byte the reference would escape (below 0x20,
 *      '"' or '\').
 *   5. RPC_VALUES_RANGE, with no string byte read, if a STR slot's span leaves
 *      the strings: a STR slot is offset | (uint64_t)length << 32, the args'
 *      encoding, relative to d_str_base[i] (NULL: 0), and d_str_base[i] +
 *      offset, computed without 64-bit wrap, and the length must lie inside
 *      [0, strings_bytes).  (With d_strings the unpack's bodies and d_str_base
 *      its body offsets a handler echoes a string the args found without
 *      moving it.)
 *   6. Each value's text, RPC_VALUES_DEFER if one has none here:
 *      I32   %d of the slot's low 32 bits read as int32_t
 *            (cJSON_CreateNumber((double)r): every int prints as its digits).
 *      I64   a JSON string, '"' + %lld + '"': the reference sends i64 quoted in
 *            both directions (skeleton :183-185, client gen :52-53), and the
 *            args' I64-from-string path reads it back.
 *      BOOL  true when the slot is non-zero, else false.
 *      STR   '"' + the bytes + '"'; bytes >= 0x80 as they are.  A byte below
 *            0x20, a '"' or a '\' is DEFER: the reference would escape it
 *            (print_string_ptr), and a 0 byte ends its C string.
 *      F64   the bytes of print_number (third_party/cJSON.c:591-658) for the
 *            double d with the slot's bits:
 *            a. NaN or an infinity: null.
 *            b. d integer-valued with -2147483648 <= d <= 2147483647: %d.
 *               -0.0 prints 0; 2147483648.0 is not this case (valueint
 *               saturates) and prints 2147483648 by d.
 *            c. d subnormal: DEFER.
 *            d. t15 = "%.15g" of d, r = strtod(t15); the text is t15 when
 *               fabs(r - d) <= fmax(fabs(r), fabs(d)) * DBL_EPSILON, evaluated
 *               in doubles, else "%.17g" of d.  Both correctly rounded, exact
 *               ties to even, in C's %g shape.  At most 24 bytes.  Not the
 *               shortest round-trip text: 0.1 + 0.2 prints 0.3 (one ulp away
 *               keeps 15 digits), 1/3 prints 0.33333333333333331 (17 digits,
 *               never 16), 9.999999999999999e22 prints 1e+23, 1e-05 but
 *               0.0001, 1e+15 but 123456789012345, 100000000000000.5 prints
 *               itself.  Above 1.797693134862315e308 t15 reads back as
 *               infinity and inf <= inf keeps the 15 digits:
 *               1.7976931348623157e308 prints 1.79769313486232e+308.
 *            An F64 value is the rule's bytes or the entry is DEFER, never a
 *            wrong digit.  The DEFER classes: (1) a subnormal d; (2) a rounding
 *            the implementation proved it cannot decide: the digits are d's
 *            significand times a 128-bit power of ten whose error is bounded,
 *            and a fraction within that bound of one half is undecided unless
 *            the power is exact (10^0 .. 10^55) or an exact integer compare
 *            settles it (10^-1 .. 10^-27) -- every tie of a 53-bit significand
 *            lies in those two ranges, and no double is known to fall in this
 *            class; (3) a read-back r that leaves the converter's range: r is
 *            neither normal, nor infinite, nor one of the subnormals beside
 *            the smallest normal for which step d is decided in integers.
 *   7. RESULT: the entry is the value text.  PARAMS: '{' + '"name":value' per
 *      declared parameter in declaration order, joined by ',', + '}', no
 *      blanks (cJSON_PrintUnformatted); a method without parameters gives {}.
 *      RPC_VALUES_OK.  An entry over 32 bits is RPC_VALUES_RANGE; that is
 *      judged from the slots alone, before any string byte is read, a value
 *      that has no text (rule 6) counting no bytes, nor its name, so it wins
 *      over DEFER.
 * Precedence within an entry: BAD_SCHEMA, then RANGE, then DEFER, then OK.
 * Every entry that is not OK or TEXT has size 0.
 * d_value_offsets[i] is the exclusive 64-bit sum of the sizes, d_value_lens[i]
 * the size and *d_total their sum; the layout never depends on out_cap.  An
 * entry that does not end inside out_cap is not written, not even in part, and
 * reads RPC_VALUES_NO_ROOM; no byte of d_out outside a written entry is
 * written; d_out NULL with out_cap 0 is the layout-only call.  *d_ndefer is the
 * number of DEFER entries: a non-zero count means the host formats those and
 * calls again with them as TEXT.  d_reply_status[i] is d_status[i] (0 without
 * one) for NONE, OK and TEXT and -32603 for every other status: an entry
 * nobody handled answers "Internal error", never a wrong or empty result.
 * d_out, d_value_offsets, d_value_lens, d_reply_status are the reply's
 * d_values, d_value_offsets, d_value_lens, d_status in RESULT form and the
 * request's d_params, d_params_offsets, d_params_lens in PARAMS form.
 * No byte outside d_strings, d_texts, the slots and the schema arrays is read,
 * not even by an aligned load window.  All pointers are device pointers; every
 * output is optional; the call is asynchronous on `stream`.
 * RPCCRC_EINVAL, before any device is touched: form neither of the two; n *
 * (PARAMS: width, RESULT: 1) >= 0xFFFFFFFF; width 0 or > RPC_ARGS_MAX_PARAMS;
 * nmethods > RPC_ROUTE_MAX_METHODS; out_cap > 0 with d_out NULL; n > 0 with
 * d_method or d_slots NULL; strings_bytes > 0 with d_strings NULL; texts_bytes
 * > 0 with d_texts NULL; RESULT: nmethods > 0 with d_result_types NULL; PARAMS:
 * nparams > RPC_ARGS_MAX_SCHEMA_PARAMS, name_bytes > RPC_ARGS_MAX_NAME_BYTES,
 * nmethods > 0 with d_param_first NULL, nparams > 0 with d_param_types or
 * d_param_name_off NULL, name_bytes > 0 with d_param_names NULL.  n == 0 with
 * neither d_total nor d_ndefer is RPCCRC_OK with no device; with them, they
 * are written as 0. */
#define RPC_VALUES_NONE 0u       /* nothing to format for this entry */
#define RPC_VALUES_OK 1u         /* text from the slots */
#define RPC_VALUES_TEXT 2u       /* the host's text, verbatim */
#define RPC_VALUES_DEFER 3u      /* a value has no text here: the host formats the entry */
#define RPC_VALUES_RANGE 4u      /* a span lies outside its buffer, or the entry is over 32 bits: nothing read */
#define RPC_VALUES_BAD_SCHEMA 5u /* the method's schema words are broken: no string byte read */
#define RPC_VALUES_NO_ROOM 6u    /* the entry does not end inside out_cap: nothing written */
#define RPC_VALUES_MODE_NONE 0u
#define RPC_VALUES_MODE_ENCODE 1u
#define RPC_VALUES_MODE_TEXT 2u
#define RPC_VALUES_FORM_RESULT 0
#define RPC_VALUES_FORM_PARAMS 1
RPCCRC_API int rpc_frames_values_device(int form, const uint8_t *d_mode, const int32_t *d_status,
                           const uint16_t *d_method, const uint64_t *d_slots, uint32_t width, uint64_t n,
                           const uint8_t *d_result_types,
                           const uint32_t *d_param_first, uint32_t nmethods,
                           const uint8_t *d_param_types, const uint32_t *d_param_name_off, uint32_t nparams,
                           const uint8_t *d_param_names, uint32_t name_bytes,
                           const uint8_t *d_strings, uint64_t strings_bytes, const uint64_t *d_str_base,
                           const uint8_t *d_texts, uint64_t texts_bytes,
                           const uint64_t *d_text_offsets, const uint32_t *d_text_lens,
                           uint8_t *d_out, uint64_t out_cap,
                           uint64_t *d_value_offsets, uint32_t *d_value_lens, uint8_t *d_values_status,
                           int32_t *d_reply_status, uint32_t *d_ndefer, uint64_t *d_total, void *stream);

/* ---- batched server receive ring -------------------
 * Replaces the one-frame-at-a-time verify of the reference server loop
 * (server/rpc_server_main.c:135-238, verify at :227) for a receive loop that
 * batches: frames from any connections are landed straight into pinned host
 * segments (recv() into the pointer rpc_rx_ring_reserve returns, then
 * rpc_rx_ring_commit), a full segment -- or one flushed by rpc_rx_ring_submit
 * -- is verified on the GPU (one H2D copy, rpc_frames_verify_device, one D2H
 * copy of the verdicts) while the next one fills, and rpc_rx_ring_poll returns
 * the verdicts in arrival order with the caller's tag.  A ring is used by one
 * thread; it works on the HIP device current at creation. */
typedef struct rpc_rx_ring rpc_rx_ring_t;

typedef struct {
  uint64_t tag;         /* the caller's tag from rpc_rx_ring_commit / _push */
  const uint8_t *frame; /* the frame (12-byte header + body) in the ring's pinned
                           memory; valid until the next rpc_rx_ring_poll */
  uint32_t body_len;    /* header fields, host order (rpc.h:3-8) */
  uint16_t version;
  uint16_t type;
  uint32_t header_crc;  /* the crc32 the sender stamped */
  uint32_t crc;         /* rpc_crc32 of the body, computed on the GPU (0 if not read) */
  uint8_t ok;           /* verdict is RPC_FRAME_OK or RPC_FRAME_CONTROL */
  uint8_t verdict;      /* RPC_FRAME_* */
} rpc_rx_frame_t;

/* nsegments (2..64) segments of segment_bytes bytes and max_frames frames each;
 * flags as rpc_frames_verify_device (one role bit, optionally LIFT_CAP). */
RPCCRC_API int rpc_rx_ring_create(rpc_rx_ring_t **ring, size_t segment_bytes, size_t max_frames, int nsegments,
                                  int flags);
RPCCRC_API void rpc_rx_ring_destroy(rpc_rx_ring_t *ring);
/* *dst = where to land a frame of frame_len bytes (header + body).  A segment
 * that cannot take it is submitted first; RPCCRC_EAGAIN when every segment is
 * still in flight or unpolled (call rpc_rx_ring_poll). */
RPCCRC_API int rpc_rx_ring_reserve(rpc_rx_ring_t *ring, size_t frame_len, uint8_t **dst);
/* Accepts the reserved frame; RPCCRC_EINVAL (frame dropped) unless the landed
 * length is exactly what the reference reads for that header: 12 + body_len for
 * a data frame, the 12-byte header alone for a control frame or a data frame over
 * the cap (the reference reads no body for either, rpc_server_main.c:172-195,
 * rpc_async.c:303-315; the bytes after such a header belong to the next frame). */
RPCCRC_API int rpc_rx_ring_commit(rpc_rx_ring_t *ring, uint64_t tag);
/* reserve + memcpy + commit. */
RPCCRC_API int rpc_rx_ring_push(rpc_rx_ring_t *ring, const void *frame, size_t frame_len, uint64_t tag);
/* Sends the partly filled segment to the GPU now (e.g. when the socket loop idles). */
RPCCRC_API int rpc_rx_ring_submit(rpc_rx_ring_t *ring);
/* Up to max_frames verdicts of the oldest submitted segment, in arrival order;
 * returns their count (0 if none is ready and wait == 0) or a negative code. */
RPCCRC_API int64_t rpc_rx_ring_poll(rpc_rx_ring_t *ring, rpc_rx_frame_t *out, size_t max_frames, int wait);

/* ---- helpers ----------------------------------------------------------- */

/* zlib crc32_combine (zlib.h:1750): crc(A||B) from crc(A), crc(B), |B|. */
RPCCRC_API uint32_t rpc_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* Fill d_dst with the counter-based splitmix64 stream used by tests/bench
 * (word k = mix64(seed + (k+1)*0x9E3779B97F4A7C15), little-endian).
 * nbytes must be a multiple of 8. */
RPCCRC_API int rpc_crc32_fill_random_device(void *d_dst, uint64_t nbytes, uint64_t seed, void *stream);

/* HBM read probe over nbytes (multiple of 4096): pattern 0 = coalesced 16-B
 * lanes, 1 = the CRC kernel's 64-B-per-lane segments (both a plain grid-stride
 * loop), 2 = the rows kernel itself with its CRC work compiled out: the same
 * dealing (workgroup rounds + tail stealing), loads (4 x 16 B non-temporal per
 * lane, a row ahead) and launch shape, i.e. the ceiling of the product's memory
 * stream (nbytes >= 256 MiB on 256 CUs; `nontemporal` is ignored). */
RPCCRC_API int rpc_crc32_stream_read_device(const void *d_src, uint64_t nbytes, int pattern, int nontemporal, void *stream);

/* Tuning knobs (process-wide): nontemporal loads (0/1, default 1) and the
 * persistent-grid size cap in workgroups (0 = one per CU). */
RPCCRC_API int rpc_crc32_set_options(int nontemporal, int max_blocks);

/* Kernel for ragged device batches (process-wide; used by rpc_crc32_device_batch,
 * rpc_crc32_batch and the frames calls).  Results are identical either way.
 *   RPCCRC_RAGGED_AUTO   frames calls (bodies <= MAX_BODY_LEN): split;
 *                        other batches: rows (default)
 *   RPCCRC_RAGGED_ROWS   one wavefront per body, 4 KiB rows
 *   RPCCRC_RAGGED_PACKED 1 KiB chunks of consecutive bodies packed four per
 *                        row, balanced by chunk count
 *   RPCCRC_RAGGED_SPLIT  bodies of <= 1 KiB (with their 16-B end pad) four per
 *                        row, the rest one wavefront per body
 * Returns RPCCRC_EINVAL for any other value. */
#define RPCCRC_RAGGED_AUTO 0
#define RPCCRC_RAGGED_ROWS 1
#define RPCCRC_RAGGED_PACKED 2
#define RPCCRC_RAGGED_SPLIT 3
RPCCRC_API int rpc_crc32_set_ragged_path(int path);

/* Human-readable text for a negative return code. */
RPCCRC_API const char *rpc_crc32_strerror(int err);

/* Writes "device=<name> arch=<gcn> cus=<n>" for the current device. */
RPCCRC_API int rpc_crc32_device_info(char *buf, size_t buflen);

/* Device error status of the current device: RPCCRC_OK, or RPCCRC_EIO once a
 * kernel launched by an ASYNCHRONOUS call (device batches, large bodies, frames,
 * the receive ring) has stored into the device's error word -- a bounded wait of
 * the rows kernel's dealing protocol ran out (after 30 s), so CRCs of that launch
 * may be stale.  While it is set, every asynchronous call on the device returns
 * RPCCRC_EIO.  Device calls are asynchronous: check after synchronising the
 * stream.  The synchronous calls (rpc_crc32, rpc_crc32_verify, rpc_crc32_batch,
 * rpc_crc32_verify_batch) report their own launches' errors in their own return
 * (the drop-in calls abort) and are neither affected by nor recorded in it. */
RPCCRC_API int rpc_crc32_device_status(void);

/* Clears the current device's error word so asynchronous calls work again, and
 * returns what rpc_crc32_device_status returned before (RPCCRC_OK or
 * RPCCRC_EIO).  Call it after synchronising every stream whose results are in
 * doubt: outputs of the launch that failed are not repaired. */
RPCCRC_API int rpc_crc32_device_clear_status(void);

/* Stops the resident drop-in service kernel (the one that answers rpc_crc32 /
 * rpc_crc32_verify calls of <= 1 KiB without a launch) on every
 * device this process has used, and waits (up to 200 ms each) until it has left.
 * A device-wide synchronise (hipDeviceSynchronize, torch.cuda.synchronize())
 * otherwise waits for the service: up to ~2 ms after the last drop-in call
 * (INTEGRATION.md 5).  The next drop-in call starts it again.  Call it with no
 * drop-in call in flight: one racing it waits for its answer (up to 2 s) and then
 * launches a kernel instead.  Returns RPCCRC_OK, or RPCCRC_EIO if an instance did
 * not leave in time (it was still queued behind other work; it then runs and
 * serves calls as usual).  Not part of crc.h; the reference has no counterpart. */
RPCCRC_API int rpc_crc32_service_stop(void);

/* Counters of the drop-in service, summed over every device this process has
 * used (no device needed; all zero before the first drop-in call).  A request
 * that gets no answer in 2 s is given up and the call launches a kernel
 * instead; after that, while the device's latest service instance has not
 * started (queued behind other kernels), drop-in calls launch a kernel without
 * posting (`bypassed`), and posted calls wait 2 ms, not 2 s (`fallbacks_short`),
 * until one is answered again.  Not part of crc.h. */
typedef struct rpccrc_service_stats {
  uint64_t services;        /* devices with a drop-in service */
  uint64_t running;         /* of them, with an instance running or queued */
  uint64_t launched;        /* instances launched */
  uint64_t answered;        /* drop-in calls the service answered */
  uint64_t fallbacks_full;  /* requests given up after the full 2-s wait */
  uint64_t fallbacks_short; /* requests given up after the 2-ms wait that follows a give-up */
  uint64_t bypassed;        /* calls that did not post (instance not started after a give-up) */
} rpccrc_service_stats_t;
RPCCRC_API int rpc_crc32_service_stats(rpccrc_service_stats_t *out);

#ifdef __cplusplus
}
#endif
