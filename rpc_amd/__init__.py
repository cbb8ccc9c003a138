"""rpc_amd -- MI355X-native body checksum for KlinLike/RPC.

Python mirror of the reference interface ``crc.h`` (``rpc_crc32`` at crc.h:8,
``rpc_crc32_verify`` at crc.h:11) plus the batched host/device API of
``include/rpccrc.h``.  Every CRC is computed by the HIP kernels in
``rpc_amd/csrc`` through ``rpc_amd/lib/librpccrc.so``; importing this package
fails if that library is missing, and the calls fail (raise or, for the two
drop-in functions, abort in C) if no HIP device is usable.  There is no CPU
implementation here.

Device-buffer functions take torch tensors on the current HIP device (torch is
only plumbing for device memory and streams) and run on torch's current stream
unless ``stream`` (a ``torch.cuda.Stream``) is given.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib, rx_ring
from ._lib import RpcCrcError, check, lib
from .rx_ring import RxRing

__all__ = [
    "RpcCrcError",
    "rpc_crc32",
    "rpc_crc32_verify",
    "crc32_batch",
    "verify_batch",
    "crc32_combine",
    "rpc_crc32_update",
    "crc32_gather",
    "device_batch",
    "device_uniform",
    "device_large",
    "device_gather",
    "frames_verify",
    "frames_stamp",
    "frames_pack",
    "FramePack",
    "frames_unpack",
    "FrameUnpack",
    "frames_carry",
    "FrameCarry",
    "carry_slots",
    "frames_scan",
    "FrameScan",
    "set_scan_path",
    "RxRing",
    "fill_random",
    "stream_read",
    "set_options",
    "set_ragged_path",
    "device_info",
    "device_status",
    "device_clear_status",
    "RPC_HEADER_LEN",
    "RPC_TYPE_DATA",
    "RPC_TYPE_PING",
    "RPC_TYPE_PONG",
    "MAX_BODY_LEN",
    "FRAME_BAD_CRC",
    "FRAME_OK",
    "FRAME_CONTROL",
    "FRAME_TOO_LARGE",
    "FRAME_MALFORMED",
    "FRAME_RECV_ERR",
    "FRAME_NOT_REACHED",
    "FRAME_SKIPPED",
    "TYPE_NONE",
    "CONN_OPEN",
    "CONN_CLOSED",
    "CARRY_ROOM",
    "CARRY_OK",
    "CARRY_CLOSED",
    "CARRY_INVALID",
    "CARRY_NO_ROOM",
    "frames_route",
    "FrameRoute",
    "route_table",
    "RouteTable",
    "ROUTE_NONE",
    "ROUTE_CALL",
    "ROUTE_NOT_FOUND",
    "ROUTE_INVALID",
    "ROUTE_DEFER",
    "ROUTE_RANGE",
    "ROUTE_NO_METHOD",
    "ROUTE_MAX_BODY",
    "ROUTE_MAX_DEPTH",
    "ROUTE_MAX_TOKENS",
    "ROUTE_MAX_METHODS",
    "ROUTE_MAX_METHOD_BYTES",
    "frames_args",
    "FrameArgs",
    "args_schema",
    "ArgsSchema",
    "ARGS_NONE",
    "ARGS_OK",
    "ARGS_INVALID",
    "ARGS_DEFER",
    "ARGS_RANGE",
    "ARGS_BAD_SCHEMA",
    "ARG_I32",
    "ARG_I64",
    "ARG_F64",
    "ARG_BOOL",
    "ARG_STR",
    "ARGS_MAX_PARAMS",
    "ARGS_MAX_SCHEMA_PARAMS",
    "ARGS_MAX_NAME_BYTES",
    "frames_resolve",
    "FrameResolve",
    "RESOLVE_NONE",
    "RESOLVE_MATCHED",
    "RESOLVE_UNKNOWN",
    "RESOLVE_DUPLICATE",
    "RESOLVE_INVALID",
    "RESOLVE_DEFER",
    "RESOLVE_RANGE",
    "RESOLVE_NO_SLOT",
    "RESOLVE_MAX_PENDING",
    "frames_reply",
    "FrameReply",
    "REPLY_NONE",
    "REPLY_RESULT",
    "REPLY_ERROR",
    "REPLY_RAW",
    "REPLY_RANGE",
    "REPLY_NO_ROOM",
    "frames_request",
    "FrameRequest",
    "REQUEST_NONE",
    "REQUEST_CALL",
    "REQUEST_RAW",
    "REQUEST_BAD_METHOD",
    "REQUEST_RANGE",
    "REQUEST_NO_ROOM",
    "frames_values",
    "FrameValues",
    "result_types",
    "VALUES_NONE",
    "VALUES_OK",
    "VALUES_TEXT",
    "VALUES_DEFER",
    "VALUES_RANGE",
    "VALUES_BAD_SCHEMA",
    "VALUES_NO_ROOM",
    "VALUES_MODE_NONE",
    "VALUES_MODE_ENCODE",
    "VALUES_MODE_TEXT",
    "VALUES_FORM_RESULT",
    "VALUES_FORM_PARAMS",
]

# reference rpc.h:11-17
RPC_TYPE_DATA = 0
RPC_TYPE_PING = 1
RPC_TYPE_PONG = 2
RPC_HEADER_LEN = 12
MAX_BODY_LEN = 1024

# frame verdicts and flags (include/rpccrc.h RPC_FRAME_* / RPC_FRAMES_*)
FRAME_BAD_CRC = 0
FRAME_OK = 1
FRAME_CONTROL = 2
FRAME_TOO_LARGE = 3
FRAME_MALFORMED = 4
FRAME_RECV_ERR = 5  # client role, body_len 0: rpc_async.c:330-349 drops the connection (RPC_RECV_ERR)
FRAME_NOT_REACHED = 6  # frames_scan(verify=True): behind a frame that closed its connection
FRAME_SKIPPED = 7  # frames_pack: the caller asked for no frame here (TYPE_NONE)
TYPE_NONE = 0xFFFF  # frames_pack: a type value meaning "emit nothing for this entry"
CONN_OPEN = 0
CONN_CLOSED = 1
FRAMES_SERVER = 0x1
FRAMES_CLIENT = 0x2
FRAMES_LIFT_CAP = 0x4
# frames_carry (include/rpccrc.h RPC_FRAMES_CARRY_ROOM / RPC_CARRY_*)
CARRY_ROOM = 1040  # >= 12 + MAX_BODY_LEN - 1, a multiple of 16: any tail with the cap in force
CARRY_OK = 0
CARRY_CLOSED = 1
CARRY_INVALID = 2
CARRY_NO_ROOM = 3
# frames_route (include/rpccrc.h RPC_ROUTE_*)
ROUTE_NONE = 0
ROUTE_CALL = 1
ROUTE_NOT_FOUND = 2
ROUTE_INVALID = 3
ROUTE_DEFER = 4
ROUTE_RANGE = 5
ROUTE_NO_METHOD = 0xFFFF
ROUTE_MAX_BODY = 1024
ROUTE_MAX_DEPTH = 32
ROUTE_MAX_TOKENS = 256
ROUTE_MAX_METHODS = 256
ROUTE_MAX_METHOD_BYTES = 4096
# frames_args (include/rpccrc.h RPC_ARGS_* / RPC_ARG_*)
ARGS_NONE = 0
ARGS_OK = 1
ARGS_INVALID = 2
ARGS_DEFER = 3
ARGS_RANGE = 4
ARGS_BAD_SCHEMA = 5
ARG_I32 = 0
ARG_I64 = 1
ARG_F64 = 2
ARG_BOOL = 3
ARG_STR = 4
ARGS_MAX_PARAMS = 8
ARGS_MAX_SCHEMA_PARAMS = 1024
ARGS_MAX_NAME_BYTES = 4096
# frames_resolve (include/rpccrc.h RPC_RESOLVE_*)
RESOLVE_NONE = 0
RESOLVE_MATCHED = 1
RESOLVE_UNKNOWN = 2
RESOLVE_DUPLICATE = 3
RESOLVE_INVALID = 4
RESOLVE_DEFER = 5
RESOLVE_RANGE = 6
RESOLVE_NO_SLOT = 0xFFFFFFFF
RESOLVE_MAX_PENDING = 1 << 24
# frames_reply (include/rpccrc.h RPC_REPLY_*)
REPLY_NONE = 0
REPLY_RESULT = 1
REPLY_ERROR = 2
REPLY_RAW = 3
REPLY_RANGE = 4
REPLY_NO_ROOM = 5
# frames_request (include/rpccrc.h RPC_REQUEST_*)
REQUEST_NONE = 0
REQUEST_CALL = 1
REQUEST_RAW = 2
REQUEST_BAD_METHOD = 3
REQUEST_RANGE = 4
REQUEST_NO_ROOM = 5
# frames_values (include/rpccrc.h RPC_VALUES_*)
VALUES_NONE = 0
VALUES_OK = 1
VALUES_TEXT = 2
VALUES_DEFER = 3
VALUES_RANGE = 4
VALUES_BAD_SCHEMA = 5
VALUES_NO_ROOM = 6
VALUES_MODE_NONE = 0
VALUES_MODE_ENCODE = 1
VALUES_MODE_TEXT = 2
VALUES_FORM_RESULT = 0
VALUES_FORM_PARAMS = 1


def _as_buffer(data) -> tuple[Optional[int], int, object]:
    """(address, nbytes, keepalive) for bytes-like / numpy input; None -> NULL."""
    if data is None:
        return None, 0, None
    if isinstance(data, np.ndarray):
        arr = np.ascontiguousarray(data)
        return arr.ctypes.data, arr.nbytes, arr
    mv = memoryview(data).cast("B")
    if mv.readonly:
        buf = ctypes.create_string_buffer(bytes(mv), len(mv))
        return ctypes.addressof(buf), len(mv), buf
    arr = np.frombuffer(mv, dtype=np.uint8)
    return arr.ctypes.data, arr.nbytes, arr


# ---- drop-in ---------------------------------------------------------------

def rpc_crc32(data, length: Optional[int] = None) -> int:
    """rpc_crc32(data, len) -- reference crc.c:4-9.  ``length`` defaults to len(data)."""
    addr, n, keep = _as_buffer(data)
    if length is None:
        length = n
    r = _lib.rpc_crc32(addr, length)
    del keep
    return int(r)


def rpc_crc32_verify(data, expected_crc: int, length: Optional[int] = None) -> bool:
    """rpc_crc32_verify(data, len, expected) -- reference crc.c:11-14."""
    addr, n, keep = _as_buffer(data)
    if length is None:
        length = n
    r = _lib.rpc_crc32_verify(addr, length, expected_crc & 0xFFFFFFFF)
    del keep
    return bool(r)


def rpc_crc32_update(crc: int, data, length: Optional[int] = None) -> int:
    """zlib's running form crc32(crc, data, len); ``data`` None -> 0.  ``length`` defaults to len(data)."""
    addr, n, keep = _as_buffer(data)
    if length is None:
        length = n
    r = _lib.rpc_crc32_update(crc & 0xFFFFFFFF, addr, length)
    del keep
    return int(r)


def crc32_combine(crc1: int, crc2: int, len2: int) -> int:
    """zlib crc32_combine semantics (zlib.h:1750)."""
    return int(_lib.rpc_crc32_combine(crc1 & 0xFFFFFFFF, crc2 & 0xFFFFFFFF, len2))


# ---- batched, host buffers ---------------------------------------------------

def crc32_batch(buf, offsets: Sequence[int], lengths: Sequence[int]) -> np.ndarray:
    """CRC of every body ``buf[offsets[i] : offsets[i] + lengths[i]]`` (host memory)."""
    addr, _, keep = _as_buffer(buf)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lengths, dtype=np.uint32)
    if off.shape != ln.shape:
        raise ValueError("offsets and lengths differ in length")
    out = np.empty(off.shape[0], dtype=np.uint32)
    check(_lib.rpc_crc32_batch(addr, off.ctypes.data, ln.ctypes.data, off.shape[0], out.ctypes.data, 0),
          "rpc_crc32_batch")
    del keep
    return out


def verify_batch(buf, offsets, lengths, expected) -> tuple[int, np.ndarray]:
    """(mismatch count, ok[] uint8) -- batched rpc_crc32_verify."""
    addr, _, keep = _as_buffer(buf)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lengths, dtype=np.uint32)
    exp = np.ascontiguousarray(expected, dtype=np.uint32)
    ok = np.empty(off.shape[0], dtype=np.uint8)
    bad = check(_lib.rpc_crc32_verify_batch(addr, off.ctypes.data, ln.ctypes.data, exp.ctypes.data,
                                            off.shape[0], ok.ctypes.data), "rpc_crc32_verify_batch")
    del keep
    return int(bad), ok


def crc32_gather(buf, seg_offsets: Sequence[int], seg_lengths: Sequence[int], seg_first: Sequence[int],
                 seed: Optional[Sequence[int]] = None) -> np.ndarray:
    """CRC of every body given as a segment list over host memory: body i is the
    concatenation of ``buf[seg_offsets[s] : seg_offsets[s] + seg_lengths[s]]`` for
    s = seg_first[i] .. seg_first[i+1]-1; with ``seed`` the bodies continue those running CRCs."""
    addr, _, keep = _as_buffer(buf)
    off = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(seg_lengths, dtype=np.uint32)
    first = np.ascontiguousarray(seg_first, dtype=np.uint64)
    if off.shape != ln.shape:
        raise ValueError("seg_offsets and seg_lengths differ in length")
    if first.shape[0] < 1:
        raise ValueError("seg_first needs n + 1 entries")
    n = first.shape[0] - 1
    sd = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint32)
    if sd is not None and sd.shape[0] != n:
        raise ValueError("seed and seg_first differ in length")
    out = np.empty(n, dtype=np.uint32)
    check(_lib.rpc_crc32_batch_gather(addr, off.ctypes.data, ln.ctypes.data, off.shape[0], first.ctypes.data, n,
                                      None if sd is None else sd.ctypes.data, out.ctypes.data, 0),
          "rpc_crc32_batch_gather")
    del keep
    return out


# ---- batched, device buffers (torch tensors as HBM plumbing) -----------------

def _torch():
    if _lib.torch is None:
        raise RuntimeError("device-buffer calls need torch (ROCm) for device memory")
    return _lib.torch


# The stream contract of every device-buffer call below.  ``stream=None`` is torch's current
# stream.  ``stream=s`` alone is enough: every launch, memset and copy of the call -- the
# library's and the wrapper's own, a read-back included -- goes to ``s`` and to no other stream,
# whatever torch's current stream is and however busy it is; the wrapper allocates (``t.empty``,
# no fill) and does nothing else on the device.  What the caller owes: the inputs are ready in
# ``s``'s order, and the tensors handed in and returned stay alive until ``s`` has run the call
# (torch's allocator knows the current stream only).  ``s`` is a ``torch.cuda.Stream`` or any
# object whose ``cuda_stream`` is a ``hipStream_t``; the variants that read a count or a total
# back (``out=None``; ``frames_scan`` unless ``read_count=False``) copy it on ``s`` and wait
# for ``s`` alone.

def _stream_handle(stream) -> int:
    t = _torch()
    s = stream if stream is not None else t.cuda.current_stream()
    return int(s.cuda_stream)


def _read_back(x, stream) -> int:
    """x[0] on the host, copied on the call's stream: that stream is synchronised, no other."""
    t = _torch()
    if stream is None:
        return int(x.cpu()[0])
    own = stream if isinstance(stream, t.cuda.Stream) else t.cuda.ExternalStream(int(stream.cuda_stream),
                                                                                 device=x.device)
    with t.cuda.stream(own):
        return int(x.cpu()[0])


def _dev_u32_out(n: int, device, out):
    t = _torch()
    if out is None:
        out = t.empty(n, dtype=t.int32, device=device)
    if out.numel() < n or out.element_size() != 4 or not out.is_contiguous():
        raise ValueError("out must be a contiguous 4-byte tensor with >= n elements")
    return out


def device_batch(base, offsets, lengths, out=None, stream=None, max_len: int = 0):
    """Ragged batch over a device byte tensor; offsets int64/uint64, lengths int32/uint32 device tensors.
    ``max_len``: an upper bound on the lengths the caller knows (0 = none); below 256 KiB the
    big-body route's passes are skipped (rpc_crc32_device_batch_bounded; results never depend on it)."""
    n = offsets.numel()
    if lengths.numel() != n:
        raise ValueError("offsets and lengths differ in length")
    out = _dev_u32_out(n, base.device, out)
    if _lib.rpc_crc32_device_batch_bounded is None:  # an older build under A/B (tools/ab_lib.sh)
        check(_lib.rpc_crc32_device_batch(base.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n,
                                          out.data_ptr(), _stream_handle(stream)), "rpc_crc32_device_batch")
        return out
    check(_lib.rpc_crc32_device_batch_bounded(base.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n,
                                              int(max_len) & 0xFFFFFFFF, out.data_ptr(), _stream_handle(stream)),
          "rpc_crc32_device_batch_bounded")
    return out


def device_uniform(base, n: int, body_len: int, stride: Optional[int] = None, out=None, stream=None):
    """Equal-length batch: body i = base[i*stride : i*stride + body_len]."""
    if stride is None:
        stride = body_len
    if n and (n - 1) * stride + body_len > base.numel() * base.element_size():
        raise ValueError("bodies exceed the base tensor")
    out = _dev_u32_out(n, base.device, out)
    check(_lib.rpc_crc32_device_uniform(base.data_ptr(), n, body_len, stride, out.data_ptr(),
                                        _stream_handle(stream)), "rpc_crc32_device_uniform")
    return out


def device_large(base, offsets: Iterable[int], lengths: Iterable[int], chunk: int = 0, out=None, stream=None):
    """Large bodies (host-known offsets/lengths, device data), chunked + GF(2)-combined."""
    off = np.ascontiguousarray(list(offsets), dtype=np.uint64)
    ln = np.ascontiguousarray(list(lengths), dtype=np.uint64)
    n = off.shape[0]
    out = _dev_u32_out(n, base.device, out)
    check(_lib.rpc_crc32_device_large(base.data_ptr(), off.ctypes.data, ln.ctypes.data, n, out.data_ptr(),
                                      chunk, _stream_handle(stream)), "rpc_crc32_device_large")
    return out


def device_gather(base, seg_offsets, seg_lengths, seg_first, seed=None, out=None, stream=None,
                  max_seg_len: int = 0):
    """Bodies given as segment lists over a device byte tensor (rpc_crc32_device_gather).

    Segment s = base[seg_offsets[s] : + seg_lengths[s]]; body i is the concatenation of
    segments seg_first[i] .. seg_first[i+1]-1 (CSR, int64/uint64 device tensor of n + 1
    entries).  ``seed`` (4-byte device tensor, n entries): running CRCs the bodies continue
    (zlib crc32(seed, body)); ``out`` may be the same tensor.  ``max_seg_len``: an upper
    bound on the segment lengths (0 = none), as device_batch's ``max_len``.  With no
    segments at all ``base``, ``seg_offsets`` and ``seg_lengths`` may be None."""
    n = seg_first.numel() - 1
    if n < 0:
        raise ValueError("seg_first needs n + 1 entries")
    nseg = 0 if seg_offsets is None else seg_offsets.numel()
    if (0 if seg_lengths is None else seg_lengths.numel()) != nseg:
        raise ValueError("seg_offsets and seg_lengths differ in length")
    if nseg and base is None:
        raise ValueError("segments need a base tensor")
    if seed is not None and (seed.numel() < n or seed.element_size() != 4 or not seed.is_contiguous()):
        raise ValueError("seed must be a contiguous 4-byte tensor with >= n elements")
    out = _dev_u32_out(n, seg_first.device, out)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(_lib.rpc_crc32_device_gather(ptr(base), ptr(seg_offsets), ptr(seg_lengths), nseg,
                                       int(max_seg_len) & 0xFFFFFFFF, seg_first.data_ptr(), n, ptr(seed),
                                       out.data_ptr(), _stream_handle(stream)), "rpc_crc32_device_gather")
    return out


def _frames_flags(role: str, lift_cap: bool) -> int:
    try:
        f = {"server": FRAMES_SERVER, "client": FRAMES_CLIENT}[role]
    except KeyError:
        raise ValueError("role must be 'server' (PING is control) or 'client' (PONG is control)") from None
    return f | (FRAMES_LIFT_CAP if lift_cap else 0)


def frames_verify(stream_buf, frame_offsets, role: str = "server", lift_cap: bool = False, stream_bytes=None,
                  crc_out=None, stream=None):
    """Verify n wire frames (rpc.h header + body) in a device byte tensor.

    Returns (verdict uint8 tensor of FRAME_*, crc int32 tensor).  ``role`` picks the
    heartbeat that is a control frame: "server" -> PING (rpc_server_main.c:172),
    "client" -> PONG (rpc_async.c:303).  Without ``lift_cap`` a data frame whose
    body_len exceeds MAX_BODY_LEN is FRAME_TOO_LARGE (rpc_server_main.c:189)."""
    t = _torch()
    n = frame_offsets.numel()
    nbytes = stream_buf.numel() * stream_buf.element_size() if stream_bytes is None else int(stream_bytes)
    verdict = t.empty(n, dtype=t.uint8, device=stream_buf.device)
    crc = _dev_u32_out(n, stream_buf.device, crc_out)
    check(_lib.rpc_frames_verify_device(stream_buf.data_ptr(), nbytes, frame_offsets.data_ptr(), n,
                                        _frames_flags(role, lift_cap), verdict.data_ptr(), crc.data_ptr(),
                                        _stream_handle(stream)), "rpc_frames_verify_device")
    return verdict, crc


def frames_stamp(stream_buf, frame_offsets, body_lens, version: int = 1, type_: int = RPC_TYPE_DATA,
                 lift_cap: bool = False, stream_bytes=None, stream=None):
    """Write rpc.h headers (BE version/type/body_len/crc32) in front of device-resident
    bodies; returns the per-frame verdict (FRAME_OK stamped, FRAME_TOO_LARGE /
    FRAME_MALFORMED not stamped)."""
    t = _torch()
    n = frame_offsets.numel()
    nbytes = stream_buf.numel() * stream_buf.element_size() if stream_bytes is None else int(stream_bytes)
    verdict = t.empty(n, dtype=t.uint8, device=stream_buf.device)
    check(_lib.rpc_frames_stamp_device(stream_buf.data_ptr(), nbytes, frame_offsets.data_ptr(), body_lens.data_ptr(),
                                       n, version, type_, FRAMES_LIFT_CAP if lift_cap else 0, verdict.data_ptr(),
                                       _stream_handle(stream)), "rpc_frames_stamp_device")
    return verdict


class FramePack(NamedTuple):
    """What frames_pack returns (device tensors; ``total`` is the host-side byte count, or with
    a caller's ``out`` -- nothing is read back then -- a one-element int64 device tensor)."""
    stream: object            # uint8: the wire bytes; connection c is stream[conn_bytes_first[c] : conn_bytes_first[c + 1]]
    offsets: object           # int64 [n]: where each entry's frame starts (entries of size 0 share the next one's)
    verdict: object           # uint8 [n]: FRAME_OK / _CONTROL / _SKIPPED / _TOO_LARGE / _MALFORMED
    crc: object               # int32 [n]: the CRC stamped (0 for everything that is no data frame)
    conn_bytes_first: object  # int64 [nconn + 1], or None without conn_first
    total: object             # bytes of all frames, whether they fitted or not


def frames_pack(bodies, body_offsets, body_lens, types=None, version: int = 1, type_: int = RPC_TYPE_DATA,
                versions=None, conn_first=None, lift_cap: bool = False, out=None, stream=None):
    """Build wire streams from bodies (rpc_frames_pack_device): the mirror image of frames_scan.

    Entry i is the body ``bodies[body_offsets[i] : + body_lens[i]]`` (uint8 device tensor;
    int64/uint64 and int32/uint32 device tensors) with type ``types[i]`` and version
    ``versions[i]`` (int16/uint16 device tensors), or ``type_`` / ``version`` for all.  A type
    of TYPE_NONE emits nothing (FRAME_SKIPPED), PING / PONG a bare 12-byte heartbeat
    (FRAME_CONTROL; offset and length are not looked at), anything else a data frame: header,
    then the body.  ``conn_first`` (int64 [nconn + 1]) is a
    CSR over the entries, as frames_scan returns it; connection c's bytes to send are
    ``stream[conn_bytes_first[c] : conn_bytes_first[c + 1]]``.

    ``out=None`` makes the layout-only call first, reads the total (one synchronisation, as
    frames_scan does for its count), allocates exactly and packs.  With ``out`` (a contiguous
    uint8 device tensor that does not overlap ``bodies``) nothing is read back: frames that do
    not end inside it are FRAME_MALFORMED and not written, and ``total`` stays on the device."""
    t = _torch()
    if body_offsets is not None:
        n = body_offsets.numel()
    elif types is not None:
        n = types.numel()
    else:
        raise ValueError("the number of entries comes from body_offsets or types")
    for name, x, size in (("body_lens", body_lens, 4), ("types", types, 2), ("versions", versions, 2),
                          ("body_offsets", body_offsets, 8)):
        if x is not None and (x.numel() != n or x.element_size() != size or not x.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if conn_first is not None and (conn_first.numel() < 1 or conn_first.element_size() != 8):
        raise ValueError("conn_first needs nconn + 1 8-byte entries")
    if out is not None and (out.element_size() != 1 or not out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor")
    dev = next(x for x in (bodies, body_offsets, types, out) if x is not None).device
    nconn = 0 if conn_first is None else conn_first.numel() - 1
    nbytes = 0 if bodies is None else bodies.numel() * bodies.element_size()
    flags = FRAMES_LIFT_CAP if lift_cap else 0
    sh = _stream_handle(stream)
    offsets = t.empty(n, dtype=t.int64, device=dev)
    verdict = t.empty(n, dtype=t.uint8, device=dev)
    crc = t.empty(n, dtype=t.int32, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    def run(dst, layout_only):
        check(_lib.rpc_frames_pack_device(ptr(bodies), nbytes if ptr(bodies) else 0, ptr(body_offsets), ptr(body_lens), n,
                                          ptr(types), int(type_) & 0xFFFF, ptr(versions), int(version) & 0xFFFF,
                                          None if conn_first is None else conn_first.data_ptr(), nconn, flags,
                                          ptr(dst), 0 if dst is None else dst.numel(),
                                          None if layout_only else ptr(offsets), None if layout_only else ptr(verdict),
                                          None if layout_only else ptr(crc), None if layout_only else ptr(cbf),
                                          total.data_ptr(), sh), "rpc_frames_pack_device")

    if out is not None:
        run(out, False)
        return FramePack(out, offsets, verdict, crc, cbf, total)
    run(None, True)  # layout only: the total (read on the call's stream: one synchronisation)
    nb = _read_back(total, stream)
    out = t.empty(nb, dtype=t.uint8, device=dev)
    run(out, False)
    return FramePack(out, offsets, verdict, crc, cbf, nb)


class FrameUnpack(NamedTuple):
    """What frames_unpack returns (device tensors; ``total`` is the host-side byte count, or with
    a caller's ``out`` -- nothing is read back then -- a one-element int64 device tensor)."""
    bodies: object            # uint8: the delivered bodies back to back, each followed by a 0 byte with nul
    body_offsets: object      # int64 [n]: where each entry's body starts (entries of size 0 share the next one's)
    body_lens: object         # int32 [n]: body_len of a delivered entry, else 0
    reply_types: object       # int16 [n]: frames_pack's types: DATA / PONG / TYPE_NONE
    versions: object          # int16 [n]: the request's version, which the reply echoes
    verdict: object           # uint8 [n]: FRAME_OK (delivered) / _CONTROL / _MALFORMED / the input verdict
    conn_bytes_first: object  # int64 [nconn + 1], or None without conn_first
    total: object             # bytes of all delivered entries, whether they fitted or not


def frames_unpack(stream_buf, frame_offsets, verdict, role: str = "server", lift_cap: bool = False, nul: bool = True,
                  conn_first=None, out=None, stream=None, stream_bytes=None):
    """Verified bodies as C strings and the reply plan (rpc_frames_unpack_device): what sits
    between ``frames_scan(verify=True)`` and the dispatcher, and what feeds ``frames_pack``.

    ``frame_offsets`` / ``verdict`` (int64/uint64 and uint8 device tensors, n entries; the padded
    arrays of a scan as they are) say where the frames lie in ``stream_buf`` and what the verify
    found.  Every FRAME_OK entry whose header agrees is delivered: its body is copied to
    ``bodies[body_offsets[i] : + body_lens[i]]`` and, with ``nul``, followed by one 0 byte (the
    string the reference's dispatcher takes).  A heartbeat (FRAME_CONTROL) delivers nothing
    and gets reply type PONG at a server, TYPE_NONE at a client; everything else gets TYPE_NONE.
    ``bodies, body_offsets, body_lens, reply_types, versions`` and the same ``conn_first`` go to
    ``frames_pack`` unchanged.

    ``out=None`` makes the layout-only call first, reads the total (one synchronisation),
    allocates exactly and unpacks.  With ``out`` (a contiguous uint8 device tensor that does
    not overlap ``stream_buf``) nothing is read back: entries that do not end inside it are
    FRAME_MALFORMED / TYPE_NONE and not written, and ``total`` stays on the device."""
    t = _torch()
    n = frame_offsets.numel()
    for name, x, size in (("frame_offsets", frame_offsets, 8), ("verdict", verdict, 1)):
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if conn_first is not None and (conn_first.numel() < 1 or conn_first.element_size() != 8):
        raise ValueError("conn_first needs nconn + 1 8-byte entries")
    if out is not None and (out.element_size() != 1 or not out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor")
    dev = stream_buf.device
    nconn = 0 if conn_first is None else conn_first.numel() - 1
    nbytes = stream_buf.numel() * stream_buf.element_size() if stream_bytes is None else int(stream_bytes)
    flags = _frames_flags(role, lift_cap)
    sh = _stream_handle(stream)
    body_offsets = t.empty(n, dtype=t.int64, device=dev)
    body_lens = t.empty(n, dtype=t.int32, device=dev)
    reply_types = t.empty(n, dtype=t.int16, device=dev)
    versions = t.empty(n, dtype=t.int16, device=dev)
    verdict_out = t.empty(n, dtype=t.uint8, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    def run(dst, layout_only):
        outs = (None,) * 6 if layout_only else (ptr(body_offsets), ptr(body_lens), ptr(reply_types), ptr(versions),
                                                ptr(verdict_out), ptr(cbf))
        check(_lib.rpc_frames_unpack_device(ptr(stream_buf), nbytes if ptr(stream_buf) else 0, ptr(frame_offsets),
                                            ptr(verdict), n, None if conn_first is None else conn_first.data_ptr(),
                                            nconn, flags, 1 if nul else 0, ptr(dst), 0 if dst is None else dst.numel(),
                                            *outs, total.data_ptr(), sh), "rpc_frames_unpack_device")

    if out is not None:
        run(out, False)
        return FrameUnpack(out, body_offsets, body_lens, reply_types, versions, verdict_out, cbf, total)
    run(None, True)  # layout only: the total (read on the call's stream: one synchronisation)
    nb = _read_back(total, stream)
    out = t.empty(nb, dtype=t.uint8, device=dev)
    run(out, False)
    return FrameUnpack(out, body_offsets, body_lens, reply_types, versions, verdict_out, cbf, nb)


class FrameCarry(NamedTuple):
    """What frames_carry returns (device tensors; nothing is read back)."""
    next_offsets: object  # int64 [nconn]: the next round's connections in next_buf ...
    next_lengths: object  # int64 [nconn]: ... tail + new bytes (0 / 0 unless status is CARRY_OK)
    status: object        # uint8 [nconn]: CARRY_OK / _CLOSED / _INVALID / _NO_ROOM
    carried: object       # int64 [1]: the sum of the tails written


def carry_slots(new_lengths, room: int = CARRY_ROOM, align: int = 16):
    """Where a round's new bytes go in the next buffer: the connections back to back, ``room``
    bytes of headroom in front of each connection's new bytes, each start a multiple of
    ``align``.  Returns ``(next_at, total_bytes)``: an int64 array for ``frames_carry`` and the
    size of the buffer -- a host fills one pinned staging buffer of that size at these positions
    and does one H2D per round."""
    nl = np.asarray(new_lengths, dtype=np.int64)
    if nl.ndim != 1 or (nl < 0).any() or room < 0 or align < 1:
        raise ValueError("new_lengths must be a list of non-negative lengths, room >= 0, align >= 1")
    at = np.empty(nl.size, dtype=np.int64)
    cur = 0
    for c, n in enumerate(nl.tolist()):
        at[c] = -(-(cur + room) // align) * align
        cur = int(at[c]) + n
    return at, cur


def frames_carry(stream_buf, conn_offsets, conn_lengths, consumed, state, next_buf, next_at, room: int = CARRY_ROOM,
                 new_lengths=None, stream=None):
    """Partial frames join the next read (rpc_frames_carry_device): what sits between two rounds.

    ``conn_offsets`` / ``conn_lengths`` are the connections a ``frames_scan`` walked in
    ``stream_buf``, ``consumed`` and ``state`` what it returned (``state=None``: every connection
    is open).  ``next_buf`` is the next round's buffer, a contiguous uint8 device tensor that does
    not overlap ``stream_buf``; connection c's ``new_lengths[c]`` new bytes begin at
    ``next_at[c]`` with at least ``room`` free bytes in front of them (``carry_slots``).  Each
    open connection's unconsumed tail is copied so that it ends at ``next_at[c]``;
    ``next_offsets`` / ``next_lengths`` are the connections to scan in ``next_buf``.  The new
    bytes are never looked at: their H2D may still be in flight on another stream.  All index
    tensors are int64/uint64 device tensors of nconn entries, ``state`` uint8."""
    t = _torch()
    nconn = conn_offsets.numel()
    for name, x, size, opt in (("conn_offsets", conn_offsets, 8, False), ("conn_lengths", conn_lengths, 8, False),
                               ("consumed", consumed, 8, False), ("state", state, 1, True),
                               ("next_at", next_at, 8, False), ("new_lengths", new_lengths, 8, True)):
        if x is None and opt:
            continue
        if x.numel() != nconn or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with nconn = {nconn} elements")
    for name, x in (("stream_buf", stream_buf), ("next_buf", next_buf)):
        if x.element_size() != 1 or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint8 tensor")
    if room < 0:
        raise ValueError("room must not be negative")
    dev = next_buf.device
    next_offsets = t.empty(nconn, dtype=t.int64, device=dev)
    next_lengths = t.empty(nconn, dtype=t.int64, device=dev)
    status = t.empty(nconn, dtype=t.uint8, device=dev)
    carried = t.empty(1, dtype=t.int64, device=dev)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    check(_lib.rpc_frames_carry_device(ptr(stream_buf), stream_buf.numel() if ptr(stream_buf) else 0, ptr(conn_offsets),
                                       ptr(conn_lengths), ptr(consumed), ptr(state), nconn, ptr(next_buf),
                                       next_buf.numel() if ptr(next_buf) else 0, ptr(next_at), int(room),
                                       ptr(new_lengths), ptr(next_offsets), ptr(next_lengths), ptr(status),
                                       carried.data_ptr(), _stream_handle(stream)), "rpc_frames_carry_device")
    return FrameCarry(next_offsets, next_lengths, status, carried)


class RouteTable(NamedTuple):
    """A server's method table on the device (route_table)."""
    names: object    # uint8: the names back to back
    offsets: object  # int32 [nmethods + 1]: name m is names[offsets[m] : offsets[m + 1]]
    nmethods: int


def route_table(names, device=None) -> RouteTable:
    """The two table tensors of frames_route from ``bytes`` / ``str`` method names (at most
    ROUTE_MAX_METHODS names and ROUTE_MAX_METHOD_BYTES bytes), in the order that gives a
    CALL's method index."""
    t = _torch()
    raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    if len(raw) > ROUTE_MAX_METHODS or sum(map(len, raw)) > ROUTE_MAX_METHOD_BYTES:
        raise ValueError(f"at most {ROUTE_MAX_METHODS} names and {ROUTE_MAX_METHOD_BYTES} bytes of names")
    offs = np.zeros(len(raw) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(r) for r in raw], dtype=np.int64)
    dev = "cuda" if device is None else device
    return RouteTable(t.from_numpy(np.frombuffer(b"".join(raw), dtype=np.uint8).copy()).to(dev),
                      t.from_numpy(offs).to(dev), len(raw))


class FrameRoute(NamedTuple):
    """What frames_route returns (device tensors; nothing is read back)."""
    kind: object         # uint8 [n]: ROUTE_NONE / _CALL / _NOT_FOUND / _INVALID / _DEFER / _RANGE
    method: object       # int16 [n]: the table index of a CALL, else ROUTE_NO_METHOD (view as uint16)
    id: object           # int32 [n]: the request's id (view as uint32)
    params_off: object   # int32 [n]: a CALL's `params` value, relative to the body's first byte ...
    params_len: object   # int32 [n]: ... 0 / 0 when the request has none
    order: object        # int32 [n], or None: entry indices group by group; order[:group_first[-1]] is written
    group_first: object  # int32 [nmethods + 4], or None: CSR over CALL by method, NOT_FOUND, INVALID, DEFER


def frames_route(bodies, body_offsets, body_lens, table: RouteTable, reply_types=None, group: bool = True,
                 stream=None) -> FrameRoute:
    """The JSON-RPC envelope of every delivered body (rpc_frames_route_device): what sits between
    ``frames_unpack`` and the handlers.

    ``bodies, body_offsets, body_lens, reply_types`` are ``frames_unpack``'s outputs unchanged
    (``reply_types=None``: every entry is DATA).  Per entry: the kind, the index of the method
    in ``table`` (``route_table``), the id, and where the first top-level ``params`` value lies
    in the body.  Bodies outside the strict subset of include/rpccrc.h read ROUTE_DEFER: parse
    those on the host as before.  With ``group`` the entries are also listed group by group
    (CALL by method index, then NOT_FOUND, INVALID, DEFER; a stable sort), so that a handler
    runs once over ``order[group_first[m] : group_first[m + 1]]``."""
    t = _torch()
    n = body_offsets.numel()
    for name, x, size, opt in (("body_offsets", body_offsets, 8, False), ("body_lens", body_lens, 4, False),
                               ("reply_types", reply_types, 2, True)):
        if x is None and opt:
            continue
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if bodies.element_size() != 1 or not bodies.is_contiguous():
        raise ValueError("bodies must be a contiguous uint8 tensor")
    if table.offsets.numel() != table.nmethods + 1 or table.offsets.element_size() != 4:
        raise ValueError("table.offsets needs nmethods + 1 4-byte entries")
    dev = bodies.device
    kind = t.empty(n, dtype=t.uint8, device=dev)
    method = t.empty(n, dtype=t.int16, device=dev)
    rid = t.empty(n, dtype=t.int32, device=dev)
    poff = t.empty(n, dtype=t.int32, device=dev)
    plen = t.empty(n, dtype=t.int32, device=dev)
    order = t.empty(max(n, 1), dtype=t.int32, device=dev) if group else None  # (never a null pointer)
    first = t.empty(table.nmethods + 4, dtype=t.int32, device=dev) if group else None

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    check(_lib.rpc_frames_route_device(ptr(bodies), bodies.numel() if ptr(bodies) else 0, ptr(body_offsets),
                                       ptr(body_lens), ptr(reply_types), n, ptr(table.names), table.names.numel(),
                                       ptr(table.offsets), table.nmethods, ptr(kind), ptr(method), ptr(rid), ptr(poff),
                                       ptr(plen), order.data_ptr() if group else None,
                                       first.data_ptr() if group else None, _stream_handle(stream)),
          "rpc_frames_route_device")
    return FrameRoute(kind, method, rid, poff, plen, order[:n] if group else None, first)


class ArgsSchema(NamedTuple):
    """A server's parameter schema on the device (args_schema)."""
    first: object     # int32 [nmethods + 1]: method m declares parameters first[m] : first[m + 1]
    types: object     # uint8 [nparams]: ARG_I32 / _I64 / _F64 / _BOOL / _STR
    name_off: object  # int32 [nparams + 1]: parameter p is called names[name_off[p] : name_off[p + 1]]
    names: object     # uint8: the parameter names back to back
    nmethods: int
    nparams: int
    width: int        # the most parameters any method declares (at least 1)


_ARG_TYPES = {"i32": ARG_I32, "i64": ARG_I64, "double": ARG_F64, "f64": ARG_F64, "bool": ARG_BOOL, "string": ARG_STR,
              "str": ARG_STR}


def args_schema(methods, device=None) -> ArgsSchema:
    """The schema tensors of frames_args from ``[(name, [(param, type), ...]), ...]`` in the order
    of ``route_table`` (one list builds both: ``route_table(m for m, _ in methods)``).  A type is
    an ``ARG_*`` constant or one of the IDL's names: i32, i64, double, bool, string."""
    t = _torch()
    first, types, noff, names = [0], [], [0], bytearray()
    for _, params in methods:
        if len(params) > ARGS_MAX_PARAMS:
            raise ValueError(f"at most {ARGS_MAX_PARAMS} parameters per method")
        for pname, ptype in params:
            types.append(_ARG_TYPES[ptype] if isinstance(ptype, str) else int(ptype))
            names += pname.encode() if isinstance(pname, str) else bytes(pname)
            noff.append(len(names))
        first.append(len(types))
    if len(first) - 1 > ROUTE_MAX_METHODS or len(types) > ARGS_MAX_SCHEMA_PARAMS or len(names) > ARGS_MAX_NAME_BYTES:
        raise ValueError(f"at most {ROUTE_MAX_METHODS} methods, {ARGS_MAX_SCHEMA_PARAMS} parameters and "
                         f"{ARGS_MAX_NAME_BYTES} bytes of names")
    dev = "cuda" if device is None else device
    width = max([1] + [b - a for a, b in zip(first, first[1:])])
    return ArgsSchema(t.tensor(first, dtype=t.int32).to(dev), t.tensor(types, dtype=t.uint8).to(dev),
                      t.tensor(noff, dtype=t.int32).to(dev), t.tensor(list(names), dtype=t.uint8).to(dev),
                      len(first) - 1, len(types), width)


class FrameArgs(NamedTuple):
    """What frames_args returns (device tensors; nothing is read back)."""
    status: object        # uint8 [n]: ARGS_NONE / _OK / _INVALID / _DEFER / _RANGE / _BAD_SCHEMA
    reply_status: object  # int32 [n]: 0, -32602 (INVALID) or -32603: frames_reply's ``status``
    slots: object         # int64 [width, n]: slots[k] is parameter k's column (F64: .view(torch.float64))


def frames_args(bodies, body_offsets, body_lens, route: FrameRoute, schema: ArgsSchema, width: Optional[int] = None,
                stream=None) -> FrameArgs:
    """The declared parameters of every routed request as typed 64-bit slots
    (rpc_frames_args_device): what sits between ``frames_route`` and the handlers.

    ``bodies, body_offsets, body_lens`` are ``frames_unpack``'s outputs and ``route`` is
    ``frames_route``'s, all unchanged; ``schema`` (``args_schema``) lists each method's
    parameters in the order of the route's table.  Per CALL entry the method's parameters are
    looked up by name in the ``params`` object and converted column by column: an I32 / I64 /
    BOOL slot is the value, an F64 slot the double's bits, a STR slot ``offset | length << 32``
    of the bytes between the quotes, relative to the body's first byte.  ARGS_INVALID entries
    answer -32602 without the host looking at them; spans outside the strict subset of
    include/rpccrc.h read ARGS_DEFER: parse those on the host as before (``json.loads`` on the
    span) and overwrite their ``reply_status``.  ``width`` (default ``schema.width``) is the
    number of slot columns."""
    t = _torch()
    n = body_offsets.numel()
    for name, x, size in (("body_offsets", body_offsets, 8), ("body_lens", body_lens, 4), ("route.kind", route.kind, 1),
                          ("route.method", route.method, 2), ("route.params_off", route.params_off, 4),
                          ("route.params_len", route.params_len, 4)):
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if bodies.element_size() != 1 or not bodies.is_contiguous():
        raise ValueError("bodies must be a contiguous uint8 tensor")
    if (schema.first.numel() != schema.nmethods + 1 or schema.types.numel() != schema.nparams or
            schema.name_off.numel() != schema.nparams + 1 or schema.first.element_size() != 4 or
            schema.types.element_size() != 1 or schema.name_off.element_size() != 4):
        raise ValueError("schema needs nmethods + 1 4-byte CSR words, nparams types and nparams + 1 4-byte name words")
    width = schema.width if width is None else int(width)
    dev = bodies.device
    status = t.empty(n, dtype=t.uint8, device=dev)
    reply_status = t.empty(n, dtype=t.int32, device=dev)
    slots = t.empty((width if 1 <= width <= ARGS_MAX_PARAMS else 0, n), dtype=t.int64, device=dev)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    check(_lib.rpc_frames_args_device(ptr(bodies), bodies.numel() if ptr(bodies) else 0, ptr(body_offsets),
                                      ptr(body_lens), ptr(route.kind), ptr(route.method), ptr(route.params_off),
                                      ptr(route.params_len), n, ptr(schema.first), schema.nmethods, ptr(schema.types),
                                      ptr(schema.name_off), schema.nparams, ptr(schema.names), schema.names.numel(),
                                      width, ptr(slots), ptr(status), ptr(reply_status), _stream_handle(stream)),
          "rpc_frames_args_device")
    return FrameArgs(status, reply_status, slots)


class FrameResolve(NamedTuple):
    """What frames_resolve returns (device tensors; nothing is read back)."""
    kind: object        # uint8 [n]: RESOLVE_NONE / _MATCHED / _UNKNOWN / _DUPLICATE / _INVALID / _DEFER / _RANGE
    id: object          # int32 [n]: the reply's id (view as uint32)
    result_off: object  # int32 [n]: the `result` value, relative to the body's first byte ...
    result_len: object  # int32 [n]: ... 0 / 0 when the reply has none
    error_off: object   # int32 [n]: the `error` value likewise
    error_len: object   # int32 [n]
    slot: object        # int32 [n]: the pending slot a MATCHED / DUPLICATE entry names, else RESOLVE_NO_SLOT (-1)
    slot_entry: object  # int32 [npending]: the entry that completes each slot, -1 while it stays open
    open: object        # int32 [npending]: open[:nopen] lists the open slots, ascending
    nopen: object       # int32 [1]


def frames_resolve(bodies, body_offsets, body_lens, pending_ids=None, reply_types=None, stream=None) -> FrameResolve:
    """The JSON-RPC reply envelope of every delivered body, matched to the pending calls
    (rpc_frames_resolve_device): what sits between a client's ``frames_unpack`` and its
    completions.

    ``bodies, body_offsets, body_lens, reply_types`` are ``frames_unpack``'s outputs unchanged
    (``reply_types=None``: every entry is DATA).  ``pending_ids[s]`` is the id of the call in the
    caller's slot ``s`` (a 4-byte tensor; ``None`` or empty: decode only, every decoded entry
    reads RESOLVE_UNKNOWN).  Per entry: the kind, the id, where the first top-level ``result``
    and ``error`` values lie in the body, and the slot the reply answers; per slot: the entry
    that completes it.  Bodies outside the strict subset of include/rpccrc.h read RESOLVE_DEFER:
    parse those on the host as before."""
    t = _torch()
    n = body_offsets.numel()
    for name, x, size, opt in (("body_offsets", body_offsets, 8, False), ("body_lens", body_lens, 4, False),
                               ("reply_types", reply_types, 2, True)):
        if x is None and opt:
            continue
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if bodies.element_size() != 1 or not bodies.is_contiguous():
        raise ValueError("bodies must be a contiguous uint8 tensor")
    npending = 0 if pending_ids is None else pending_ids.numel()
    if npending and (pending_ids.element_size() != 4 or not pending_ids.is_contiguous()):
        raise ValueError("pending_ids must be a contiguous 4-byte tensor")
    if npending > RESOLVE_MAX_PENDING:
        raise ValueError(f"at most {RESOLVE_MAX_PENDING} pending ids")
    dev = bodies.device
    kind = t.empty(n, dtype=t.uint8, device=dev)
    rid, roff, rlen, eoff, elen, slot = (t.empty(n, dtype=t.int32, device=dev) for _ in range(6))
    slot_entry = t.empty(npending, dtype=t.int32, device=dev)
    opened = t.empty(max(npending, 1), dtype=t.int32, device=dev)  # (never a null pointer)
    nopen = t.empty(1, dtype=t.int32, device=dev)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    check(_lib.rpc_frames_resolve_device(ptr(bodies), bodies.numel() if ptr(bodies) else 0, ptr(body_offsets),
                                         ptr(body_lens), ptr(reply_types), n, ptr(pending_ids), npending, ptr(kind),
                                         ptr(rid), ptr(roff), ptr(rlen), ptr(eoff), ptr(elen), ptr(slot),
                                         ptr(slot_entry), opened.data_ptr(), nopen.data_ptr(), _stream_handle(stream)),
          "rpc_frames_resolve_device")
    return FrameResolve(kind, rid, roff, rlen, eoff, elen, slot, slot_entry, opened[:npending], nopen)


class FrameReply(NamedTuple):
    """What frames_reply returns (device tensors; ``total`` is the host-side byte count, or with
    a caller's ``out`` -- nothing is read back then -- a one-element int64 device tensor)."""
    bodies: object            # uint8: the reply bodies back to back
    body_offsets: object      # int64 [n]: where each entry's body starts (entries of size 0 share the next one's)
    body_lens: object         # int32 [n]: its length (view as uint32)
    types: object             # int16 [n]: frames_pack's types: DATA / what reply_types held / TYPE_NONE
    status: object            # uint8 [n]: REPLY_NONE / _RESULT / _ERROR / _RAW / _RANGE / _NO_ROOM
    conn_bytes_first: object  # int64 [nconn + 1], or None without conn_first
    total: object             # bytes of all entries, whether they fitted or not


def frames_reply(kind, rid, values, value_offsets, value_lens, status=None, reply_types=None, conn_first=None,
                 out=None, stream=None) -> FrameReply:
    """JSON-RPC reply bodies from id + value (rpc_frames_reply_device): what sits between the
    handlers and ``frames_pack``.

    ``kind`` and ``rid`` are ``frames_route``'s ``kind`` and ``id`` unchanged (``kind=None``: every
    DATA entry is a CALL), ``reply_types`` is ``frames_unpack``'s (``None``: every entry is DATA).
    Entry i's value is ``values[value_offsets[i] : + value_lens[i]]``: the JSON text of a CALL's
    result, wrapped as ``{"jsonrpc":"2.0","id":<id>,"result":<value>}`` (``null`` when empty);
    with ``status[i] != 0`` the error form with that code -- one of the reference's five codes
    brings its own message, any other takes the value as the (escaped) message; for a
    ROUTE_DEFER entry the whole reply the host built, copied verbatim.  NOT_FOUND and INVALID
    entries are answered from ``rid`` alone.  ``bodies, body_offsets, body_lens, types`` go to
    ``frames_pack`` unchanged, with the unpack's versions and the same ``conn_first``.

    ``out=None`` makes the layout-only call first, reads the total (one synchronisation),
    allocates exactly and builds.  With ``out`` (a contiguous uint8 device tensor that does not
    overlap ``values``) nothing is read back: entries that do not end inside it are
    REPLY_NO_ROOM / TYPE_NONE and not written, and ``total`` stays on the device."""
    t = _torch()
    n = rid.numel()
    for name, x, size, opt in (("kind", kind, 1, True), ("rid", rid, 4, False), ("status", status, 4, True),
                               ("reply_types", reply_types, 2, True), ("value_offsets", value_offsets, 8, False),
                               ("value_lens", value_lens, 4, False)):
        if x is None and opt:
            continue
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if values.element_size() != 1 or not values.is_contiguous():
        raise ValueError("values must be a contiguous uint8 tensor")
    if conn_first is not None and (conn_first.numel() < 1 or conn_first.element_size() != 8):
        raise ValueError("conn_first needs nconn + 1 8-byte entries")
    if out is not None and (out.element_size() != 1 or not out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor")
    dev = rid.device
    nconn = 0 if conn_first is None else conn_first.numel() - 1
    sh = _stream_handle(stream)
    body_offsets = t.empty(n, dtype=t.int64, device=dev)
    body_lens = t.empty(n, dtype=t.int32, device=dev)
    types = t.empty(n, dtype=t.int16, device=dev)
    state = t.empty(n, dtype=t.uint8, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    def run(dst, layout_only):
        outs = (None,) * 5 if layout_only else (ptr(body_offsets), ptr(body_lens), ptr(types), ptr(state), ptr(cbf))
        check(_lib.rpc_frames_reply_device(ptr(kind), ptr(rid), ptr(status), ptr(reply_types), n, ptr(values),
                                           values.numel() if ptr(values) else 0, ptr(value_offsets), ptr(value_lens),
                                           None if conn_first is None else conn_first.data_ptr(), nconn, ptr(dst),
                                           0 if dst is None else dst.numel(), *outs, total.data_ptr(), sh),
              "rpc_frames_reply_device")

    if out is not None:
        run(out, False)
        return FrameReply(out, body_offsets, body_lens, types, state, cbf, total)
    run(None, True)  # layout only: the total (read on the call's stream: one synchronisation)
    nb = _read_back(total, stream)
    out = t.empty(nb, dtype=t.uint8, device=dev)
    run(out, False)
    return FrameReply(out, body_offsets, body_lens, types, state, cbf, nb)


class FrameRequest(NamedTuple):
    """What frames_request returns (device tensors; ``total`` is the host-side byte count, or with
    a caller's ``out`` -- nothing is read back then -- a one-element int64 device tensor)."""
    bodies: object            # uint8: the request bodies back to back
    body_offsets: object      # int64 [n]: where each entry's body starts (entries of size 0 share the next one's)
    body_lens: object         # int32 [n]: its length (view as uint32)
    types: object             # int16 [n]: frames_pack's types: DATA / what types held / TYPE_NONE
    status: object            # uint8 [n]: REQUEST_NONE / _CALL / _RAW / _BAD_METHOD / _RANGE / _NO_ROOM
    conn_bytes_first: object  # int64 [nconn + 1], or None without conn_first
    total: object             # bytes of all entries, whether they fitted or not


def frames_request(method, rid, params, params_offsets, params_lens, table: RouteTable, types=None, conn_first=None,
                   out=None, stream=None) -> FrameRequest:
    """JSON-RPC request bodies from method + params + id (rpc_frames_request_device): what sits in
    front of a client's ``frames_pack``.

    ``method[i]`` indexes ``table`` (``route_table``: the server's table, so the index is what
    ``frames_route`` gives back), ``rid[i]`` is the call's id -- the ids are ``frames_resolve``'s
    ``pending_ids`` -- and entry i's params are ``params[params_offsets[i] : + params_lens[i]]``:
    JSON text, wrapped as ``{"jsonrpc":"2.0","method":"<name>","params":<params>,"id":<id>}``, or
    without the ``params`` member when empty.  ``method[i] == ROUTE_NO_METHOD`` copies the bytes
    verbatim: a whole request the host built.  ``types`` are ``frames_pack``'s (``None``: every
    entry is DATA); an entry of another type has no body and keeps its type.  ``bodies,
    body_offsets, body_lens, types`` go to ``frames_pack`` unchanged, with the same ``conn_first``.

    ``out=None`` makes the layout-only call first, reads the total (one synchronisation),
    allocates exactly and builds.  With ``out`` (a contiguous uint8 device tensor that does not
    overlap ``params``) nothing is read back: entries that do not end inside it are
    REQUEST_NO_ROOM / TYPE_NONE and not written, and ``total`` stays on the device."""
    t = _torch()
    n = rid.numel()
    for name, x, size, opt in (("method", method, 2, False), ("rid", rid, 4, False), ("types", types, 2, True),
                               ("params_offsets", params_offsets, 8, False), ("params_lens", params_lens, 4, False)):
        if x is None and opt:
            continue
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    if params.element_size() != 1 or not params.is_contiguous():
        raise ValueError("params must be a contiguous uint8 tensor")
    if table.offsets.numel() != table.nmethods + 1 or table.offsets.element_size() != 4:
        raise ValueError("table.offsets needs nmethods + 1 4-byte entries")
    if conn_first is not None and (conn_first.numel() < 1 or conn_first.element_size() != 8):
        raise ValueError("conn_first needs nconn + 1 8-byte entries")
    if out is not None and (out.element_size() != 1 or not out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor")
    dev = rid.device
    nconn = 0 if conn_first is None else conn_first.numel() - 1
    sh = _stream_handle(stream)
    body_offsets = t.empty(n, dtype=t.int64, device=dev)
    body_lens = t.empty(n, dtype=t.int32, device=dev)
    types_out = t.empty(n, dtype=t.int16, device=dev)
    state = t.empty(n, dtype=t.uint8, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    def run(dst, layout_only):
        outs = (None,) * 5 if layout_only else (ptr(body_offsets), ptr(body_lens), ptr(types_out), ptr(state), ptr(cbf))
        check(_lib.rpc_frames_request_device(ptr(method), ptr(rid), ptr(types), n, ptr(table.names),
                                             table.names.numel(), ptr(table.offsets), table.nmethods, ptr(params),
                                             params.numel() if ptr(params) else 0, ptr(params_offsets),
                                             ptr(params_lens), None if conn_first is None else conn_first.data_ptr(),
                                             nconn, ptr(dst), 0 if dst is None else dst.numel(), *outs,
                                             total.data_ptr(), sh),
              "rpc_frames_request_device")

    if out is not None:
        run(out, False)
        return FrameRequest(out, body_offsets, body_lens, types_out, state, cbf, total)
    run(None, True)  # layout only: the total (read on the call's stream: one synchronisation)
    nb = _read_back(total, stream)
    out = t.empty(nb, dtype=t.uint8, device=dev)
    run(out, False)
    return FrameRequest(out, body_offsets, body_lens, types_out, state, cbf, nb)


def result_types(methods, results, device=None):
    """The ``d_result_types`` tensor of frames_values' RESULT form: ``results[m]`` is the result
    type of ``methods[m]`` (the list ``args_schema`` and ``route_table`` are built from), an
    ``ARG_*`` constant or one of the IDL's names."""
    t = _torch()
    if len(results) != len(methods):
        raise ValueError("one result type per method")
    if len(results) > ROUTE_MAX_METHODS:
        raise ValueError(f"at most {ROUTE_MAX_METHODS} methods")
    codes = [_ARG_TYPES[r] if isinstance(r, str) else int(r) for r in results]
    return t.tensor(codes, dtype=t.uint8).to("cuda" if device is None else device)


class FrameValues(NamedTuple):
    """What frames_values returns (device tensors; ``total`` is the host-side byte count, or with
    a caller's ``out`` -- nothing is read back then -- a one-element int64 device tensor)."""
    values: object         # uint8: the value texts back to back
    value_offsets: object  # int64 [n]: where each entry's text starts
    value_lens: object     # int32 [n]: its length (view as uint32)
    status: object         # uint8 [n]: VALUES_NONE / _OK / _TEXT / _DEFER / _RANGE / _BAD_SCHEMA / _NO_ROOM
    reply_status: object   # int32 [n]: the given status, or -32603 for an entry nobody formatted
    ndefer: object         # int32 [1]: the number of VALUES_DEFER entries
    total: object          # bytes of all entries, whether they fitted or not


def frames_values(method, slots, schema, form: int = VALUES_FORM_RESULT, mode=None, status=None, strings=None,
                  str_base=None, texts=None, text_offsets=None, text_lens=None, out=None, stream=None) -> FrameValues:
    """Typed results or params as JSON text (rpc_frames_values_device): the args' mirror, what
    sits between the handlers' columns and ``frames_reply`` (RESULT form) and between a client's
    columns and ``frames_request`` (PARAMS form).

    ``slots`` is an 8-byte tensor ``[width, n]``, column-major as ``frames_args`` leaves it: an
    I32 / I64 / BOOL slot is the value, an F64 slot the double's bits, a STR slot
    ``offset | length << 32`` into ``strings``, relative to ``str_base[i]``.  ``schema`` is
    ``result_types(...)`` in RESULT form (slot 0 is the result) and ``args_schema(...)`` in PARAMS
    form.  ``mode[i]`` (``None``: ENCODE) picks VALUES_MODE_NONE, _ENCODE or _TEXT, the host's own
    text ``texts[text_offsets[i] : + text_lens[i]]``; an entry with ``status[i] != 0`` has no
    value.  A double's text is cJSON's print_number byte for byte; strings that need an escape
    and subnormals read VALUES_DEFER: format those on the host and call again with them as TEXT
    (``ndefer`` says whether there are any).  ``values, value_offsets, value_lens, reply_status``
    go to ``frames_reply`` as ``values, value_offsets, value_lens, status``, or the first three to
    ``frames_request`` as its params.

    ``out=None`` makes the layout-only call first, reads the total (one synchronisation),
    allocates exactly and builds.  With ``out`` nothing is read back: entries that do not end
    inside it are VALUES_NO_ROOM and not written, and ``total`` stays on the device."""
    t = _torch()
    n = method.numel()
    params = form == VALUES_FORM_PARAMS
    if slots.dim() != 2 or slots.element_size() != 8 or not slots.is_contiguous() or slots.shape[1] != n:
        raise ValueError(f"slots must be a contiguous 8-byte tensor [width, {n}]")
    width = slots.shape[0]
    for name, x, size in (("method", method, 2), ("mode", mode, 1), ("status", status, 4), ("str_base", str_base, 8),
                          ("text_offsets", text_offsets, 8), ("text_lens", text_lens, 4)):
        if x is None:
            continue
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with n = {n} elements")
    for name, x in (("strings", strings), ("texts", texts), ("out", out)):
        if x is not None and (x.element_size() != 1 or not x.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor")
    if params:
        if (schema.first.numel() != schema.nmethods + 1 or schema.types.numel() != schema.nparams or
                schema.name_off.numel() != schema.nparams + 1 or schema.first.element_size() != 4 or
                schema.types.element_size() != 1 or schema.name_off.element_size() != 4):
            raise ValueError("schema needs nmethods + 1 4-byte CSR words, nparams types and nparams + 1 4-byte name words")
    elif schema.element_size() != 1 or not schema.is_contiguous():
        raise ValueError("result types must be a contiguous uint8 tensor")
    dev = method.device
    sh = _stream_handle(stream)
    value_offsets = t.empty(n, dtype=t.int64, device=dev)
    value_lens = t.empty(n, dtype=t.int32, device=dev)
    state = t.empty(n, dtype=t.uint8, device=dev)
    reply_status = t.empty(n, dtype=t.int32, device=dev)
    ndefer = t.empty(1, dtype=t.int32, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    if params:
        sch = (None, ptr(schema.first), schema.nmethods, ptr(schema.types), ptr(schema.name_off), schema.nparams,
               ptr(schema.names), schema.names.numel())
    else:
        sch = (ptr(schema), None, schema.numel(), None, None, 0, None, 0)

    def run(dst, layout_only):
        outs = (None,) * 5 if layout_only else (ptr(value_offsets), ptr(value_lens), ptr(state), ptr(reply_status),
                                                ndefer.data_ptr())
        check(_lib.rpc_frames_values_device(int(form), ptr(mode), ptr(status), ptr(method), ptr(slots), width, n, *sch,
                                            ptr(strings), strings.numel() if ptr(strings) else 0, ptr(str_base),
                                            ptr(texts), texts.numel() if ptr(texts) else 0, ptr(text_offsets),
                                            ptr(text_lens), ptr(dst), 0 if dst is None else dst.numel(), *outs,
                                            total.data_ptr(), sh),
              "rpc_frames_values_device")

    if out is not None:
        run(out, False)
        return FrameValues(out, value_offsets, value_lens, state, reply_status, ndefer, total)
    run(None, True)  # layout only: the total (read on the call's stream: one synchronisation)
    nb = _read_back(total, stream)
    out = t.empty(nb, dtype=t.uint8, device=dev)
    run(out, False)
    return FrameValues(out, value_offsets, value_lens, state, reply_status, ndefer, nb)


class FrameScan(NamedTuple):
    """What frames_scan returns (device tensors; ``nframes`` is the host-side count)."""
    frame_offsets: object  # int64 [max_frames]: absolute offsets, padding entries = stream_bytes
    frame_conn: object     # int32 [max_frames]: the frame's connection (-1 in the padding)
    conn_first: object     # int64 [nconn + 1]: CSR over the frames found
    consumed: object       # int64 [nconn]: bytes of each connection that may be dropped
    state: object          # uint8 [nconn]: CONN_OPEN / CONN_CLOSED
    verdict: object        # uint8 [max_frames] (verify=True), else None
    crc: object            # int32 [max_frames] (verify=True), else None
    nframes: object        # frames found (int64 [1] on the device with read_count=False)


def frames_scan(stream_buf, conn_offsets, conn_lengths, role: str = "server", lift_cap: bool = False,
                max_frames: Optional[int] = None, verify: bool = False, stream=None, stream_bytes=None,
                read_count: bool = True):
    """Find the wire frames in raw connection bytes (rpc_frames_scan_device).

    Connection c is ``stream_buf[conn_offsets[c] : + conn_lengths[c]]`` (int64/uint64 device
    tensors).  Each connection's headers are walked from its first byte with the
    reference's stop rules (include/rpccrc.h); a trailing partial frame is left for the
    next read: ``consumed[c]`` bytes may be dropped, the rest is the carry-over.
    ``max_frames=None`` counts first, synchronises once and allocates exactly; otherwise
    the call raises if more than ``max_frames`` frames are found.  With ``max_frames`` and
    ``read_count=False`` nothing is read back and nothing synchronises: ``nframes`` is a
    one-element int64 device tensor, and of more than ``max_frames`` frames the first
    ``max_frames`` are kept (the count still says how many there were).  ``verify=True`` also
    runs frames_verify on the frames found and marks what lies behind a closing frame
    FRAME_NOT_REACHED (rpc_frames_scan_verify_device)."""
    t = _torch()
    dev = stream_buf.device
    nconn = conn_offsets.numel()
    if conn_lengths.numel() != nconn:
        raise ValueError("conn_offsets and conn_lengths differ in length")
    nbytes = stream_buf.numel() * stream_buf.element_size() if stream_bytes is None else int(stream_bytes)
    flags = _frames_flags(role, lift_cap)
    sh = _stream_handle(stream)
    conn_first = t.empty(nconn + 1, dtype=t.int64, device=dev)
    consumed = t.empty(nconn, dtype=t.int64, device=dev)
    state = t.empty(nconn, dtype=t.uint8, device=dev)
    nframes = t.empty(1, dtype=t.int64, device=dev)

    def ptr(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()

    def run(cap, offs, conn, verdict, crc):
        common = (stream_buf.data_ptr(), nbytes, ptr(conn_offsets), ptr(conn_lengths), nconn, flags, ptr(offs),
                  ptr(conn), cap, conn_first.data_ptr(), ptr(consumed), ptr(state), nframes.data_ptr())
        if verdict is None:
            check(_lib.rpc_frames_scan_device(*common, sh), "rpc_frames_scan_device")
        else:
            check(_lib.rpc_frames_scan_verify_device(*common, ptr(verdict), ptr(crc), sh),
                  "rpc_frames_scan_verify_device")

    def count():  # (the count is read on the call's stream: one synchronisation)
        return _read_back(nframes, stream)

    if max_frames is None and not read_count:
        raise ValueError("read_count=False needs max_frames")
    if max_frames is None:
        run(0, None, None, None, None)
        cap = count()
    else:
        cap = int(max_frames)
    offs = t.empty(cap, dtype=t.int64, device=dev)
    conn = t.empty(cap, dtype=t.int32, device=dev)
    verdict = t.empty(cap, dtype=t.uint8, device=dev) if verify else None
    crc = t.empty(cap, dtype=t.int32, device=dev) if verify else None
    run(cap, offs, conn, verdict, crc)
    if not read_count:
        return FrameScan(offs, conn, conn_first, consumed, state, verdict, crc, nframes)
    found = count() if max_frames is not None else cap
    if found > cap:
        raise ValueError(f"frames_scan found {found} frames, max_frames is {cap}")
    return FrameScan(offs, conn, conn_first, consumed, state, verdict, crc, found)


#: rpc_frames_set_scan_path codes (include/rpccrc.h RPCCRC_SCAN_*)
SCAN_PATHS = {"auto": 0, "serial": 1, "tiled": 2}


def set_scan_path(path="auto"):
    """Route of frames_scan (results identical): "auto" (long connections tiled, the rest
    serial), "serial" (one lane per connection walks its headers) or "tiled" (every
    cap-in-force connection of more than one tile takes the tile-map route)."""
    code = SCAN_PATHS[path] if isinstance(path, str) else int(path)
    check(_lib.rpc_frames_set_scan_path(code), "rpc_frames_set_scan_path")


def fill_random(tensor, seed: int, stream=None):
    """splitmix64 counter stream into a device tensor (nbytes multiple of 8)."""
    nbytes = tensor.numel() * tensor.element_size()
    check(_lib.rpc_crc32_fill_random_device(tensor.data_ptr(), nbytes, seed & (2**64 - 1), _stream_handle(stream)),
          "rpc_crc32_fill_random_device")
    return tensor


def stream_read(tensor, pattern: int = 0, nontemporal: bool = False, nbytes: Optional[int] = None, stream=None):
    """HBM read probe: pattern 0 coalesced 16-B lanes, 1 = 64-B lane segments (grid-stride
    loops), 2 = the rows kernel's own dealing and loads with the CRC work compiled out."""
    if nbytes is None:
        nbytes = (tensor.numel() * tensor.element_size()) // 4096 * 4096
    check(_lib.rpc_crc32_stream_read_device(tensor.data_ptr(), nbytes, pattern, int(nontemporal),
                                            _stream_handle(stream)), "rpc_crc32_stream_read_device")


def set_options(nontemporal: bool = False, max_blocks: int = 0):
    check(_lib.rpc_crc32_set_options(int(nontemporal), max_blocks), "rpc_crc32_set_options")


#: rpc_crc32_set_ragged_path codes (include/rpccrc.h RPCCRC_RAGGED_*)
RAGGED_PATHS = {"auto": 0, "rows": 1, "packed": 2, "split": 3}


def set_ragged_path(path="auto"):
    """Kernel for ragged device batches: "auto" (frames: split, other batches: rows),
    "rows" (one wavefront per body), "packed" (1 KiB chunks of consecutive
    bodies, four per row) or "split" (bodies <= 1 KiB four per row, the rest
    one wavefront per body)."""
    code = RAGGED_PATHS[path] if isinstance(path, str) else int(path)
    check(_lib.rpc_crc32_set_ragged_path(code), "rpc_crc32_set_ragged_path")


def device_status() -> int:
    """0, or -5 (RPCCRC_EIO) once a kernel of an asynchronous call has reported an
    error into the device's error word (until device_clear_status())."""
    return int(_lib.rpc_crc32_device_status())


def device_clear_status() -> int:
    """Clears the device error word; returns the status it held (0 or -5)."""
    return int(_lib.rpc_crc32_device_clear_status())


def service_stop() -> int:
    """Stops the resident drop-in service (the next drop-in call restarts it), so a
    device-wide synchronize does not wait for it; 0, or -5 if it did not leave in time."""
    return int(_lib.rpc_crc32_service_stop())


def service_stats() -> dict:
    """The drop-in service's counters over every device this process used
    (rpccrc_service_stats_t): services, running, launched, answered,
    fallbacks_full, fallbacks_short, bypassed."""
    st = _lib.ServiceStats()
    check(_lib.rpc_crc32_service_stats(ctypes.byref(st)), "rpc_crc32_service_stats")
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def device_info() -> str:
    buf = ctypes.create_string_buffer(256)
    check(_lib.rpc_crc32_device_info(buf, 256), "rpc_crc32_device_info")
    return buf.value.decode()
