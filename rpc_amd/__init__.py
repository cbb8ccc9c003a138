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

This module holds the host and device CRC calls; the frame stages live in
``rpc_amd.frames``, the constants in ``rpc_amd.constants``, and both are
re-exported here.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib, rx_ring  # (_lib first: it imports torch before it loads the library)
from ._lib import RpcCrcError, check, lib
from .rx_ring import RxRing
from .constants import *  # noqa: F401,F403
from ._device import _dev_u32_out, _read_back, _stream_handle, _torch  # noqa: F401
from .frames import (  # noqa: F401
    SCAN_PATHS, ArgsSchema, FrameArgs, FrameCarry, FramePack, FrameReply, FrameRequest, FrameResolve, FrameResults,
    FrameRoute, FrameScan, FrameUnpack, FrameValues, RouteTable, args_schema, carry_slots, frames_args, frames_carry,
    frames_pack, frames_reply, frames_request, frames_resolve, frames_results, frames_route, frames_scan, frames_stamp,
    frames_unpack, frames_values, frames_verify, result_types, route_table, set_scan_path,
)

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
    "frames_results",
    "FrameResults",
    "RESULTS_NONE",
    "RESULTS_OK",
    "RESULTS_ABSENT",
    "RESULTS_MISMATCH",
    "RESULTS_DEFER",
    "RESULTS_RANGE",
    "RESULTS_BAD_SCHEMA",
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
    # (None is NULL; an empty tensor passes its own address, whatever that is)
    base_at, offs_at, lens_at, seed_at = (None if x is None else x.data_ptr()
                                          for x in (base, seg_offsets, seg_lengths, seed))
    check(_lib.rpc_crc32_device_gather(base_at, offs_at, lens_at, nseg, int(max_seg_len) & 0xFFFFFFFF,
                                       seg_first.data_ptr(), n, seed_at, out.data_ptr(), _stream_handle(stream)),
          "rpc_crc32_device_gather")
    return out


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
