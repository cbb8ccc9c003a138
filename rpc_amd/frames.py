"""The frame stages of include/rpccrc.h on device tensors: verify, stamp, scan, unpack, carry,
route, args, resolve, results, values, reply, request and pack, with their result types and the builders
of the method table and the parameter schema.  ``rpc_amd`` re-exports all of it.

Every wrapper checks its tensors, allocates its outputs and makes one call of ``_lib.<entry>``,
looked up when the wrapper runs.  The stages whose output size is only known on the device
(pack, unpack, reply, request, values) share one sizing protocol, ``_sized``.  The stream
contract is the one stated in ``_device``."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._device import _count, _dev_u32_out, _ptr, _read_back, _stream_handle, _torch
from ._lib import check
from .constants import (ARG_BOOL, ARG_F64, ARG_I32, ARG_I64, ARG_STR, ARGS_MAX_NAME_BYTES, ARGS_MAX_PARAMS,
                        ARGS_MAX_SCHEMA_PARAMS, CARRY_ROOM, FRAMES_CLIENT, FRAMES_LIFT_CAP, FRAMES_SERVER,
                        RESOLVE_MAX_PENDING, ROUTE_MAX_METHOD_BYTES, ROUTE_MAX_METHODS, RPC_TYPE_DATA,
                        VALUES_FORM_PARAMS, VALUES_FORM_RESULT)


# ---- what the wrappers share: argument checks and the sizing protocol ------------------------

def _check_tensors(count: str, n: int, entries, optional=()):
    """Every ``(name, tensor, element size)`` entry is a contiguous tensor of ``n`` elements of that
    size; ``count`` is what the message calls n.  A name in ``optional`` may be None."""
    for name, x, size in entries:
        if x is None and name in optional:
            continue
        if x.numel() != n or x.element_size() != size or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {size}-byte tensor with {count} = {n} elements")


def _check_bytes(name: str, x):
    """``x`` is a byte buffer: contiguous uint8, any length."""
    if x.element_size() != 1 or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous uint8 tensor")


def _check_conn_first(conn_first) -> int:
    """The CSR over the entries, if given: nconn + 1 8-byte entries.  Returns nconn."""
    if conn_first is None:
        return 0
    if conn_first.numel() < 1 or conn_first.element_size() != 8:
        raise ValueError("conn_first needs nconn + 1 8-byte entries")
    return conn_first.numel() - 1


def _check_table(table: RouteTable):
    if table.offsets.numel() != table.nmethods + 1 or table.offsets.element_size() != 4:
        raise ValueError("table.offsets needs nmethods + 1 4-byte entries")


def _check_schema(schema: ArgsSchema):
    if (schema.first.numel() != schema.nmethods + 1 or schema.types.numel() != schema.nparams or
            schema.name_off.numel() != schema.nparams + 1 or schema.first.element_size() != 4 or
            schema.types.element_size() != 1 or schema.name_off.element_size() != 4):
        raise ValueError("schema needs nmethods + 1 4-byte CSR words, nparams types and nparams + 1 4-byte name words")


def _sized(run, total, out, stream, device):
    """The sizing protocol of the stages that write ``out``: ``run(dst, layout_only)`` is the
    stage's C call, which always writes the byte count to ``total`` (int64 [1] on the device).
    With ``out`` one call, and ``total`` stays on the device.  Without: the layout-only call (no
    destination, no per-entry outputs), the total read back on the call's stream (the one
    synchronisation), a uint8 tensor of exactly that size, and the real call.  Returns
    ``(out, total)``, the total as that device tensor or as the int read back."""
    if out is not None:
        run(out, False)
        return out, total
    run(None, True)
    nb = _read_back(total, stream)
    t = _torch()
    out = t.empty(nb, dtype=t.uint8, device=device)
    run(out, False)
    return out, nb


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
    _check_tensors("n", n, (("body_lens", body_lens, 4), ("types", types, 2), ("versions", versions, 2),
                            ("body_offsets", body_offsets, 8)),
                   optional=("body_lens", "types", "versions", "body_offsets"))
    nconn = _check_conn_first(conn_first)
    if out is not None:
        _check_bytes("out", out)
    dev = next(x for x in (bodies, body_offsets, types, out) if x is not None).device
    nbytes = 0 if bodies is None else bodies.numel() * bodies.element_size()
    flags = FRAMES_LIFT_CAP if lift_cap else 0
    sh = _stream_handle(stream)
    offsets = t.empty(n, dtype=t.int64, device=dev)
    verdict = t.empty(n, dtype=t.uint8, device=dev)
    crc = t.empty(n, dtype=t.int32, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def run(dst, layout_only):
        outs = (None,) * 4 if layout_only else (_ptr(offsets), _ptr(verdict), _ptr(crc), _ptr(cbf))
        check(_lib.rpc_frames_pack_device(_ptr(bodies), nbytes if _ptr(bodies) else 0, _ptr(body_offsets), _ptr(body_lens), n,
                                          _ptr(types), int(type_) & 0xFFFF, _ptr(versions), int(version) & 0xFFFF,
                                          None if conn_first is None else conn_first.data_ptr(), nconn, flags,
                                          _ptr(dst), _count(dst), *outs, total.data_ptr(), sh), "rpc_frames_pack_device")

    out, size = _sized(run, total, out, stream, dev)
    return FramePack(out, offsets, verdict, crc, cbf, size)


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
    _check_tensors("n", n, (("frame_offsets", frame_offsets, 8), ("verdict", verdict, 1)))
    nconn = _check_conn_first(conn_first)
    if out is not None:
        _check_bytes("out", out)
    dev = stream_buf.device
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

    def run(dst, layout_only):
        outs = (None,) * 6 if layout_only else (_ptr(body_offsets), _ptr(body_lens), _ptr(reply_types), _ptr(versions),
                                                _ptr(verdict_out), _ptr(cbf))
        check(_lib.rpc_frames_unpack_device(_ptr(stream_buf), nbytes if _ptr(stream_buf) else 0, _ptr(frame_offsets),
                                            _ptr(verdict), n, None if conn_first is None else conn_first.data_ptr(),
                                            nconn, flags, 1 if nul else 0, _ptr(dst), _count(dst), *outs,
                                            total.data_ptr(), sh), "rpc_frames_unpack_device")

    out, size = _sized(run, total, out, stream, dev)
    return FrameUnpack(out, body_offsets, body_lens, reply_types, versions, verdict_out, cbf, size)


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
    _check_tensors("nconn", nconn, (("conn_offsets", conn_offsets, 8), ("conn_lengths", conn_lengths, 8),
                                    ("consumed", consumed, 8), ("state", state, 1), ("next_at", next_at, 8),
                                    ("new_lengths", new_lengths, 8)), optional=("state", "new_lengths"))
    _check_bytes("stream_buf", stream_buf)
    _check_bytes("next_buf", next_buf)
    if room < 0:
        raise ValueError("room must not be negative")
    dev = next_buf.device
    next_offsets = t.empty(nconn, dtype=t.int64, device=dev)
    next_lengths = t.empty(nconn, dtype=t.int64, device=dev)
    status = t.empty(nconn, dtype=t.uint8, device=dev)
    carried = t.empty(1, dtype=t.int64, device=dev)

    check(_lib.rpc_frames_carry_device(_ptr(stream_buf), _count(stream_buf), _ptr(conn_offsets), _ptr(conn_lengths),
                                       _ptr(consumed), _ptr(state), nconn, _ptr(next_buf), _count(next_buf), _ptr(next_at),
                                       int(room), _ptr(new_lengths), _ptr(next_offsets), _ptr(next_lengths), _ptr(status),
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
    _check_tensors("n", n, (("body_offsets", body_offsets, 8), ("body_lens", body_lens, 4),
                            ("reply_types", reply_types, 2)), optional=("reply_types",))
    _check_bytes("bodies", bodies)
    _check_table(table)
    dev = bodies.device
    kind = t.empty(n, dtype=t.uint8, device=dev)
    method = t.empty(n, dtype=t.int16, device=dev)
    rid = t.empty(n, dtype=t.int32, device=dev)
    poff = t.empty(n, dtype=t.int32, device=dev)
    plen = t.empty(n, dtype=t.int32, device=dev)
    order = t.empty(max(n, 1), dtype=t.int32, device=dev) if group else None  # (never a null pointer)
    first = t.empty(table.nmethods + 4, dtype=t.int32, device=dev) if group else None

    check(_lib.rpc_frames_route_device(_ptr(bodies), _count(bodies), _ptr(body_offsets),
                                       _ptr(body_lens), _ptr(reply_types), n, _ptr(table.names), table.names.numel(),
                                       _ptr(table.offsets), table.nmethods, _ptr(kind), _ptr(method), _ptr(rid), _ptr(poff),
                                       _ptr(plen), order.data_ptr() if group else None,
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
    _check_tensors("n", n, (("body_offsets", body_offsets, 8), ("body_lens", body_lens, 4), ("route.kind", route.kind, 1),
                            ("route.method", route.method, 2), ("route.params_off", route.params_off, 4),
                            ("route.params_len", route.params_len, 4)))
    _check_bytes("bodies", bodies)
    _check_schema(schema)
    width = schema.width if width is None else int(width)
    dev = bodies.device
    status = t.empty(n, dtype=t.uint8, device=dev)
    reply_status = t.empty(n, dtype=t.int32, device=dev)
    slots = t.empty((width if 1 <= width <= ARGS_MAX_PARAMS else 0, n), dtype=t.int64, device=dev)

    check(_lib.rpc_frames_args_device(_ptr(bodies), _count(bodies), _ptr(body_offsets),
                                      _ptr(body_lens), _ptr(route.kind), _ptr(route.method), _ptr(route.params_off),
                                      _ptr(route.params_len), n, _ptr(schema.first), schema.nmethods, _ptr(schema.types),
                                      _ptr(schema.name_off), schema.nparams, _ptr(schema.names), schema.names.numel(),
                                      width, _ptr(slots), _ptr(status), _ptr(reply_status), _stream_handle(stream)),
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
    _check_tensors("n", n, (("body_offsets", body_offsets, 8), ("body_lens", body_lens, 4),
                            ("reply_types", reply_types, 2)), optional=("reply_types",))
    _check_bytes("bodies", bodies)
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

    check(_lib.rpc_frames_resolve_device(_ptr(bodies), _count(bodies), _ptr(body_offsets),
                                         _ptr(body_lens), _ptr(reply_types), n, _ptr(pending_ids), npending, _ptr(kind),
                                         _ptr(rid), _ptr(roff), _ptr(rlen), _ptr(eoff), _ptr(elen), _ptr(slot),
                                         _ptr(slot_entry), opened.data_ptr(), nopen.data_ptr(), _stream_handle(stream)),
          "rpc_frames_resolve_device")
    return FrameResolve(kind, rid, roff, rlen, eoff, elen, slot, slot_entry, opened[:npending], nopen)


class FrameResults(NamedTuple):
    """What frames_results returns (device tensors; nothing is read back)."""
    status: object             # uint8 [n]: RESULTS_NONE / _OK / _ABSENT / _MISMATCH / _DEFER / _RANGE / _BAD_SCHEMA
    value: object              # int64 [n]: the typed `result` (F64: .view(torch.float64)), 0 unless RESULTS_OK
    error_status: object       # uint8 [n]: the `error` member's status, same codes
    error_code: object         # int32 [n]: its `code`, 0 unless RESULTS_OK
    error_message: object      # int64 [n]: its `message` as offset | length << 32 into the body
    slot_status: object        # uint8 [npending]: the completing entry's status, 0 (RESULTS_NONE) while the slot is open
    slot_value: object         # int64 [npending]
    slot_error_status: object  # uint8 [npending]
    slot_error_code: object    # int32 [npending]
    slot_str_base: object      # int64 [npending]: the completing entry's body offset: frames_values' ``str_base``
    ndefer: object             # int32 [1]: entries whose status or error status is RESULTS_DEFER


def frames_results(bodies, body_offsets, body_lens, resolve: FrameResolve, pending_method, result_types,
                   stream=None) -> FrameResults:
    """The typed result of every matched reply, per entry and per pending slot
    (rpc_frames_results_device): what sits between a client's ``frames_resolve`` and its
    completions.

    ``bodies, body_offsets, body_lens`` are ``frames_unpack``'s outputs and ``resolve`` is
    ``frames_resolve``'s, all unchanged.  ``pending_method[s]`` (a 2-byte tensor beside
    ``pending_ids``) is the method slot ``s``'s request was sent with -- ``frames_request``'s
    ``method`` -- and ``result_types`` (``result_types(...)``) holds each method's result type.
    Per MATCHED entry the ``result`` span is converted as the reference's generated client reads
    it: an I32 / I64 / BOOL value is the value, an F64 value the double's bits, a STR value
    ``offset | length << 32`` of the bytes between the quotes, relative to the body's first byte;
    a missing member (RESULTS_ABSENT) or one of the wrong JSON type (RESULTS_MISMATCH) reads the
    default, 0.  The ``error`` member is decoded beside it into ``code`` and ``message``.  The
    ``slot_*`` columns hold the same answers indexed by pending slot, 0 while a slot stays open.
    Spans outside the strict subset of include/rpccrc.h read RESULTS_DEFER: parse those on the
    host as before (``json.loads`` on the span); ``ndefer`` says whether there are any."""
    t = _torch()
    n = body_offsets.numel()
    _check_tensors("n", n, (("body_offsets", body_offsets, 8), ("body_lens", body_lens, 4), ("resolve.kind", resolve.kind, 1),
                            ("resolve.slot", resolve.slot, 4), ("resolve.result_off", resolve.result_off, 4),
                            ("resolve.result_len", resolve.result_len, 4), ("resolve.error_off", resolve.error_off, 4),
                            ("resolve.error_len", resolve.error_len, 4)))
    _check_bytes("bodies", bodies)
    npending = 0 if pending_method is None else pending_method.numel()
    if npending > RESOLVE_MAX_PENDING:
        raise ValueError(f"at most {RESOLVE_MAX_PENDING} pending slots")
    _check_tensors("npending", npending, (("pending_method", pending_method, 2), ("resolve.slot_entry", resolve.slot_entry, 4)),
                   optional=("pending_method",))
    if result_types.element_size() != 1 or not result_types.is_contiguous() or result_types.numel() > ROUTE_MAX_METHODS:
        raise ValueError(f"result_types must be a contiguous 1-byte tensor of at most {ROUTE_MAX_METHODS} elements")
    dev = bodies.device
    status, estatus = (t.empty(n, dtype=t.uint8, device=dev) for _ in range(2))
    value, emsg = (t.empty(n, dtype=t.int64, device=dev) for _ in range(2))
    ecode = t.empty(n, dtype=t.int32, device=dev)
    s_status, s_estatus = (t.empty(npending, dtype=t.uint8, device=dev) for _ in range(2))
    s_value, s_base = (t.empty(npending, dtype=t.int64, device=dev) for _ in range(2))
    s_ecode = t.empty(npending, dtype=t.int32, device=dev)
    ndefer = t.empty(1, dtype=t.int32, device=dev)

    check(_lib.rpc_frames_results_device(_ptr(bodies), _count(bodies), _ptr(body_offsets), _ptr(body_lens),
                                         _ptr(resolve.kind), _ptr(resolve.slot), _ptr(resolve.result_off),
                                         _ptr(resolve.result_len), _ptr(resolve.error_off), _ptr(resolve.error_len),
                                         _ptr(resolve.slot_entry), n, _ptr(pending_method), npending, _ptr(result_types),
                                         result_types.numel(), _ptr(status), _ptr(value), _ptr(estatus), _ptr(ecode),
                                         _ptr(emsg), _ptr(s_status), _ptr(s_value), _ptr(s_estatus), _ptr(s_ecode),
                                         _ptr(s_base), ndefer.data_ptr(), _stream_handle(stream)),
          "rpc_frames_results_device")
    return FrameResults(status, value, estatus, ecode, emsg, s_status, s_value, s_estatus, s_ecode, s_base, ndefer)


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
    _check_tensors("n", n, (("kind", kind, 1), ("rid", rid, 4), ("status", status, 4), ("reply_types", reply_types, 2),
                            ("value_offsets", value_offsets, 8), ("value_lens", value_lens, 4)),
                   optional=("kind", "status", "reply_types"))
    _check_bytes("values", values)
    nconn = _check_conn_first(conn_first)
    if out is not None:
        _check_bytes("out", out)
    dev = rid.device
    sh = _stream_handle(stream)
    body_offsets = t.empty(n, dtype=t.int64, device=dev)
    body_lens = t.empty(n, dtype=t.int32, device=dev)
    types = t.empty(n, dtype=t.int16, device=dev)
    state = t.empty(n, dtype=t.uint8, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def run(dst, layout_only):
        outs = (None,) * 5 if layout_only else (_ptr(body_offsets), _ptr(body_lens), _ptr(types), _ptr(state), _ptr(cbf))
        check(_lib.rpc_frames_reply_device(_ptr(kind), _ptr(rid), _ptr(status), _ptr(reply_types), n, _ptr(values),
                                           _count(values), _ptr(value_offsets), _ptr(value_lens),
                                           None if conn_first is None else conn_first.data_ptr(), nconn, _ptr(dst),
                                           _count(dst), *outs, total.data_ptr(), sh), "rpc_frames_reply_device")

    out, size = _sized(run, total, out, stream, dev)
    return FrameReply(out, body_offsets, body_lens, types, state, cbf, size)


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
    _check_tensors("n", n, (("method", method, 2), ("rid", rid, 4), ("types", types, 2),
                            ("params_offsets", params_offsets, 8), ("params_lens", params_lens, 4)), optional=("types",))
    _check_bytes("params", params)
    _check_table(table)
    nconn = _check_conn_first(conn_first)
    if out is not None:
        _check_bytes("out", out)
    dev = rid.device
    sh = _stream_handle(stream)
    body_offsets = t.empty(n, dtype=t.int64, device=dev)
    body_lens = t.empty(n, dtype=t.int32, device=dev)
    types_out = t.empty(n, dtype=t.int16, device=dev)
    state = t.empty(n, dtype=t.uint8, device=dev)
    cbf = None if conn_first is None else t.empty(nconn + 1, dtype=t.int64, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)  # (the call always writes it)

    def run(dst, layout_only):
        outs = (None,) * 5 if layout_only else (_ptr(body_offsets), _ptr(body_lens), _ptr(types_out), _ptr(state), _ptr(cbf))
        check(_lib.rpc_frames_request_device(_ptr(method), _ptr(rid), _ptr(types), n, _ptr(table.names),
                                             table.names.numel(), _ptr(table.offsets), table.nmethods, _ptr(params),
                                             _count(params), _ptr(params_offsets), _ptr(params_lens),
                                             None if conn_first is None else conn_first.data_ptr(), nconn, _ptr(dst),
                                             _count(dst), *outs, total.data_ptr(), sh), "rpc_frames_request_device")

    out, size = _sized(run, total, out, stream, dev)
    return FrameRequest(out, body_offsets, body_lens, types_out, state, cbf, size)


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
    _check_tensors("n", n, (("method", method, 2), ("mode", mode, 1), ("status", status, 4), ("str_base", str_base, 8),
                            ("text_offsets", text_offsets, 8), ("text_lens", text_lens, 4)),
                   optional=("mode", "status", "str_base", "text_offsets", "text_lens"))
    for name, x in (("strings", strings), ("texts", texts), ("out", out)):
        if x is not None:
            _check_bytes(name, x)
    if params:
        _check_schema(schema)
    else:
        _check_bytes("result types", schema)
    dev = method.device
    sh = _stream_handle(stream)
    value_offsets = t.empty(n, dtype=t.int64, device=dev)
    value_lens = t.empty(n, dtype=t.int32, device=dev)
    state = t.empty(n, dtype=t.uint8, device=dev)
    reply_status = t.empty(n, dtype=t.int32, device=dev)
    ndefer = t.empty(1, dtype=t.int32, device=dev)
    total = t.empty(1, dtype=t.int64, device=dev)

    if params:
        sch = (None, _ptr(schema.first), schema.nmethods, _ptr(schema.types), _ptr(schema.name_off), schema.nparams,
               _ptr(schema.names), schema.names.numel())
    else:
        sch = (_ptr(schema), None, schema.numel(), None, None, 0, None, 0)

    def run(dst, layout_only):
        outs = (None,) * 5 if layout_only else (_ptr(value_offsets), _ptr(value_lens), _ptr(state), _ptr(reply_status),
                                                ndefer.data_ptr())
        check(_lib.rpc_frames_values_device(int(form), _ptr(mode), _ptr(status), _ptr(method), _ptr(slots), width, n, *sch,
                                            _ptr(strings), _count(strings), _ptr(str_base), _ptr(texts), _count(texts),
                                            _ptr(text_offsets), _ptr(text_lens), _ptr(dst), _count(dst), *outs,
                                            total.data_ptr(), sh), "rpc_frames_values_device")

    out, size = _sized(run, total, out, stream, dev)
    return FrameValues(out, value_offsets, value_lens, state, reply_status, ndefer, size)


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

    def run(cap, offs, conn, verdict, crc):
        common = (stream_buf.data_ptr(), nbytes, _ptr(conn_offsets), _ptr(conn_lengths), nconn, flags, _ptr(offs),
                  _ptr(conn), cap, conn_first.data_ptr(), _ptr(consumed), _ptr(state), nframes.data_ptr())
        if verdict is None:
            check(_lib.rpc_frames_scan_device(*common, sh), "rpc_frames_scan_device")
        else:
            check(_lib.rpc_frames_scan_verify_device(*common, _ptr(verdict), _ptr(crc), sh),
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
