"""Shared by test_scan_emu.py and test_frames_scan.py: the frame walk of
rpc_frames_scan_device restated in plain Python (the reference for both), the
categories a walk went through, and builders for connections that hit them.

The walk (include/rpccrc.h, frame scan):

    p = 0; state = OPEN
    loop:
      if len - p < 12: stop                      # clean end (p == len) or partial header
      read type, body_len at p (big-endian, rpc.h:3-8)
      if control (PING at a server, PONG at a client): emit p; p += 12; continue
      if body_len > 1024 and not lift_cap:        emit p; p += 12; state = CLOSED; stop
      if body_len == 0 and role == client:        emit p; p += 12; state = CLOSED; stop
      if len - (p + 12) < body_len: stop          # partial body: not emitted
      emit p; p += 12 + body_len
    consumed = p
"""
import struct
import zlib

import numpy as np

HDR = 12
MAX_BODY = 1024
E = HDR + MAX_BODY
OPEN, CLOSED = 0, 1
PING, PONG = 1, 2


def walk(buf, off, length, role="server", lift_cap=False, tile=None, cats=None):
    """The plain walk over connection buf[off : off + length] (buf: bytes).  Returns
    (absolute frame offsets, consumed, state).  With ``cats`` (a dict of counters) and
    ``tile`` (T) it also records which categories this walk met, positions being
    relative to the connection's start."""
    if off > len(buf) or length > len(buf) - off:
        return [], 0, CLOSED
    control = PING if role == "server" else PONG
    frames, p, state = [], 0, OPEN
    note = (lambda k, v=1: cats.__setitem__(k, cats.get(k, 0) + v)) if cats is not None else (lambda k, v=1: None)
    T = tile
    while True:
        if length - p < HDR:
            note("end_clean" if p == length else "end_in_header")
            break
        typ, bl = struct.unpack_from(">HI", buf, off + p + 2)
        straddle = T is not None and p % T + HDR > T  # header split across a tile edge
        if straddle:
            note("split_far_%d" % ((p % T + HDR) - T))
        if typ == control:
            note("control")
            if straddle:
                note("control_straddles")
            frames.append(off + p)
            if T is not None and (p + HDR) // T > p // T:
                note("exit_%d" % ((p + HDR) % T))
            p += HDR
            continue
        if (bl > MAX_BODY and not lift_cap) or (bl == 0 and role == "client"):
            note("close_too_large" if bl else "close_empty")
            if T is not None and p % T >= T - HDR:
                note("close_last_in_tile")
            frames.append(off + p)
            p += HDR
            state = CLOSED
            break
        if length - (p + HDR) < bl:
            note("end_in_body")
            break
        if T is not None and not lift_cap and (p + HDR + bl) // T > p // T:
            # the chain leaves this tile x bytes into the next: 0 = a body ending exactly at
            # the tile's end, 1035 = a 1024-byte body whose frame starts at its last byte
            note("exit_%d" % ((p + HDR + bl) % T))
        note("data")
        frames.append(off + p)
        p += HDR + bl
    return frames, p, state


def decoys(buf, off, length, frames):
    """Positions of the connection that look like a header of an in-cap data or
    heartbeat frame (version 1, type <= 2, body_len <= 1024) and are NOT on the
    true chain: where a chain from a wrong entry can plausibly run."""
    a = np.frombuffer(buf, dtype=np.uint8, count=length, offset=off)
    if length < HDR:
        return 0
    n = length - HDR + 1
    look = ((a[0:n] == 0) & (a[1:n + 1] == 1) & (a[2:n + 2] == 0) & (a[3:n + 3] <= 2) & (a[4:n + 4] == 0)
            & (a[5:n + 5] == 0) & ((a[6:n + 6].astype(np.uint32) << 8 | a[7:n + 7]) <= MAX_BODY))
    true = np.asarray(frames, dtype=np.int64) - off
    true = true[true < n]
    return int(look.sum()) - int(look[true].sum())


def frame(body=b"", typ=0, blen=None, crc=None, version=1):
    """One wire frame; blen / crc override what the header claims."""
    return struct.pack(">HHII", version, typ, len(body) if blen is None else blen,
                       zlib.crc32(body) if crc is None else crc) + body


def rand_body(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def decoy_body(rng, n):
    """A body of n bytes holding whole well-formed frames (and a header whose body
    runs out of it), so that a chain started inside it keeps going."""
    out = b""
    while len(out) < n:
        room = n - len(out)
        if room < HDR:
            out += rand_body(rng, room)
        elif room < 40:
            out += frame(rand_body(rng, room - HDR))
        else:
            k = int(rng.integers(0, min(room - HDR, 300) + 1))
            out += frame(rand_body(rng, k), typ=int(rng.choice([0, 0, 0, PING, PONG, 7])))
    return out[:n]


def filler(rng, nbytes, role="server", decoy_every=3):
    """Frames that keep the chain open, nbytes in all (0, or >= 12): data frames
    (every few of them with decoys inside), heartbeats, empty bodies at a server."""
    control = PING if role == "server" else PONG
    other = PONG if role == "server" else PING
    assert nbytes == 0 or nbytes >= HDR
    out, left, i = [], nbytes, 0

    def sized(a):  # a frame of a bytes in all, 12 <= a <= 1036
        if a == HDR:
            return frame(b"", typ=control, blen=int(rng.integers(0, 2000)), crc=int(rng.integers(0, 2**32)))
        body = decoy_body(rng, a - HDR) if i % decoy_every == 0 else rand_body(rng, a - HDR)
        return frame(body, typ=int(rng.choice([0, 0, 0, 9, other])))

    while left:
        if left > 2 * E:  # plenty of room: any frame
            kind = int(rng.integers(0, 8))
            if kind == 0:
                f = sized(HDR)
            elif kind == 1 and role == "server":
                f = frame(b"", crc=int(rng.integers(0, 2)))  # an empty body is a data frame at a server
            else:
                f = sized(HDR + (int(rng.integers(1, MAX_BODY + 1)) if kind != 2 else MAX_BODY))
        elif left > E:  # two more frames
            f = sized(int(rng.integers(max(HDR, left - E), min(E, left - HDR) + 1)))
        else:
            f = sized(left)
        out.append(f)
        left -= len(f)
        i += 1
    assert sum(map(len, out)) == nbytes
    return b"".join(out)


def closing(rng, role):
    """A header that closes the connection (over the cap; or empty at a client)."""
    if role == "client" and rng.integers(0, 2):
        return frame(b"", typ=int(rng.choice([0, PING, 5])), crc=int(rng.integers(0, 2**32)))
    return frame(b"", blen=int(rng.integers(MAX_BODY + 1, 2**32)), crc=7)


ENDINGS = ("clean", "in_header", "in_body", "close")


def random_conn(rng, nbytes, role="server", lift_cap=False, ending=None):
    """A connection of about nbytes bytes of mixed frames with the given ending."""
    ending = ending or ENDINGS[int(rng.integers(0, len(ENDINGS)))]
    body = filler(rng, nbytes, role) if nbytes >= HDR else b""
    if lift_cap and len(body) >= 4 * HDR:  # a frame over the cap that the lifted cap walks through
        big = frame(rand_body(rng, int(rng.integers(MAX_BODY + 1, 3000))))
        body = body + big + filler(rng, 3 * HDR, role)
    if ending == "clean":
        return body
    if ending == "in_header":
        return body + frame(rand_body(rng, 20))[:int(rng.integers(1, HDR))]
    if ending == "in_body":
        f = frame(rand_body(rng, int(rng.integers(1, MAX_BODY + 1))))
        return body + f[:int(rng.integers(HDR, len(f)))]
    tail = filler(rng, 5 * HDR + 40, role)  # behind a closing header nothing is looked at
    if lift_cap and role == "server":  # (nothing closes a server's connection with the cap lifted)
        return body + tail
    return body + closing(rng, role) + tail


def place(rng, parts, cur, target, role):
    """Filler so that the next frame starts at connection offset `target`."""
    gap = target - cur
    assert gap == 0 or gap >= HDR, (cur, target)
    parts.append(filler(rng, gap, role))
    return target


def crafted_conn(rng, T, role="server", ending="clean"):
    """A connection whose true chain meets every tile-edge case at tile size T: each
    header split 1..11 bytes across an edge, a heartbeat straddling one, a body
    ending exactly at a tile end (exit 0), a 1024-byte body starting at a tile's last
    byte (exit 1035); then the ending: "close" puts a closing header as the last 12
    bytes of a tile."""
    control = PING if role == "server" else PONG
    parts, cur, edge = [], 0, T * (1 + (2 * E + 4 * HDR) // T)
    step = T * (1 + (2 * E + 4 * HDR) // T)

    def put(start, f):
        nonlocal cur
        cur = place(rng, parts, cur, start, role)
        parts.append(f)
        cur += len(f)

    for far in range(1, HDR):
        put(edge - (HDR - far), frame(decoy_body(rng, int(rng.integers(1, MAX_BODY + 1)))))
        edge += step
    put(edge - 5, frame(b"", typ=control, blen=77, crc=0x01020304))
    edge += step
    n = int(rng.integers(1, MAX_BODY + 1))
    put(edge - HDR - n, frame(rand_body(rng, n)))
    edge += step
    put(edge - 1, frame(decoy_body(rng, MAX_BODY)))
    edge += step
    if ending == "close":
        put(edge - HDR, closing(rng, "server"))  # over the cap: closes either role
        parts.append(filler(rng, 2 * E, role))
    elif ending == "in_header":
        parts.append(filler(rng, 3 * E, role) + frame(b"abc")[:7])
    elif ending == "in_body":
        parts.append(filler(rng, 3 * E, role) + frame(rand_body(rng, 500))[:300])
    else:
        parts.append(filler(rng, 3 * E, role))
    return b"".join(parts)


def layout(rng, conns, gap_max=9):
    """Connections at unaligned, non-adjacent offsets of one stream (junk between them)."""
    blob, offs = bytearray(rand_body(rng, int(rng.integers(1, gap_max + 1)))), []
    for c in conns:
        offs.append(len(blob))
        blob += c
        blob += rand_body(rng, int(rng.integers(1, gap_max + 1)))
    return bytes(blob), np.array(offs, dtype=np.uint64), np.array([len(c) for c in conns], dtype=np.uint64)


def expected(blob, offs, lens, role, lift_cap, tile=None, want_decoys=True):
    """The plain walk over every connection: (frame offsets, frame conn, conn_first,
    consumed, state, categories)."""
    cats, fo, fc, first, consumed, state = {}, [], [], [0], [], []
    for c, (o, n) in enumerate(zip(offs.tolist(), lens.tolist())):
        f, p, s = walk(blob, o, n, role, lift_cap, tile, cats)
        if want_decoys and f and decoys(blob, o, n, f):
            cats["decoys"] = cats.get("decoys", 0) + 1
        fo += f
        fc += [c] * len(f)
        first.append(len(fo))
        consumed.append(p)
        state.append(s)
    return fo, fc, first, consumed, state, cats
