"""Shared by test_reply_emu.py, test_frames_reply.py and test_reply_golden.py: the rules of
rpc_frames_reply_device restated in plain Python (the reference for all layers; nothing here
shares code with rpc_amd/csrc/frames_reply.h), and the case tables the layers run.

Entry i = (type, kind, id, status, value offset, value length), in this order
(include/rpccrc.h, frame reply):

    1. types given and type != DATA:        size 0, type out = type, REPLY_NONE
    2. kind NONE, RANGE or above:           size 0, TYPE_NONE, REPLY_NONE
    3. kind NOT_FOUND / INVALID:            the error form, code -32601 / -32600, the id
    4. kind CALL, s = status (0 without):   s == 0: the result form around the value (`null` when empty)
                                            s one of the five codes: the error form, its fixed message
                                            other s: the error form, the value as the message (`error` when empty)
    5. kind DEFER:                          the value verbatim (RAW); empty: size 0, TYPE_NONE, REPLY_NONE
    6. a value rules 4-5 look at that is not inside the values, or a body over 32 bits:
                                            size 0, TYPE_NONE, REPLY_RANGE

    body_offsets[i] = sum of the sizes before i; total = sum of all sizes
    an entry of non-zero size with offset + size > out_cap: not written, REPLY_NO_ROOM, TYPE_NONE
"""
from typing import NamedTuple

import numpy as np

DATA, PING, PONG, TYPE_NONE = 0, 1, 2, 0xFFFF
K_NONE, CALL, NOT_FOUND, INVALID, DEFER, K_RANGE = range(6)
R_NONE, R_RESULT, R_ERROR, R_RAW, R_RANGE, R_NO_ROOM = range(6)
FILL = 0xA5
MESSAGES = {-32700: b"Parse error", -32600: b"Invalid Request", -32601: b"Method not found",
            -32602: b"Invalid params", -32603: b"Internal error"}
U64 = 1 << 64


def result_body(rid, value):
    return b'{"jsonrpc":"2.0","id":%d,"result":%s}' % (rid, value or b"null")


def error_body(rid, code, message):
    return b'{"jsonrpc":"2.0","id":%d,"error":{"code":%d,"message":"%s"}}' % (rid, code, message)


def rule(values, nbytes, typed, typ, kind, rid, status, voff, vlen):
    """Rules 1-6 for one entry: (body, type out, state).  values: the buffer, or None for a
    buffer of nbytes bytes that must not be read (a body is then b"?" * its length)."""
    if typed and typ != DATA:
        return b"", typ, R_NONE
    if kind == K_NONE or kind >= K_RANGE:
        return b"", TYPE_NONE, R_NONE
    if kind == NOT_FOUND:
        return error_body(rid, -32601, MESSAGES[-32601]), DATA, R_ERROR
    if kind == INVALID:
        return error_body(rid, -32600, MESSAGES[-32600]), DATA, R_ERROR
    if kind == CALL and status in MESSAGES:
        return error_body(rid, status, MESSAGES[status]), DATA, R_ERROR
    if not (voff <= nbytes and vlen <= nbytes - voff):  # (Python integers: no wrap)
        return b"", TYPE_NONE, R_RANGE
    value = b"?" * vlen if values is None else bytes(values[voff:voff + vlen])
    if kind == DEFER:
        return (value, DATA, R_RAW) if value else (b"", TYPE_NONE, R_NONE)
    body = result_body(rid, value) if status == 0 else error_body(rid, status, value or b"error")
    if len(body) > 0xFFFFFFFF:
        return b"", TYPE_NONE, R_RANGE
    return body, DATA, R_RESULT if status == 0 else R_ERROR


class Expected(NamedTuple):
    body_offsets: list
    body_lens: list
    types: list
    status: list
    total: int
    conn_bytes_first: list  # [nconn + 1], or [] without a CSR
    out: bytes              # out_cap bytes, FILL where nothing is written
    chunks: list            # [n] the bytes of each entry, whatever out_cap is


class Case(NamedTuple):
    name: str
    values: object      # bytes, or an int: a buffer of that many bytes that is never read (layout-only)
    entries: list       # [(type, kind, id, status, value offset, value length)]
    conn_first: object  # list, or None
    typed: bool = True  # d_reply_types given
    kinded: bool = True  # d_kind given
    stated: bool = True  # d_status given
    out_caps: tuple = (None,)  # None: exactly the total


def want_of(case, cap):
    values, nbytes = (None, case.values) if isinstance(case.values, int) else (case.values, len(case.values))
    chunks, types, status = [], [], []
    for typ, kind, rid, st, voff, vlen in case.entries:
        c, t, s = rule(values, nbytes, case.typed, typ, kind if case.kinded else CALL, rid, st if case.stated else 0,
                       voff, vlen)
        chunks.append(c)
        types.append(t)
        status.append(s)
    offs = [0]
    for c in chunks:
        offs.append(offs[-1] + len(c))
    total = offs.pop()
    lim = total if cap is None else cap
    out = bytearray([FILL]) * (lim if values is not None else 0)
    for i, c in enumerate(chunks):
        if not c:
            continue
        if offs[i] + len(c) > lim:
            types[i], status[i] = TYPE_NONE, R_NO_ROOM
        elif values is not None:
            out[offs[i]:offs[i] + len(c)] = c
    cf = case.conn_first
    cbf = [] if cf is None else [(offs + [total])[min(k, len(chunks))] for k in cf[:-1]] + [total]
    return Expected(offs, [len(c) for c in chunks], types, status, total, cbf, bytes(out), chunks)


# ---- the case table -------------------------------------------------------------------------
IDS = (0, 9, 10, 4294967295)
CODES = (-32700, -32600, -32601, -32602, -32603, 1, -1, 2147483647, -2147483648, -32000, -32604, -32599)
LENS = (0, 1, 15, 16, 17, 31, 33)
RAW_RUN = 20000   # one-byte RAW entries: a tile holds more entries than the LDS staging of 1,536
ZERO_RUN = 5000   # zero-size entries between two results
FAR = U64 - 8     # an offset near 2^64: offset + length wraps


def value_text(rng, n):
    """n bytes of JSON-looking text (any bytes would do: nothing is validated)."""
    return bytes(rng.choice(np.frombuffer(b'0123456789abcxyz"\\{}[]:, .-', dtype=np.uint8), n))


class _Pool:
    """The values buffer: values at chosen addresses mod 16."""

    def __init__(self, rng):
        self.rng, self.buf = rng, bytearray(value_text(rng, 3))

    def add(self, n, at=None):
        if at is not None:
            self.buf += value_text(self.rng, (at - len(self.buf)) % 16)
        off = len(self.buf)
        self.buf += value_text(self.rng, n)
        return off


def table_case(T, mis, seed=1):
    """One batch that meets every case of the list at tile size T with the output's address
    mis bytes past a 16-byte boundary."""
    rng = np.random.default_rng(seed * 1000 + T + mis)
    pool = _Pool(rng)
    ents, conn = [], [0, 0]  # an empty connection at the start
    out_at = [0]  # output bytes so far (d_reply_types, d_kind and d_status all given)

    def add(typ, kind, rid, status, voff, vlen):
        ents.append((typ, kind, rid, status, voff, vlen))
        out_at[0] += len(rule(pool.buf, len(pool.buf), True, typ, kind, rid, status, voff, vlen)[0])

    # every id beside every code, and beside a result
    v5 = pool.add(5)
    for rid in IDS:
        add(DATA, CALL, rid, 0, v5, 5)
        for code in CODES:
            add(DATA, CALL, rid, code, v5, 5)
        add(DATA, NOT_FOUND, rid, 77, FAR, 9)   # (neither the status nor the value is looked at)
        add(DATA, INVALID, rid, 0, FAR, 9)
    conn.append(len(ents))
    # every kind beside every reply_types value
    for typ in (DATA, PING, PONG, TYPE_NONE, 7):
        for kind in (K_NONE, CALL, NOT_FOUND, INVALID, DEFER, K_RANGE, 6, 255):
            add(typ, kind, 12345, 0, v5 if typ == DATA else FAR, 5)
    conn.append(len(ents))
    # every (value address mod 16) x (copied bytes' output address mod 16) x length, the three
    # copying forms in turn; RAW fillers of 1-15 bytes move the output on
    fill = pool.add(15)
    src = {(ln, sa): pool.add(ln, sa) for ln in LENS for sa in range(16)}
    k = 0
    for ln in LENS:
        for sa in range(16):
            for da in range(16):
                kind, status = ((CALL, 0), (CALL, -5), (DEFER, 0))[k % 3]
                rid = IDS[k % 4]
                k += 1
                front = 0 if kind == DEFER else len(result_body(rid, b"x")) - 2 if status == 0 else \
                    len(error_body(rid, status, b"")) - 3
                pad = (da - mis - out_at[0] - front) % 16
                if pad:
                    add(DATA, DEFER, 0, 0, fill, pad)
                add(DATA, kind, rid, status, src[ln, sa], ln)
    conn.append(len(ents))
    # a value of three tiles and a bit at an odd values offset, between small entries
    big = pool.add(40001 if T >= 4096 else 3 * T + 5, 7)
    add(DATA, CALL, 7, 0, big, 40001 if T >= 4096 else 3 * T + 5)
    add(DATA, CALL, 8, 1, big + 1, 3 * 256 + 5)
    add(DATA, DEFER, 0, 0, big, 40001 if T >= 4096 else 3 * T + 5)
    # values outside the buffer: one byte past it, near 2^64, and an empty one past it
    outside = len(ents)  # (the buffer's size is known at the end: two of these are patched below)
    add(DATA, CALL, 1, 0, 0, 0)
    add(DATA, DEFER, 1, 0, FAR, 16)
    add(DATA, CALL, 1, -7, FAR, 16)
    add(DATA, CALL, 1, 0, 0, 0)
    conn.append(len(ents))
    one = pool.add(1)
    for _ in range(RAW_RUN):
        add(DATA, DEFER, 0, 0, one, 1)
    conn.append(len(ents))
    add(DATA, CALL, 3, 0, v5, 5)
    for i in range(ZERO_RUN):
        add(*((PONG, CALL, 1, 0, FAR, 5), (TYPE_NONE, CALL, 1, 0, FAR, 5), (DATA, DEFER, 0, 0, v5, 0))[i % 3])
    add(DATA, CALL, 4, 0, v5, 5)
    last = pool.add(21)  # a value ending at the buffer's last byte, at an odd offset
    if last % 2 == 0:
        pool.buf.insert(last, 0x20)
        last += 1
    add(DATA, CALL, 5, 0, last, 21)
    nb = len(pool.buf)
    assert last + 21 == nb and last % 2 == 1
    ents[outside] = (DATA, CALL, 1, 0, nb - 4, 5)      # one byte outside
    ents[outside + 3] = (DATA, CALL, 1, 0, nb + 1, 0)  # an empty value past the end
    conn += [len(ents)] * 2  # an empty connection at the end
    return Case("table", bytes(pool.buf), ents, conn)


def small_cases(T, seed=2):
    rng = np.random.default_rng(seed * 1000 + T)
    pool = _Pool(rng)
    a, b, c = pool.add(40, 5), pool.add(33, 9), pool.add(18)
    ents = [(DATA, CALL, 1, 0, a, 40), (PONG, CALL, 0, 0, FAR, 1), (DATA, CALL, 22, -9, b, 33), (DATA, DEFER, 0, 0, c, 18),
            (DATA, NOT_FOUND, 333, 0, FAR, 0), (DATA, CALL, 4444, 0, b, 33), (TYPE_NONE, K_NONE, 0, 0, 0, 0)]
    values = bytes(pool.buf)
    case = Case("capacity", values, ents, [0, 2, 2, len(ents)])
    e = want_of(case, None)
    at = e.body_offsets
    caps = (None, e.total - 1,          # exactly at the end; inside the last entry's suffix
            at[5] + 10, at[5] + 40,     # the last result: inside its prefix, inside its value
            at[2] + e.body_lens[2] - 2,  # the custom error: inside its suffix
            at[2] + e.body_lens[2],     # exactly at an entry's end
            at[3] + 5, 0)               # inside a RAW entry; nothing
    out = [case._replace(out_caps=caps)]
    for flags in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        out.append(case._replace(name="null_%d%d%d" % flags, typed=flags[0], kinded=flags[1], stated=flags[2],
                                 out_caps=(None, at[2] + 3)))
    out.append(Case("one_result", values, [(DATA, CALL, 9, 0, a, 40)], [0, 1], out_caps=(None, 20, 0)))
    out.append(Case("one_error", values, [(DATA, INVALID, 0, 0, FAR, 0)], None))
    out.append(Case("one_raw", values, [(DATA, DEFER, 0, 0, c, 1)], [0, 1]))
    out.append(Case("one_nothing", values, [(PONG, CALL, 0, 0, 0, 0)], [0, 1]))
    out.append(Case("one_range", values, [(DATA, DEFER, 0, 0, len(values), 1)], [0, 1]))
    out.append(Case("no_values", b"", [(DATA, CALL, 1, 0, 0, 0), (DATA, CALL, 2, -32603, 5, 5), (DATA, CALL, 3, 3, 0, 0),
                                       (DATA, DEFER, 0, 0, 0, 0), (DATA, CALL, 4, 0, 0, 1)], [0, 5]))
    return out


def wide_cases():
    """Bodies at the 32-bit edge, on a values buffer that is only claimed (layout-only calls):
    front + length + suffix == 0xFFFFFFFF fits, one more does not."""
    nb = 1 << 33
    full = 0xFFFFFFFF
    ents = [(DATA, CALL, 1, 0, 5, full - 34), (DATA, CALL, 1, 0, 5, full - 33), (DATA, CALL, 10, 0, 5, full - 34),
            (DATA, DEFER, 0, 0, nb - full, full), (DATA, CALL, 1, -1, 0, full - 57), (DATA, CALL, 1, -1, 0, full - 56),
            (DATA, CALL, 1, 0, nb - 2, 3), (DATA, CALL, 2, 0, 0, 2)]
    return [Case("wide", nb, ents, [0, 3, len(ents)], out_caps=(0,))]


def all_cases(T, mis):
    return [table_case(T, mis)] + small_cases(T)
