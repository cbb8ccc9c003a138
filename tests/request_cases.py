"""Shared by test_request_emu.py, test_frames_request.py, test_request_golden.py and
test_request_fuzz.py: the rules of rpc_frames_request_device restated in plain Python (the
reference for all layers; nothing here shares code with rpc_amd/csrc/frames_request.h), and the
case tables the layers run.

Entry i = (type, method, id, params offset, params length), in this order (include/rpccrc.h,
frame request):

    1. types given and type != DATA:     size 0, type out = type, REQUEST_NONE
    2. method == NO_METHOD:              the value verbatim (RAW); empty: size 0, TYPE_NONE, REQUEST_NONE
    3. method >= nmethods, a table word that is not monotone or leaves method_bytes, a name with
       a byte < 0x20, `"` or `\\`:        size 0, TYPE_NONE, REQUEST_BAD_METHOD
    4. a value rules 2 and 5 look at that is not inside the params, or a body over 32 bits:
                                         size 0, TYPE_NONE, REQUEST_RANGE
    5. otherwise REQUEST_CALL:           {"jsonrpc":"2.0","method":"<name>","params":<value>,"id":<id>}
                                         {"jsonrpc":"2.0","method":"<name>","id":<id>}  (an empty value)

    body_offsets[i] = sum of the sizes before i; total = sum of all sizes
    an entry of non-zero size with offset + size > out_cap: not written, REQUEST_NO_ROOM, TYPE_NONE
"""
from typing import NamedTuple

import numpy as np

DATA, PING, PONG, TYPE_NONE = 0, 1, 2, 0xFFFF
NO_METHOD = 0xFFFF
Q_NONE, Q_CALL, Q_RAW, Q_BAD_METHOD, Q_RANGE, Q_NO_ROOM = range(6)
FILL = 0xA5
U64 = 1 << 64


class Table(NamedTuple):
    """A method table as the call takes it: the names back to back and nmethods + 1 words."""
    names: bytes
    offsets: list

    @property
    def nmethods(self):
        return len(self.offsets) - 1


def make_table(names):
    offs = [0]
    for nm in names:
        offs.append(offs[-1] + len(nm))
    return Table(b"".join(names), offs)


def name_of(table, m):
    """Name m, or None where rule 3 refuses it."""
    if m >= table.nmethods:
        return None
    a, b = table.offsets[m], table.offsets[m + 1]
    if a > b or b > len(table.names):
        return None
    name = table.names[a:b]
    if any(c < 0x20 or c in b'"\\' for c in name):
        return None
    return name


def call_body(name, value, rid):
    if value:
        return b'{"jsonrpc":"2.0","method":"%s","params":%s,"id":%d}' % (name, value, rid)
    return b'{"jsonrpc":"2.0","method":"%s","id":%d}' % (name, rid)


def rule(params, nbytes, table, typed, typ, method, rid, poff, plen):
    """Rules 1-5 for one entry: (size, body, type out, state).  params: the buffer, or None for
    a buffer of nbytes bytes that must not be read (the body is then None)."""
    if typed and typ != DATA:
        return 0, b"", typ, Q_NONE
    raw = method == NO_METHOD
    name = None
    if not raw:
        name = name_of(table, method)
        if name is None:
            return 0, b"", TYPE_NONE, Q_BAD_METHOD
    if not (poff <= nbytes and plen <= nbytes - poff):  # (Python integers: no wrap)
        return 0, b"", TYPE_NONE, Q_RANGE
    value = None if params is None else bytes(params[poff:poff + plen])
    if raw:
        return (plen, value, DATA, Q_RAW) if plen else (0, b"", TYPE_NONE, Q_NONE)
    size = (45 + len(name) + plen + len(str(rid))) if plen else (35 + len(name) + len(str(rid)))
    if size > 0xFFFFFFFF:
        return 0, b"", TYPE_NONE, Q_RANGE
    body = None if params is None else call_body(name, value, rid)
    assert body is None or len(body) == size
    return size, body, DATA, Q_CALL


class Expected(NamedTuple):
    body_offsets: list
    body_lens: list
    types: list
    status: list
    total: int
    conn_bytes_first: list  # [nconn + 1], or [] without a CSR
    out: bytes              # out_cap bytes, FILL where nothing is written
    chunks: list            # [n] the bytes of each entry, whatever out_cap is (None on a claimed buffer)


class Case(NamedTuple):
    name: str
    params: object      # bytes, or an int: a buffer of that many bytes that is never read (layout-only)
    table: Table
    entries: list       # [(type, method, id, params offset, params length)]
    conn_first: object  # list, or None
    typed: bool = True  # d_types given
    out_caps: tuple = (None,)  # None: exactly the total


def want_of(case, cap):
    params, nbytes = (None, case.params) if isinstance(case.params, int) else (case.params, len(case.params))
    lens, chunks, types, status = [], [], [], []
    for typ, method, rid, poff, plen in case.entries:
        ln, c, t, s = rule(params, nbytes, case.table, case.typed, typ, method, rid, poff, plen)
        lens.append(ln)
        chunks.append(c)
        types.append(t)
        status.append(s)
    offs = [0]
    for ln in lens:
        offs.append(offs[-1] + ln)
    total = offs.pop()
    lim = total if cap is None else cap
    out = bytearray([FILL]) * (lim if params is not None else 0)
    for i, ln in enumerate(lens):
        if not ln:
            continue
        if offs[i] + ln > lim:
            types[i], status[i] = TYPE_NONE, Q_NO_ROOM
        elif params is not None:
            out[offs[i]:offs[i] + ln] = chunks[i]
    cf = case.conn_first
    cbf = [] if cf is None else [(offs + [total])[min(k, len(lens))] for k in cf[:-1]] + [total]
    return Expected(offs, lens, types, status, total, cbf, bytes(out), chunks)


# ---- the case table -------------------------------------------------------------------------
IDS = (0, 9, 10, 2147483648, 4294967295)
NAME_LENS = (0, 1, 15, 16, 17)
LENS = tuple(range(34))
RAW_RUN = 20000   # one-byte RAW entries: a tile holds more entries than the LDS staging of 1,536
ZERO_RUN = 5000   # zero-size entries between two requests
FAR = U64 - 8     # an offset near 2^64: offset + length wraps

GOOD_NAMES = [b"", b"a", b"f" * 15, b"s" * 16, b"v" * 17, b"echo", b"caf\xc3\xa9"]
BAD_NAMES = [b"x\x1fy", b'q"r', b"b\\s"]
M_EMPTY, M_A, M_15, M_16, M_17, M_ECHO, M_CAFE = range(7)
M_BAD0 = 7


def main_table():
    """Names of 0, 1, 15, 16 and 17 bytes, one with bytes >= 0x80, three that need an escape, a
    legal name behind them, then a word that is not monotone and one that leaves method_bytes
    (which spoil their neighbours' words too)."""
    t = make_table(GOOD_NAMES + BAD_NAMES + [b"sum"])
    end = len(t.names)
    return Table(t.names, t.offsets + [end - 3, end + 5, end + 5])


M_SUM = 10
M_NONMONO, M_LEAVES, M_LEAVES2 = 11, 12, 13   # (end, end - 3), (end - 3, end + 5), (end + 5, end + 5)
METHOD_CLASSES = (M_ECHO, NO_METHOD, 14, 0xFFFE, M_BAD0, M_NONMONO)   # 14 == nmethods


def value_text(rng, n):
    """n bytes of JSON-looking text (any bytes would do: nothing is validated)."""
    return bytes(rng.choice(np.frombuffer(b'0123456789abcxyz"\\{}[]:, .-', dtype=np.uint8), n))


class _Pool:
    """The params buffer: values at chosen addresses mod 16."""

    def __init__(self, rng):
        self.rng, self.buf = rng, bytearray(value_text(rng, 3))

    def add(self, n, at=None):
        if at is not None:
            self.buf += value_text(self.rng, (at - len(self.buf)) % 16)
        off = len(self.buf)
        self.buf += value_text(self.rng, n)
        return off


def front_of(table, method, rid, plen):
    """Bytes in front of the copied ones."""
    return 0 if method == NO_METHOD else 38 + len(name_of(table, method))


def table_case(T, mis, seed=1):
    """One batch that meets the list's cases at tile size T with the output's address mis bytes
    past a 16-byte boundary."""
    rng = np.random.default_rng(seed * 1000 + T + mis)
    pool = _Pool(rng)
    table = main_table()
    assert table.nmethods == 14
    ents, conn = [], [0, 0]  # an empty connection at the start
    out_at = [0]

    def add(typ, method, rid, poff, plen):
        ents.append((typ, method, rid, poff, plen))
        out_at[0] += rule(pool.buf, len(pool.buf), table, True, typ, method, rid, poff, plen)[0]

    # every id beside every name, with and without params
    v5 = pool.add(5)
    for rid in IDS:
        for m in range(table.nmethods + 1):
            add(DATA, m, rid, v5, 5)
            add(DATA, m, rid, v5, 0)
    conn.append(len(ents))
    # every method class beside every type
    for typ in (DATA, PING, PONG, TYPE_NONE, 7):
        for m in METHOD_CLASSES:
            add(typ, m, 12345, v5 if typ == DATA else FAR, 5)
    conn.append(len(ents))
    # every (params address mod 16) x (copied bytes' output address mod 16) x length 0..33, as a
    # call and as a raw entry; RAW fillers of 1-15 bytes move the output on
    fill = pool.add(15)
    src = {(ln, sa): pool.add(ln, sa) for ln in LENS for sa in range(16)}
    k = 0
    for ln in LENS:
        for sa in range(16):
            for da in range(16):
                for method in (M_ECHO if k % 3 else M_17, NO_METHOD):
                    rid = IDS[k % 5]
                    k += 1
                    pad = (da - mis - out_at[0] - front_of(table, method, rid, ln)) % 16
                    if pad:
                        add(DATA, NO_METHOD, 0, fill, pad)
                    add(DATA, method, rid, src[ln, sa], ln)
    conn.append(len(ents))
    # a value of three tiles and a bit at an odd params offset, between small entries
    big_n = 40 * 1024 + 1 if T >= 4096 else 3 * T + 5
    big = pool.add(big_n, 7)
    add(DATA, M_CAFE, 7, big, big_n)
    add(DATA, M_A, 8, big + 1, 3 * 256 + 5)
    add(DATA, NO_METHOD, 0, big, big_n)
    # values outside the buffer: one byte past it, near 2^64, and an empty one past it
    outside = len(ents)  # (the buffer's size is known at the end: two of these are patched below)
    add(DATA, M_ECHO, 1, 0, 0)
    add(DATA, NO_METHOD, 1, FAR, 16)
    add(DATA, M_ECHO, 1, FAR, 16)
    add(DATA, M_ECHO, 1, 0, 0)
    conn.append(len(ents))
    one = pool.add(1)
    for _ in range(RAW_RUN):
        add(DATA, NO_METHOD, 0, one, 1)
    conn.append(len(ents))
    add(DATA, M_ECHO, 3, v5, 5)
    for i in range(ZERO_RUN):
        add(*((PING, M_ECHO, 1, FAR, 5), (TYPE_NONE, M_ECHO, 1, FAR, 5), (DATA, NO_METHOD, 0, v5, 0),
              (DATA, M_BAD0, 1, FAR, 5))[i % 4])
    add(DATA, M_ECHO, 4, v5, 5)
    last = pool.add(21)  # a value ending at the buffer's last byte, at an odd offset
    if last % 2 == 0:
        pool.buf.insert(last, 0x20)
        last += 1
    add(DATA, M_SUM, 5, last, 21)
    nb = len(pool.buf)
    assert last + 21 == nb and last % 2 == 1
    # (both patched entries had size 35 + 4 + 1 and now have size 0: nothing behind them needs
    # the addresses chosen above)
    ents[outside] = (DATA, M_ECHO, 1, nb - 4, 5)      # one byte outside
    ents[outside + 3] = (DATA, M_ECHO, 1, nb + 1, 0)  # an empty value past the end
    conn += [len(ents)] * 2  # an empty connection at the end
    return Case("table", bytes(pool.buf), table, ents, conn)


def long_name_case(T, mis):
    """One name of 4096 bytes that is the whole table, lying across a tile edge (with params:
    the front ends 4134 bytes in; without: the name is followed by the id at once)."""
    name = bytes(0x41 + (i * 7 + i // 26) % 26 for i in range(4096))
    table = make_table([name])
    params = b'[1,"two",{"three":3}]' + b"x" * T
    lead = (T - 100 - mis) % T or T  # the first request starts 100 bytes in front of a tile edge
    ents = [(DATA, NO_METHOD, 0, 0, lead), (DATA, 0, 4294967295, 0, 21), (DATA, 0, 0, 0, 0), (DATA, 0, 10, 3, 17),
            (DATA, 1, 1, 0, 21)]
    return Case("long_name", params, table, ents, [0, 2, len(ents)])


def small_cases(T, seed=2):
    rng = np.random.default_rng(seed * 1000 + T)
    pool = _Pool(rng)
    table = main_table()
    a, b, c = pool.add(40, 5), pool.add(33, 9), pool.add(18)
    ents = [(DATA, M_ECHO, 1, a, 40), (PING, M_ECHO, 0, FAR, 1), (DATA, M_17, 2147483648, b, 33), (DATA, NO_METHOD, 0, c, 18),
            (DATA, M_BAD0, 333, FAR, 0), (DATA, M_16, 4444, b, 33), (TYPE_NONE, NO_METHOD, 0, 0, 0)]
    params = bytes(pool.buf)
    case = Case("capacity", params, table, ents, [0, 2, 2, len(ents)])
    e = want_of(case, None)
    at = e.body_offsets
    caps = (None, e.total - 1,          # exactly at the end; inside the last entry's `,"id":` tail
            at[5] + 10, at[5] + 30,     # the last call: inside its front, inside its name
            at[5] + 60,                 # inside its value
            at[2] + e.body_lens[2] - 14,  # inside another's `,"id":`
            at[2] + e.body_lens[2],     # exactly at an entry's end
            at[3] + 5, 0)               # inside a RAW entry; nothing
    out = [case._replace(out_caps=caps)]
    out.append(case._replace(name="untyped", typed=False, out_caps=(None, at[2] + 3)))
    out.append(Case("one_call", params, table, [(DATA, M_ECHO, 9, a, 40)], [0, 1], out_caps=(None, 20, 0)))
    out.append(Case("one_bare", params, table, [(DATA, M_EMPTY, 0, 0, 0)], None, typed=False))
    out.append(Case("one_raw", params, table, [(DATA, NO_METHOD, 0, c, 1)], [0, 1]))
    out.append(Case("one_nothing", params, table, [(PONG, M_ECHO, 0, 0, 0)], [0, 1]))
    out.append(Case("one_range", params, table, [(DATA, NO_METHOD, 0, len(params), 1)], [0, 1]))
    out.append(Case("one_bad", params, table, [(DATA, 0xFFFE, 0, 0, 1)], [0, 1]))
    out.append(Case("n257", params, table, [(DATA, (M_ECHO, M_A, NO_METHOD)[i % 3], i * 16843009 % (1 << 32),
                                             a + i % 7, 1 + i % 30) for i in range(257)], [0, 100, 257]))
    out.append(Case("no_params", b"", table, [(DATA, M_ECHO, 1, 0, 0), (DATA, NO_METHOD, 2, 0, 0), (DATA, M_A, 3, 5, 5),
                                             (DATA, M_SUM, 4, 0, 1), (DATA, M_BAD0, 4, 0, 0)], [0, 5]))
    out.append(Case("no_table", params, Table(b"", [0]), [(DATA, 0, 1, a, 4), (DATA, NO_METHOD, 2, a, 4)], [0, 2]))
    out.append(long_name_case(T, 0))
    return out


def wide_cases():
    """Bodies at the 32-bit edge, on a params buffer that is only claimed (layout-only calls):
    45 + name + length + digits == 0xFFFFFFFF fits, one more does not."""
    nb = 1 << 33
    full = 0xFFFFFFFF
    table = main_table()
    ents = [(DATA, M_ECHO, 1, 5, full - 50), (DATA, M_ECHO, 1, 5, full - 49), (DATA, M_ECHO, 10, 5, full - 50),
            (DATA, NO_METHOD, 0, nb - full, full), (DATA, M_EMPTY, 4294967295, 0, full - 55),
            (DATA, M_EMPTY, 4294967295, 0, full - 54), (DATA, M_ECHO, 1, nb - 2, 3), (DATA, M_ECHO, 2, 0, 2)]
    return [Case("wide", nb, table, ents, [0, 3, len(ents)], out_caps=(0,))]


WIDE_LENS = [0xFFFFFFFF, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 52]
WIDE_STATUS = [Q_NO_ROOM, Q_RANGE, Q_RANGE, Q_NO_ROOM, Q_NO_ROOM, Q_RANGE, Q_RANGE, Q_NO_ROOM]


def all_cases(T, mis):
    return [table_case(T, mis)] + small_cases(T)
