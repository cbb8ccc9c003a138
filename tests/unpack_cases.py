"""Shared by test_unpack_emu.py and test_frames_unpack.py: the rules of
rpc_frames_unpack_device restated in plain Python (the reference for both), built on
scan_cases.frame, and the case tables both layers run.

For entry i = (frame offset, verdict v), in this order (include/rpccrc.h, frame unpack):

    1. v not in (OK, CONTROL):          size 0, NONE, version 0, length 0, verdict out v
                                        (the offset is not looked at)
    2. header not inside the stream:    size 0, NONE, version 0, length 0, MALFORMED
    3. version, type, body_len big-endian; ctl = PING at a server, PONG at a client;
       every contradiction below: as rule 2
    4. v == CONTROL: type != ctl is a contradiction; else size 0, length 0, the header's
       version, CONTROL, reply type PONG at a server / NONE at a client
    5. v == OK: type == ctl, body_len > 1024 without lift_cap, body_len 0 at a client, a
       body not inside the stream are contradictions; else size body_len + nul, length
       body_len, the header's version, DATA, OK

    body_offsets[i] = sum of the sizes before i; total = sum of all sizes
    an entry of non-zero size with offset + size > out_cap: not written, MALFORMED, NONE
    (offset, length and version keep their values)
"""
import struct
from typing import NamedTuple

import numpy as np

import scan_cases as sc

HDR = 12
MAX_BODY = 1024
DATA, PING, PONG, NONE = 0, 1, 2, 0xFFFF
BAD_CRC, OK, CONTROL, TOO_LARGE, MALFORMED, RECV_ERR, NOT_REACHED, SKIPPED = range(8)
FILL = 0xA5
FAR = 1 << 40  # an offset that must never be looked at


class Expected(NamedTuple):
    body_offsets: list  # [n]
    body_lens: list     # [n]
    reply_types: list   # [n]
    versions: list      # [n]
    verdict: list       # [n], with the capacity downgrade
    total: int
    conn_bytes_first: list  # [nconn + 1], or [] without a CSR
    out: bytes          # out_cap bytes, FILL where nothing is written
    chunks: list        # [n] the output bytes of each entry (b"" for size 0), whatever out_cap is


def rule(stream, off, v, role, lift_cap, nul):
    """Rules 1-5 for one entry: (chunk, length, version, reply type, verdict)."""
    nothing = (b"", 0, 0, NONE)
    if v not in (OK, CONTROL):
        return nothing + (v,)
    nb = len(stream)
    if not (off <= nb and HDR <= nb - off):
        return nothing + (MALFORMED,)
    version, typ, blen = struct.unpack_from(">HHI", stream, off)
    ctl = PING if role == "server" else PONG
    if v == CONTROL:
        if typ != ctl:
            return nothing + (MALFORMED,)
        return b"", 0, version, PONG if role == "server" else NONE, CONTROL
    if typ == ctl or (blen > MAX_BODY and not lift_cap) or (blen == 0 and role == "client") or blen > nb - off - HDR:
        return nothing + (MALFORMED,)
    return bytes(stream[off + HDR:off + HDR + blen]) + b"\0" * nul, blen, version, DATA, OK


def expected(stream, offsets, verdicts, conn_first=None, role="server", lift_cap=False, nul=1, out_cap=None):
    """The rules above over entries (offsets[i], verdicts[i]); out_cap None: the total."""
    assert role in ("server", "client") and nul in (0, 1)
    chunks, lens, vers, types, verdict = [], [], [], [], []
    for off, v in zip(offsets, verdicts):
        c, ln, ver, typ, vo = rule(stream, off, v, role, lift_cap, nul)
        chunks.append(c)
        lens.append(ln)
        vers.append(ver)
        types.append(typ)
        verdict.append(vo)
    offs = [0]
    for c in chunks:
        offs.append(offs[-1] + len(c))
    total = offs.pop()
    cap = total if out_cap is None else out_cap
    out = bytearray([FILL]) * cap
    for i, c in enumerate(chunks):
        if not c:
            continue
        if offs[i] + len(c) > cap:
            verdict[i], types[i] = MALFORMED, NONE
        else:
            out[offs[i]:offs[i] + len(c)] = c
    cbf = [] if conn_first is None else [(offs + [total])[min(k, len(chunks))] for k in conn_first[:-1]] + [total]
    return Expected(offs, lens, types, vers, verdict, total, cbf, bytes(out), chunks)


class Case(NamedTuple):
    name: str
    stream: bytes
    entries: list       # [(frame offset, verdict)]
    conn_first: object  # list, or None
    role: str
    lift_cap: bool
    nul: int
    out_caps: list      # None: exactly the total


def want_of(case, cap):
    off, v = zip(*case.entries) if case.entries else ((), ())
    return expected(case.stream, off, v, case.conn_first, case.role, case.lift_cap, case.nul, cap)


class _Builder:
    """A stream that is a pool of frames -- entries may name them in any order and more than
    once -- and a list of entries laid out so that chosen bodies land at chosen output offsets."""

    def __init__(self, rng, role, nul):
        self.rng, self.role, self.nul = rng, role, nul
        self.ctl = PING if role == "server" else PONG
        self.other = PONG if role == "server" else PING
        self.stream = bytearray(sc.rand_body(rng, 3))
        self.entries = []
        self.cur = 0  # output bytes so far
        self.pool = {}  # body length -> frame offset, for the fillers
        self.smin = nul + (1 if role == "client" else 0)  # the smallest non-zero size that can be delivered
        for ln in list(range(0, 65)) + [MAX_BODY]:
            self.pool[ln] = self.frame(sc.rand_body(rng, ln), typ=int(rng.choice([0, 0, 7, self.other])),
                                       version=int(rng.integers(0, 1 << 16)))

    def frame(self, body, typ=0, version=1, body_at=None, blen=None):
        """Appends a frame (junk in front so that its body starts at a stream offset that is
        body_at mod 16); returns its offset."""
        if body_at is not None:
            self.stream += sc.rand_body(self.rng, (body_at - (len(self.stream) + HDR)) % 16)
        off = len(self.stream)
        self.stream += sc.frame(body, typ=typ, version=version, blen=blen, crc=int(self.rng.integers(0, 1 << 32)))
        return off

    def size_of(self, off):
        """Bytes entry (off, OK) delivers."""
        return len(rule(self.stream, off, OK, self.role, True, self.nul)[0])

    def ok(self, off):
        self.entries.append((off, OK))
        self.cur += self.size_of(off)

    def filler(self, nbytes):
        """Pool entries that deliver nbytes bytes in all (0, or >= smin)."""
        assert nbytes == 0 or nbytes >= self.smin, nbytes
        left, nul, smin = nbytes, self.nul, self.smin
        while left:
            for ln in (MAX_BODY, 64, 60):
                rest = left - (ln + nul)
                if rest == 0 or rest >= max(smin, 1):
                    break
            else:
                ln = left - nul
            assert 0 <= ln <= MAX_BODY and (ln + nul) >= max(smin, 1), (left, ln)
            self.ok(self.pool[ln])
            left -= ln + nul
        return nbytes

    def goto(self, target, step=16):
        """Filler so that the next entry starts at output offset target (moved on by `step`
        while the gap is too small to fill)."""
        while target - self.cur != 0 and target - self.cur < max(self.smin, 1):
            target += step
        self.filler(target - self.cur)
        assert self.cur == target
        return target

    def control(self, version=1):
        self.entries.append((self.frame(b"", typ=self.ctl, version=version, blen=int(self.rng.integers(0, 2000))), CONTROL))

    def nothing(self, v):
        self.entries.append((FAR + int(self.rng.integers(0, 1 << 20)), v))


NOT_DELIVERED = (BAD_CRC, TOO_LARGE, MALFORMED, RECV_ERR, NOT_REACHED, SKIPPED, 200)
TABLE_LENS = (0, 1, 15, 16, 17, 1024)
EMPTY_RUN = 2000


def table_case(T, mis, role="server", nul=1, seed=1):
    """One batch that meets every layout case at tile size T with the output's address mis
    bytes past a 16-byte boundary (tile edges lie at output offsets m * T - mis)."""
    rng = np.random.default_rng(seed * 1000 + T + mis + 7 * nul + (role == "client"))
    b = _Builder(rng, role, nul)
    conn = [0, 0]  # an empty connection at the start
    for v in (NOT_REACHED, MALFORMED, BAD_CRC):  # a run of nothing at the very start
        b.nothing(v)
    first = b.frame(sc.rand_body(rng, 37), body_at=5)
    b.ok(first)
    conn.append(len(b.entries))
    # every (body start in the stream mod 16) x (body start in the output mod 16), six lengths
    src = {(ln, sa): b.frame(sc.rand_body(rng, ln), body_at=sa, version=1 + sa) for ln in TABLE_LENS for sa in range(16)}
    for ln in TABLE_LENS:
        for sa in range(16):
            assert (src[ln, sa] + HDR) % 16 == sa
            for da in range(16):
                pad = (da - mis - b.cur) % 16
                if pad and pad < b.smin:
                    pad += 16
                b.filler(pad)
                assert (b.cur + mis) % 16 == da
                b.ok(src[ln, sa])
        conn.append(len(b.entries))

    def edge(back):
        """The first tile edge (output offset m * T - mis) that an entry starting `back` bytes
        before it can still be placed in front of."""
        m = -(-(b.cur + b.smin + back + mis) // T)
        return m * T - mis - back

    big = b.frame(sc.rand_body(rng, 300), body_at=3)
    b.goto(edge(300 + nul), step=T)  # an entry ending exactly on a tile edge ...
    b.ok(big)
    assert (b.cur + mis) % T == 0
    b.ok(big)  # ... and one starting on it
    if nul:  # body bytes ending on the edge, the NUL behind it
        b.goto(edge(300), step=T)
        b.ok(big)
        assert (b.cur + mis) % T == 1
    conn.append(len(b.entries))
    for v in NOT_DELIVERED:  # one entry of every verdict that delivers nothing
        b.nothing(v)
    for i in range(40):  # a run of heartbeats
        b.control(version=1 + i % 3)
    conn.append(len(b.entries))
    b.ok(b.frame(sc.rand_body(rng, 9), typ=b.other))  # the other heartbeat type is a data frame
    empty = b.frame(b"", body_at=int(rng.integers(0, 16)))
    for i in range(EMPTY_RUN):  # empty bodies: 1-byte entries at a server with nul, else nothing
        b.ok(empty)
    conn.append(len(b.entries))
    b.ok(first)
    last = b.frame(sc.rand_body(rng, 21))  # a body ending at the stream's last byte
    b.ok(last)
    nbytes = len(b.stream)
    for i in range(5):  # padding entries, as the scan leaves them
        b.entries.append((nbytes, MALFORMED))
    conn += [len(b.entries) - 5] * 2  # an empty connection at the end (the CSR ends before the padding)
    return Case("table", bytes(b.stream), b.entries, conn, role, False, nul, [None])


def lying_cases(role="server", nul=1, seed=3):
    """One entry each whose verdict the stream contradicts; `truth` entries around it."""
    rng = np.random.default_rng(seed)
    ctl, other = (PING, PONG) if role == "server" else (PONG, PING)
    good = sc.frame(sc.rand_body(rng, 50), version=7)
    out = []

    def case(name, stream, off, v):
        out.append(Case(name, bytes(stream), [(0, OK), (off, v), (0, OK)], [0, 3], role, False, nul, [None]))

    case("header_past_end", good + sc.frame(b"xy")[:11], len(good), OK)
    case("header_far", good, FAR, OK)
    case("body_past_end", good + sc.frame(sc.rand_body(rng, 40))[:-1], len(good), OK)
    case("over_cap", good + sc.frame(sc.rand_body(rng, MAX_BODY + 1)), len(good), OK)
    case("ok_on_control", good + sc.frame(b"", typ=ctl) + sc.rand_body(rng, 30), len(good), OK)
    case("control_on_data", good + sc.frame(sc.rand_body(rng, 20), typ=DATA), len(good), CONTROL)
    case("control_on_other", good + sc.frame(b"", typ=other), len(good), CONTROL)
    if role == "client":
        case("empty_at_client", good + sc.frame(b""), len(good), OK)
    return out


def small_cases(T, mis, role="server", nul=1, seed=2):
    rng = np.random.default_rng(seed * 1000 + T + mis)
    ctl = PING if role == "server" else PONG
    out = []
    bodies = [100, 0, 513, 1, 1024, 33]
    stream, offs = bytearray(sc.rand_body(rng, 5)), []
    for k, ln in enumerate(bodies):
        offs.append(len(stream))
        stream += sc.frame(sc.rand_body(rng, ln), version=k + 1)
    hb = len(stream)
    stream += sc.frame(b"", typ=ctl, version=9)
    ents = [(offs[0], OK), (hb, CONTROL), (FAR, BAD_CRC), (offs[2], OK), (offs[1], OK), (hb, CONTROL), (offs[4], OK),
            (offs[3], OK), (FAR, NOT_REACHED), (offs[5], OK), (len(stream), MALFORMED)]
    c = Case("capacity", bytes(stream), ents, [0, 2, 2, 7, len(ents)], role, False, nul, [None])
    e = want_of(c, None)
    # the total, one byte less, inside a body, on a NUL (the last byte of an entry), nothing
    caps = [None, e.total - 1, e.body_offsets[6] + 500, e.body_offsets[3] + 513 + nul - 1, 0]
    out.append(c._replace(out_caps=caps))
    out.append(Case("one_ok", bytes(stream), [(offs[5], OK)], [0, 1], role, False, nul, [None, 20, 0]))
    out.append(Case("one_control", bytes(stream), [(hb, CONTROL)], None, role, False, nul, [None]))
    out.append(Case("one_nothing", bytes(stream), [(FAR, RECV_ERR)], [0, 1], role, False, nul, [None]))
    big = 3 * T + 5  # LIFT_CAP: one body over several tiles at an odd stream offset, between small frames
    stream, offs = bytearray(sc.rand_body(rng, 1)), []
    for ln in (10, big, 2000, 6):
        stream += sc.rand_body(rng, (1 - len(stream)) % 2)
        offs.append(len(stream))
        stream += sc.frame(sc.rand_body(rng, ln))
    assert offs[1] % 2 == 1
    ents = [(offs[0], OK), (offs[1], OK), (FAR, SKIPPED), (offs[2], OK), (offs[3], OK)]
    out.append(Case("lifted", bytes(stream), ents, [0, 5], role, True, nul, [None, 10 + nul + big + nul - 1]))
    out.append(Case("lifted_not", bytes(stream), ents, [0, 5], role, False, nul, [None]))  # the cap in force: contradictions
    return out


def all_cases(T, mis, role="server", nul=1):
    return [table_case(T, mis, role, nul)] + small_cases(T, mis, role, nul) + lying_cases(role, nul)
