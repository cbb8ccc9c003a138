"""Shared by test_pack_emu.py and test_frames_pack.py: the rules of
rpc_frames_pack_device restated in plain Python (the reference for both), built on
scan_cases.frame and zlib.crc32, and the case table both layers run.

For entry i = (type, version, off, len), in this order (include/rpccrc.h, frame pack):

    1. type == NONE:           0 bytes, SKIPPED
    2. type is PING or PONG:   12 bytes (body_len 0, crc32 0), CONTROL
    3. body not inside [0, bodies_bytes):   0 bytes, MALFORMED
    4. len > 1024 and not lift_cap:         0 bytes, TOO_LARGE
    5. otherwise               12 + len bytes, OK

    offset[i] = sum of the sizes before i; total = sum of all sizes
    an entry of non-zero size with offset + size > out_cap: not written, MALFORMED
"""
import zlib
from typing import NamedTuple

import numpy as np

import scan_cases as sc

HDR = 12
MAX_BODY = 1024
DATA, PING, PONG, NONE = 0, 1, 2, 0xFFFF
BAD_CRC, OK, CONTROL, TOO_LARGE, MALFORMED, RECV_ERR, NOT_REACHED, SKIPPED = range(8)
FILL = 0xA5


class Expected(NamedTuple):
    offsets: list      # [n]
    verdict: list      # [n], with the capacity downgrade
    crc: list          # [n]
    total: int
    conn_bytes_first: list  # [nconn + 1], or [] without a CSR
    out: bytes         # out_cap bytes, FILL where nothing is written
    frames: list       # [n] the wire bytes of each entry (b"" for size 0), whatever out_cap is


def expected(bodies, entries, conn_first=None, lift_cap=False, out_cap=None):
    """The rules above over entries [(type, version, off, len)]; out_cap None: the total."""
    nb = len(bodies)
    frames, verdict, crc = [], [], []
    for typ, ver, off, ln in entries:
        if typ == NONE:
            f, v, c = b"", SKIPPED, 0
        elif typ in (PING, PONG):
            f, v, c = sc.frame(b"", typ=typ, crc=0, version=ver), CONTROL, 0
        elif not (off <= nb and ln <= nb - off):
            f, v, c = b"", MALFORMED, 0
        elif ln > MAX_BODY and not lift_cap:
            f, v, c = b"", TOO_LARGE, 0
        else:
            body = bytes(bodies[off:off + ln])
            f, v, c = sc.frame(body, typ=typ, version=ver), OK, zlib.crc32(body)
        frames.append(f)
        verdict.append(v)
        crc.append(c)
    offsets = [0]
    for f in frames:
        offsets.append(offsets[-1] + len(f))
    total = offsets.pop()
    cap = total if out_cap is None else out_cap
    out = bytearray([FILL]) * cap
    for i, f in enumerate(frames):
        if not f:
            continue
        if offsets[i] + len(f) > cap:
            verdict[i] = MALFORMED
        else:
            out[offsets[i]:offsets[i] + len(f)] = f
    cbf = [] if conn_first is None else [(offsets + [total])[min(k, len(entries))] for k in conn_first]
    return Expected(offsets, verdict, crc, total, cbf, bytes(out), frames)


class Case(NamedTuple):
    name: str
    bodies: bytes
    entries: list      # [(type, version, off, len)]
    conn_first: object  # list, or None
    lift_cap: bool
    out_caps: list     # None: exactly the total


class _Builder:
    """Lays entries out so that chosen frames start at chosen output offsets."""

    def __init__(self, rng, src_bytes=6000):
        self.rng = rng
        self.src = bytearray(sc.rand_body(rng, src_bytes))
        self.entries = []
        self.cur = 0

    def data(self, off, ln, typ=DATA, ver=1):
        self.entries.append((typ, ver, off, ln))
        self.cur += HDR + ln

    def filler(self, nbytes):
        """Data frames of nbytes in all (0, or >= 12), bodies from anywhere in the source."""
        assert nbytes == 0 or nbytes >= HDR, nbytes
        left = nbytes
        while left:
            if left > 2 * (HDR + MAX_BODY):
                size = HDR + int(self.rng.integers(0, MAX_BODY + 1))
            elif left > HDR + MAX_BODY:
                size = int(self.rng.integers(max(HDR, left - HDR - MAX_BODY), min(HDR + MAX_BODY, left - HDR) + 1))
            else:
                size = left
            ln = size - HDR
            self.data(int(self.rng.integers(0, len(self.src) - ln + 1)), ln, typ=int(self.rng.choice([0, 0, 7])))
            left -= size

    def goto(self, target):
        """Filler so that the next frame starts at output offset target (moved on by 16-byte
        steps while the gap is too small for a frame)."""
        while target - self.cur != 0 and target - self.cur < HDR:
            target += 16
        self.filler(target - self.cur)
        assert self.cur == target

    def heartbeat(self, typ=PING, ver=1):
        self.entries.append((typ, ver, int(self.rng.integers(0, 2**40)), int(self.rng.integers(0, 2**32))))
        self.cur += HDR

    def nothing(self, kind):
        if kind == "none":  # (offset and length are not looked at)
            self.entries.append((NONE, 1, int(self.rng.integers(0, 2**40)), int(self.rng.integers(0, 2**32))))
        elif kind == "too_large":
            self.entries.append((DATA, 1, 0, MAX_BODY + 1 + int(self.rng.integers(0, 2000))))
        else:  # out of range by one byte
            self.entries.append((DATA, 1, len(self.src) - 9, 10))


def table_case(T, mis, seed=1):
    """One batch that meets every layout case at tile size T with the output's address
    mis bytes past a 16-byte boundary (tile edges lie at output offsets m * T - mis)."""
    rng = np.random.default_rng(seed * 1000 + T + mis)
    b = _Builder(rng, 16 * 1100 + 6000)
    conn = [0, 0]  # an empty connection at the start
    for kind in ("none", "too_large", "none"):  # a run of nothing at the very start
        b.nothing(kind)
    b.data(0, 37)  # a body at byte 0 of the source
    b.data(len(b.src) - 21, 21)  # and one ending at its last byte
    b.nothing("range")
    conn.append(len(b.entries))
    # every (source offset mod 16) x (body start in the output mod 16), six lengths
    for ln in (0, 1, 15, 16, 17, 1024):
        for sa in range(16):
            soff = 6000 + sa * 1100 + ((sa - (6000 + sa * 1100)) % 16)  # = sa mod 16
            assert soff % 16 == sa
            for da in range(16):
                pad = (da - mis - (b.cur + HDR + HDR)) % 16  # a filler frame that turns the alignment
                b.data(int(rng.integers(0, 3000)), pad)
                assert (b.cur + HDR + mis) % 16 == da
                b.data(soff, ln)
        conn.append(len(b.entries))

    def edge(back):
        """The first tile edge (output offset m * T - mis) that a frame starting `back`
        bytes before it can still be placed in front of."""
        m = -(-(b.cur + HDR + back + mis) // T)
        return m * T - mis - back

    for k in range(1, HDR):  # a header split across a tile edge at each inner position
        b.goto(edge(k))
        assert (b.cur + mis) % T == T - k
        b.data(int(rng.integers(0, 5000)), int(rng.integers(1, 600)), ver=k)
    conn.append(len(b.entries))
    ln = 300  # a body ending exactly on a tile edge
    b.goto(edge(HDR + ln))
    b.data(77, ln)
    assert (b.cur + mis) % T == 0
    # a piece covering three frames: a 1-byte body tail, a heartbeat, the next header
    start = b.cur + HDR
    b.goto(start + (1 - mis - (HDR + 40) - start) % 16)
    b.data(5, 40)
    assert (b.cur + mis) % 16 == 1
    b.heartbeat(PONG, ver=3)
    b.data(9, 100)
    conn.append(len(b.entries))
    for kind in ("none", "too_large", "none", "none", "range", "too_large"):  # nothing, in the middle
        b.nothing(kind)
    for i in range(40):  # a run of heartbeats
        b.heartbeat(PING if i % 3 else PONG, ver=1 + i % 2)
    conn.append(len(b.entries))
    b.data(123, 1)
    for kind in ("too_large", "none", "none"):  # and at the very end
        b.nothing(kind)
    conn += [len(b.entries)] * 2  # an empty connection at the end
    return Case("table", bytes(b.src), b.entries, conn, False, [None])


def small_cases(T, mis, seed=2):
    rng = np.random.default_rng(seed * 1000 + T + mis)
    src = sc.rand_body(rng, 4 * T + 4000)
    out = []
    # capacity: the total, one byte less, the middle of a header, the middle of a body, nothing
    ents = [(DATA, 1, 3, 100), (PING, 1, 0, 0), (NONE, 1, 0, 0), (DATA, 2, 1001, 513), (DATA, 1, 40, 0), (PONG, 1, 0, 0),
            (DATA, 1, 7, 1024), (DATA, 1, 0, 2000), (DATA, 9, 2, 33), (NONE, 1, 0, 0)]
    e = expected(src, ents)
    caps = [None, e.total - 1, e.offsets[3] + 5, e.offsets[6] + HDR + 500, e.offsets[8] + HDR, 0]
    out.append(Case("capacity", src, ents, [0, 2, 2, 7, len(ents)], False, caps))
    out.append(Case("one_data", src, [(DATA, 1, 11, 29)], [0, 1], False, [None, 40, 0]))
    out.append(Case("one_heartbeat", src, [(PONG, 5, 0, 0)], None, False, [None, 11]))
    out.append(Case("one_none", src, [(NONE, 1, 0, 0)], [0, 1], False, [None]))
    big = 3 * T + 5  # LIFT_CAP: one body over several tiles, between small frames
    ents = [(DATA, 1, 1, 10), (DATA, 1, 13, big), (PING, 1, 0, 0), (DATA, 1, 2, 2000), (DATA, 1, len(src) - 5, 6)]
    out.append(Case("lifted", src, ents, [0, 5], True, [None, HDR + 10 + HDR + big - 1]))
    return out


def all_cases(T, mis):
    return [table_case(T, mis)] + small_cases(T, mis)
