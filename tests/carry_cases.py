"""Shared by test_carry_emu.py and test_frames_carry.py: the rules of
rpc_frames_carry_device restated in plain Python (the reference for both), and builders
for the cases.

The rules (include/rpccrc.h, frame carry), for connection c, in this order:

    1. state is given and state[c] != OPEN:            CLOSED,   0 / 0
    2. off > stream_bytes, len > stream_bytes - off
       or consumed > len:                              INVALID,  0 / 0
    3. tail = len - consumed; tail > room, tail > at,
       at > next_bytes or new_len > next_bytes - at:   NO_ROOM,  0 / 0
    4. next[at - tail : at] = stream[off + consumed : off + len]
       next_off = at - tail, next_len = tail + new_len OK
"""
from typing import NamedTuple, Optional

import numpy as np

import scan_cases as sc

OK, CLOSED, INVALID, NO_ROOM = 0, 1, 2, 3
ROOM = 1040
FILL = 0xA5  # what the next buffer holds where nothing is written
U64 = (1 << 64) - 1
TABLE_TAILS = (0, 1, 2, 11, 12, 15, 16, 17, 31, 32, 33, 1023, 1024, 1035)


class Case(NamedTuple):
    name: str
    stream: bytes
    conns: list            # (off, len, consumed, state) per connection
    next_bytes: int
    next_at: list
    new_len: Optional[list]  # or None: 0 everywhere
    room: int
    use_state: bool = True


class Want(NamedTuple):
    next_off: list
    next_len: list
    status: list
    carried: int
    next: bytes  # the next buffer, FILL where nothing is written


def carry_one(stream_bytes, off, ln, consumed, closed, at, nl, next_bytes, room):
    """(status, next_off, next_len, source offset, tail)."""
    if closed:
        return CLOSED, 0, 0, 0, 0
    if off > stream_bytes or ln > stream_bytes - off or consumed > ln:
        return INVALID, 0, 0, 0, 0
    tail = ln - consumed
    if tail > room or tail > at or at > next_bytes or nl > next_bytes - at:
        return NO_ROOM, 0, 0, 0, 0
    return OK, at - tail, tail + nl, off + consumed, tail


def want_of(case: Case) -> Want:
    nxt = bytearray([FILL]) * case.next_bytes
    offs, lens, status, carried = [], [], [], 0
    for c, (off, ln, consumed, state) in enumerate(case.conns):
        nl = case.new_len[c] if case.new_len is not None else 0
        st, no, nn, src, tail = carry_one(len(case.stream), off, ln, consumed, case.use_state and state != sc.OPEN,
                                          case.next_at[c], nl, case.next_bytes, case.room)
        if tail:
            assert all(b == FILL for b in nxt[no:no + tail]), "the case's tails overlap"
            nxt[no:no + tail] = case.stream[src:src + tail]
        offs.append(no)
        lens.append(nn)
        status.append(st)
        carried += tail
    return Want(offs, lens, status, carried, bytes(nxt))


def _round_up(x, a):
    return -(-x // a) * a


def table_case(room=ROOM, tails=TABLE_TAILS, seed=0xCA22):
    """Every (source mod 16, destination mod 16) pair at every tail length: the tail of
    connection (s, d, t) starts at a stream offset that is s mod 16 and goes to an offset of the
    next buffer that is d mod 16.  Consumed prefixes, gaps and new lengths vary; the regions
    [at - room, at) are disjoint."""
    rng = np.random.default_rng(seed)
    stream, conns, next_at, new_len = bytearray(), [], [], []
    cur = 0
    for t in tails:
        for s in range(16):
            for d in range(16):
                consumed = int(rng.integers(0, 40))
                start = _round_up(len(stream) + consumed + 1, 16) + s  # where the tail starts in the stream
                off = start - consumed
                stream += sc.rand_body(rng, off - len(stream))  # junk between the connections
                stream += sc.rand_body(rng, consumed + t)
                conns.append((off, consumed + t, consumed, sc.OPEN))
                at = _round_up(cur + room, 16) + 16 + (d + t) % 16  # so that at - t is d mod 16
                next_at.append(at)
                nl = int(rng.integers(0, 70))
                new_len.append(nl)
                cur = at + nl
    stream += sc.rand_body(rng, 7)
    return Case("table", bytes(stream), conns, cur + 3, next_at, new_len, room)


def corner_case(room=ROOM, seed=0xC02E):
    """The contract's corners in one call; `names` says which connection is which."""
    rng = np.random.default_rng(seed)
    big = min(room, 200)
    names, conns, next_at, new_len = [], [], [], []
    stream = bytearray(sc.rand_body(rng, 4096 + room))
    n = len(stream)
    cur = 0

    def slot(nl):
        nonlocal cur
        at = _round_up(cur + room, 16) + 16
        cur = at + nl
        return at

    def add(name, off, ln, consumed, state, at, nl):
        names.append(name)
        conns.append((off, ln, consumed, state))
        next_at.append(at)
        new_len.append(nl)

    add("dst_starts_at_0", 100, 60, 23, sc.OPEN, 37, 5)           # at - tail == 0
    cur = 37 + 5
    add("tail_gt_at", 300, 50, 10, sc.OPEN, 39, 0)                # tail 40 > at 39: nothing written
    add("src_starts_at_0", 0, big, 0, sc.OPEN, slot(9), 9)        # the tail starts at stream byte 0
    add("src_ends_at_end", n - 70, 70, 3, sc.OPEN, slot(0), 0)    # ... ends on the stream's last byte
    add("whole_stream_end_1", n - 1, 1, 0, sc.OPEN, slot(1), 1)
    add("tail_eq_room", 1000, room + 5, 5, sc.OPEN, slot(2), 2)
    add("tail_eq_room_plus_1", 1000, room + 6, 5, sc.OPEN, slot(2), 2)
    add("empty_at_stream_end", n, 0, 0, sc.OPEN, slot(4), 4)      # off == stream_bytes, nothing in it: valid
    add("off_past_end", n + 1, 0, 0, sc.OPEN, slot(0), 0)
    add("len_past_end", n - 5, 6, 0, sc.OPEN, slot(0), 0)
    add("off_len_wrap", U64 - 7, 16, 0, sc.OPEN, slot(0), 0)      # off + len wraps 2^64
    add("len_wrap", 8, U64, 0, sc.OPEN, slot(0), 0)
    add("consumed_gt_len", 500, 40, 41, sc.OPEN, slot(3), 3)
    add("consumed_eq_len", 500, 40, 40, sc.OPEN, slot(3), 3)      # an empty tail: OK, new bytes attached
    add("closed_garbage", 1 << 63, 1 << 62, U64, sc.CLOSED, U64 - 3, U64)
    add("closed_plain", 600, 50, 20, sc.CLOSED, slot(6), 6)
    add("state_other", 600, 50, 20, 7, slot(6), 6)                # anything but OPEN is closed
    add("at_past_next", 700, 20, 10, sc.OPEN, 1 << 40, 0)
    add("new_len_wrap", 700, 20, 10, sc.OPEN, slot(0), U64)
    last = slot(11)
    add("ends_at_next_end", 800, 30, 13, sc.OPEN, last, 11)       # at + new_len == next_bytes
    add("ends_past_next_end", 900, 30, 13, sc.OPEN, last, 12)     # ... and one more (nothing written: same slot)
    return Case("corners", bytes(stream), conns, last + 11, next_at, new_len, room), names


def long_case(chunk, tails, room, seed=0x10A6):
    """Long tails at odd source and destination offsets: each tail is dealt out in chunks
    aligned to the destination address."""
    rng = np.random.default_rng(seed)
    stream, conns, next_at, new_len = bytearray(sc.rand_body(rng, 3)), [], [], []
    cur = 0
    for i, t in enumerate(tails):
        consumed = 5 + i
        off = len(stream)
        stream += sc.rand_body(rng, consumed + t)
        stream += sc.rand_body(rng, 1 + i % 3)
        conns.append((off, consumed + t, consumed, sc.OPEN))
        at = _round_up(cur + room, chunk) + chunk + (7 * i + 3) % chunk  # a tail's end anywhere in a chunk
        next_at.append(at)
        new_len.append(i)
        cur = at + i
    return Case("long", bytes(stream), conns, cur + 1, next_at, new_len, room)


def long_tails(chunk):
    return [chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 0, 1, 17]
