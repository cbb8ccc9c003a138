"""Where the bodies lie: placements for the staging rounds of the frame route, resolve and args
(rpc_amd/csrc/frames_stage.h), and a model of which entries each round takes.

The three kernels judge entry i by the bytes at its (offset, length), wherever those lie, but
they bring the bytes into LDS through one piece of code whose windows depend on the placement.
Every placement here keeps entry i on body i: only the place of the bytes changes, so the plain
rules give what they give for the same bodies back to back.  Bytes that belong to no body are a
cycle of '"', '}', ',' and '7': a walk that strays into them reads another answer.

rounds() restates the window rule alone.  It says nothing about the kernels; the tests use it to
assert that an input has the property it was built for."""
import functools
import os
import random
import re
from typing import Callable, NamedTuple

import args_cases as ac
import resolve_cases as rsc
import route_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_route.h")


def kernel_constant(name):
    m = re.search(r"\b%s = (\d+)u?[,;]" % name, open(ROUTE_H).read())
    assert m, f"{name} not found in {ROUTE_H}"
    return int(m.group(1))


STAGE = kernel_constant("kRouteStage")
LANES = kernel_constant("kRouteEntries")
MAX_BODY = kernel_constant("kRouteMaxBody")
SMALL = 1088  # the emulator tests' small staging size

GAP = b'"},7'


# ---- the window rule ------------------------------------------------------------------------
def rounds(spans, pending, mis, stage=STAGE, lanes=LANES):
    """Per workgroup of ``lanes`` consecutive entries, its rounds in order: (w0, the entries the
    round takes, the pending entries it leaves behind).  w0 is in aligned space: offsets from the
    buffer's address rounded down to 16 bytes, so a multiple of 16 there is a 16-byte address
    step."""
    out = []
    for g in range(0, len(spans), lanes):
        left = [i for i in range(g, min(g + lanes, len(spans))) if pending[i]]
        group = []
        while left:
            w0 = (spans[left[0]][0] + mis) & ~15  # the lowest pending lane
            took = [i for i in left if spans[i][0] + mis >= w0 and spans[i][0] + mis + spans[i][1] <= w0 + stage]
            left = [i for i in left if not (spans[i][0] + mis >= w0 and spans[i][0] + mis + spans[i][1] <= w0 + stage)]
            group.append((w0, took, left))
        out.append(group)
    return out


def trace(spans, pending, mis, nbytes, stage=STAGE):
    """What the emulators' round trace (RPC_EMU_STAGE_TRACE) must read for a buffer of ``nbytes``:
    (workgroup, w0, bodies taken, blocks read bytewise) per round.  Only a block that is not
    wholly inside the buffer is read bytewise."""
    out = []
    for wg, group in enumerate(rounds(spans, pending, mis, stage)):
        for w0, took, _ in group:
            end = max(spans[i][0] + mis + spans[i][1] for i in took)
            edge = sum(1 for x in range(w0, end, 16) if not (x >= mis and x + 16 <= nbytes + mis))
            out.append((wg, w0, len(took), edge))
    return out


def read_trace(path):
    """An emulator's trace, each workgroup's rounds in their order, the workgroups ascending."""
    return sorted((tuple(map(int, line.split())) for line in open(path)), key=lambda r: r[0])


def walked(buf, spans):
    """The route's and the resolve's entries that reach the rounds: inside the buffer, 1 to
    kRouteMaxBody bytes."""
    return [off <= len(buf) and ln <= len(buf) - off and 1 <= ln <= MAX_BODY for off, ln in spans]


def args_walked(buf, entries, schema=ac.IDL):
    """The same for args entries: a CALL of a method with parameters whose span lies inside."""
    out = []
    for boff, blen, kind, method, poff, plen in entries:
        ok = kind == rc.CALL and method < schema.nmethods and schema.first[method] < schema.first[method + 1]
        out.append(bool(ok and boff <= len(buf) and blen <= len(buf) - boff and poff <= blen and plen <= blen - poff
                        and 1 <= plen <= MAX_BODY))
    return out


# ---- placements -----------------------------------------------------------------------------
class Placed(NamedTuple):
    name: str
    buf: bytes
    spans: list      # spans[i]: (offset, length) of body i
    holds: Callable  # holds(pending, mis): asserts the property the placement was built for
    #                  (pending: which entries reach the rounds; the stage is the one it was built at)


def lay(total, placed):
    """A buffer of ``total`` gap bytes with (offset, body) pairs written over them."""
    buf = bytearray((GAP * (total // len(GAP) + 1))[:total])
    for off, body in placed:
        assert 0 <= off and off + len(body) <= total
        buf[off:off + len(body)] = body
    return bytes(buf)


def packed(bodies, memory_order):
    """Bodies back to back in memory in ``memory_order`` (a permutation of their indices)."""
    spans, at = [None] * len(bodies), 0
    for i in memory_order:
        spans[i] = (at, len(bodies[i]))
        at += len(bodies[i])
    return lay(at, [(spans[i][0], bodies[i]) for i in range(len(bodies))]), spans


def _counts(groups):
    return [len(g) for g in groups]


def back_to_back(bodies):
    buf, spans = packed(bodies, range(len(bodies)))
    return Placed("back to back", buf, spans, lambda pending, mis: None)


def reversed_(bodies):
    """Back to back in memory, the last entry first: every window is opened by the workgroup's
    highest body and holds little else."""
    buf, spans = packed(bodies, range(len(bodies) - 1, -1, -1))

    def holds(pending, mis):
        assert max(_counts(rounds(spans, pending, mis))) >= 128

    return Placed("reversed", buf, spans, holds)


def shuffled(bodies, seed=0x5EA7):
    """Back to back in memory in a seeded permutation over the whole batch."""
    order = list(range(len(bodies)))
    random.Random(seed).shuffle(order)
    buf, spans = packed(bodies, order)

    def holds(pending, mis):
        groups = rounds(spans, pending, mis)
        assert max(_counts(groups)) >= 3
        assert any(spans[i][0] + mis < w0 for g in groups for w0, _, left in g for i in left)

    return Placed("shuffled", buf, spans, holds)


def slots(bodies, stride):
    """Body i at i * stride."""
    assert stride > MAX_BODY
    spans = [(i * stride, len(b)) for i, b in enumerate(bodies)]
    buf = lay(spans[-1][0] + spans[-1][1] + 3, [(s[0], b) for s, b in zip(spans, bodies)])

    def holds(pending, mis):
        groups = rounds(spans, pending, mis)
        if stride == 4099:
            assert max(_counts(groups)) >= 30
        if stride == 1040:
            assert 31 in {len(took) for g in groups for _, took, _ in g}

    return Placed("slots of %d" % stride, buf, spans, holds)


def one_body(bodies):
    """Workgroup g's lanes all on the same span, body g's."""
    firsts, spans = packed(bodies, range(len(bodies)))
    spans = [s for s in spans for _ in range(LANES)]

    def holds(pending, mis):
        assert all(pending) and _counts(rounds(spans, pending, mis)) == [1] * len(bodies)

    return Placed("one body", firsts, spans, holds)


def two_bodies(a, b, stage=STAGE):
    """The lanes of one workgroup alternate between two spans more than a window apart."""
    far = 7 + len(a) + stage + 1
    buf = lay(far + len(b) + 2, [(7, a), (far, b)])
    spans = [(7, len(a)) if t % 2 == 0 else (far, len(b)) for t in range(LANES)]

    def holds(pending, mis):
        (group,) = rounds(spans, pending, mis, stage)
        assert all(pending) and [took for _, took, _ in group] == [list(range(0, LANES, 2)), list(range(1, LANES, 2))]

    return Placed("two bodies", buf, spans, holds)


def nested(text):
    """Every prefix and every suffix of one text: all spans share bytes with others."""
    p, n = 5, len(text)
    buf = lay(p + n + 5, [(p, text)])
    spans = [(p, k) for k in range(1, n + 1)] + [(p + k, n - k) for k in range(n)]

    def holds(pending, mis):
        assert all(pending) and all(p <= off and off + ln <= p + n for off, ln in spans)
        # any two prefixes, any two suffixes, and a prefix and a suffix that are not the two
        # halves of one cut, share a byte
        assert all(a[0] < b[0] + b[1] and b[0] < a[0] + a[1] for a in spans[:n] for b in spans[n:] if a[1] > b[0] - p)
        assert spans.count((p, n)) == 2

    return Placed("nested", buf, spans, holds)


def window_edge(make, a, over, length, mis, stage=STAGE):
    """Lane 0's body at an aligned-space offset with low bits ``a`` opens the window at w0 = 16;
    lanes 1 and 2 hold a body of ``length`` bytes (None: the shortest) that ends ``over`` bytes
    behind the window's last byte.  Built for one mis and one stage."""
    w0 = 16
    head, tail = make(0), make(1, length)
    x1 = w0 + stage + over - len(tail)
    assert x1 >= w0 + a + len(head) and x1 - mis >= 0
    spans = [(w0 + a - mis, len(head)), (x1 - mis, len(tail)), (x1 - mis, len(tail))]
    buf = lay(x1 - mis + len(tail) + 5, [(spans[0][0], head), (spans[1][0], tail)])

    def holds(pending, mis_):
        assert mis_ == mis and all(pending)
        (group,) = rounds(spans, pending, mis, stage)
        assert group[0][0] == w0 and spans[1][0] + mis + spans[1][1] == w0 + stage + over
        assert [took for _, took, _ in group] == ([[0, 1, 2]] if over == 0 else [[0], [1, 2]])

    return Placed("window edge a=%d over=%d L=%d" % (a, over, len(tail)), buf, spans, holds)


def buffer_ends(make, mis):
    """A body at offset 0 and a body that ends on the buffer's last byte; the last 16-byte block
    holds 1 to 15 bytes of the buffer, the first 16 - mis."""
    first, last = make(2), make(3)
    total = len(first) + len(last) + 16
    total += ((mis * 7) % 15 + 1 - (mis + total)) % 16
    spans = [(0, len(first)), (total - len(last), len(last))]
    buf = lay(total, list(zip([s[0] for s in spans], [first, last])))

    def holds(pending, mis_):
        assert mis_ == mis and all(pending) and spans[0][0] == 0 and spans[1][0] + spans[1][1] == len(buf)
        assert (mis + len(buf)) % 16 != 0  # the last block is partial (the first one whenever mis != 0)

    return Placed("buffer ends mis=%d" % mis, buf, spans, holds)


WHOLE_MIS = (0, 12, 15)


def whole_buffer(body, mis):
    """The body is the whole buffer, of 8 bytes: at mis 0 its only block is both the first and the
    last; at 12 and 15 it straddles a 16-byte step and both blocks are partial."""
    assert len(body) == 8

    def holds(pending, mis_):
        assert mis_ == mis and all(pending)
        assert (mis // 16 == (mis + 7) // 16) == (mis == 0) and (mis + 8) % 16 != 0

    return Placed("whole buffer mis=%d" % mis, bytes(body), [(0, 8)], holds)


def joined(parts):
    """Placements one behind the other in one buffer, each from a multiple of 16 bytes."""
    buf, spans = bytearray(), []
    for p in parts:
        buf += lay(-len(buf) % 16, [])
        spans += [(off + len(buf), ln) for off, ln in p.spans]
        buf += p.buf
    return bytes(buf), spans


# ---- bodies -----------------------------------------------------------------------------------
# Edge bodies end in a number and '}', each with its own large number: a byte short, a byte over
# or a stale byte of the round before reads another number or none.
def _padded(build, length):
    if length is None:
        return build(None)
    body = build(length - len(build(0)))
    assert len(body) == length
    return body


def request(k, length=None):
    """A canonical request of exactly ``length`` bytes (None: the shortest) with id 4000000001 + k."""
    rid = 4000000001 + k
    return _padded(lambda pad: rc.canonical("ping", None, rid) if pad is None
                   else rc.canonical("strlen_s", {"s": "x" * pad}, rid), length)


def reply(k, length=None):
    """The same for a reply as the reference's server prints it."""
    rid = 4000000001 + k
    return _padded(lambda pad: rsc.reply(rid, result=k) if pad is None else rsc.reply(rid, result="y" * pad), length)


def params(k, length=None):
    """A `params` span of is_even, n = 2000000001 + k (a member in front pads it)."""
    n = 2000000001 + k
    return _padded(lambda pad: b'{"n":%d}' % n if pad is None else b'{"pad":"%s","n":%d}' % (b"z" * pad, n), length)


def _mixed(seed, short, long_):
    out = short + long_
    random.Random(seed).shuffle(out)
    return out


@functools.lru_cache(maxsize=None)
def route_set():
    """700 request bodies over three workgroups, the last one partial: canonical requests, mutated
    ones and 60 long ones (so that a workgroup's bodies fill several windows)."""
    rng = random.Random(0x57A6E)
    long_ = [request(100 + k, rng.randrange(700, MAX_BODY + 1)) for k in range(60)]
    return _mixed(1, rc.canonical_set(0x57A6E, 400) + rc.mutation_set(0x57A6F, 240), long_)


@functools.lru_cache(maxsize=None)
def resolve_set():
    """700 reply bodies and a shuffled pending list that waits for most of their ids."""
    rng = random.Random(0x57A70)
    long_ = [reply(100 + k, rng.randrange(700, MAX_BODY + 1)) for k in range(60)]
    bodies = _mixed(2, rsc.canonical_set(0x57A70, 400) + rsc.mutation_set(0x57A71, 240), long_)
    return bodies, pending_for(bodies, 3)


def pending_for(bodies, seed):
    """A shuffled pending list: three of every four ids the bodies decode to, and strangers."""
    ids = sorted({row[1] for row in map(rsc.decode_body, bodies) if row[0] == rsc.UNKNOWN})
    ids = [i for k, i in enumerate(ids) if k % 4] + [777777, 888888]
    random.Random(seed).shuffle(ids)
    return ids


@functools.lru_cache(maxsize=None)
def args_set():
    """700 (method, `params` span) pairs, 60 of them long."""
    rng = random.Random(0x57A72)
    long_ = [(ac.N, params(100 + k, rng.randrange(700, MAX_BODY + 1))) for k in range(60)]
    return _mixed(3, ac.canonical_set(0x57A72, 400) + ac.mutation_set(0x57A73, 240), long_)


#: lanes that carry an entry of another kind with garbage offsets (two of them lane 0 of a workgroup)
STRANGERS = (0, 77, LANES, 2 * LANES + 100)


def args_entries(spans, methods, lead=False, strangers=()):
    """args entries for placed spans.  Without ``lead`` the body is the span itself (params_off
    0); with it the body starts up to 40 bytes earlier.  The lanes in ``strangers`` get an entry
    that is no CALL, with offsets that lie nowhere."""
    rng = random.Random(0x1EAD)
    entries = []
    for (off, ln), m in zip(spans, methods):
        back = min(off, rng.randrange(41)) if lead else 0
        entries.append((off - back, ln + back, rc.CALL, m, back, ln))
    for k, t in enumerate(strangers):
        if t < len(entries):
            kind = (rc.NONE, rc.NOT_FOUND, rc.INVALID, rc.DEFER)[k % 4]
            entries[t] = ((1 << 62) + k, 5, kind, 0xFFFF, 1 << 31, 1 << 31)
    return entries


#: a schema whose one method takes the `id` of {"id":7}, the whole buffer of 8 bytes
ID_SCHEMA = ac.schema_of([(b"take_id", [(b"id", ac.I32)])])
WHOLE = b'{"id":7}'


# ---- the placements a test runs ---------------------------------------------------------------
BATCH = ["reversed", "shuffled", "slots of 1040", "slots of 4099", "one body", "two bodies", "nested"]


def batch(name, bodies, make):
    """The batch placement ``name`` of ``bodies`` (``make``: the kernel's edge bodies)."""
    if name == "back to back":
        return back_to_back(bodies)
    if name == "reversed":
        return reversed_(bodies)
    if name == "shuffled":
        return shuffled(bodies)
    if name.startswith("slots of "):
        return slots(bodies, int(name[9:]))
    if name == "one body":
        return one_body([make(10), make(11, MAX_BODY), make(12, 333)])
    if name == "two bodies":
        return two_bodies(make(20), make(21, MAX_BODY))
    assert name == "nested"
    return nested(make(30, 90))


def edge_lengths(stage):
    """The lengths of the window-edge bodies: two bodies of kRouteMaxBody do not fit the small stage."""
    return (None, MAX_BODY) if stage >= 2 * MAX_BODY + 64 else (None,)


def window_edges(make, mis, stage=STAGE):
    return [window_edge(make, a, over, length, mis, stage)
            for a in (0, 1, 15) for over in (0, 1) for length in edge_lengths(stage)]


def mixture(bodies, make, mis):
    """Every placement in one buffer: a workgroup of one round per lane, one of a single round,
    then the rest; at least 3 * kRouteEntries + 1 entries.  Returns (buffer, spans, bodies)."""
    parts = [(reversed_(bodies[:LANES]), bodies[:LANES])]
    p = one_body([make(10)])
    parts.append((p, [make(10)] * LANES))
    parts.append((two_bodies(make(20), make(21, MAX_BODY)), [make(20), make(21, MAX_BODY)] * (LANES // 2)))
    rest = bodies[LANES:LANES + 120]
    parts.append((shuffled(rest), rest))
    parts.append((slots(rest[:40], 4099), rest[:40]))
    parts.append((slots(rest[40:90], 1040), rest[40:90]))
    text = make(30, 90)
    p = nested(text)
    parts.append((p, [text[off - 5:off - 5 + ln] for off, ln in p.spans]))
    for a, over in ((1, 0), (15, 1)):
        p = window_edge(make, a, over, None, mis)
        parts.append((p, [make(0), make(1), make(1)]))
    parts.append((buffer_ends(make, 0), [make(2), make(3)]))
    buf, spans = joined([p for p, _ in parts])
    placed_bodies = [b for _, bs in parts for b in bs]
    assert len(spans) == len(placed_bodies) >= 3 * LANES + 1
    assert all(buf[off:off + ln] == b for (off, ln), b in zip(spans, placed_bodies))
    return buf, spans, placed_bodies


def args_batch(name):
    """The batch placement ``name`` of the args' spans and the method of each entry."""
    pairs = args_set()
    p = batch(name, [span for _, span in pairs], params)
    from_set = name == "back to back" or name in BATCH[:4]
    return p, [m for m, _ in pairs] if from_set else [ac.N] * len(p.spans)


def args_mixture(mis):
    """mixture() of the args' spans: (buffer, spans, methods)."""
    pairs = args_set()
    method_of = {span: m for m, span in reversed(pairs)}
    buf, spans, placed = mixture([span for _, span in pairs], params, mis)
    return buf, spans, [method_of.get(b, ac.N) for b in placed]
