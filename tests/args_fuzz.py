"""A seeded generator of `params` spans for the frame args, and the three claims that hold a
layer's rows against the reference's own dispatcher (oracle.ref_dispatch):

    NONE     (the route defers the whole body) nothing is claimed
    OK       the reply recomputed from the decoded slots -- Python handlers, then the reply's
             plain rule (reply_cases.result_body) -- is the reference's reply, byte for byte
    INVALID  the reference's reply is the -32602 form
    DEFER    nothing is claimed

The canonical class is what the reference client's stubs print (args_cases.canonical_span); the
hostile class has shuffled, duplicated and near-miss keys, every JSON type in every slot,
numbers in every RFC form (15, 17 and 19 to 20 digits, the int32 and int64 edges), i64 strings
with blanks, signs, junk and 18 to 20 digits, strings with every escape, nested extras and 2 to 4
byte edits.  a + b stays inside int32: the reference's overflow is undefined.  The generator
writes JSON text by hand and shares no code with rpc_amd/csrc/frames_args.h."""
import functools
import random
from typing import NamedTuple

import args_cases as ac
import reply_cases as rp
import route_cases as rc
from args_cases import A, E, M, N, P, S, X

INVALID_PARAMS = -32602
EDIT_POOL = b'{}[],:"\\ \t\n\r0123456789-+.eEtfnu/abnsxok\x01\x1f\x7f\x80\xff'
ESCAPES = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t", b"\\u0041", b"\\u00e9"]
EDGES = [0, 1, -1, 7, 2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**53, 2**53 + 1, 2**63 - 1, 2**63, -2**63, -2**63 - 1, 10**18,
         10**19 - 1, 10**19]


class Row(NamedTuple):
    hostile: bool
    method: int
    span: object  # bytes, or None for a request without `params`
    rid: int


def digits(rng, n):
    return str(rng.randrange(1, 10)) + "".join(rng.choice("0123456789") for _ in range(n - 1))


def number(rng):
    """A JSON number in every RFC form."""
    r = rng.random()
    if r < 0.3:
        v = rng.choice(EDGES) if rng.random() < 0.6 else rng.randrange(-1000, 1000)
        return (rng.choice(["%d", "%d", "%d.0", "%d.5", "%de0", "%dE+1", "%d.25e-2", "%de-1"]) % v).encode()
    if r < 0.4:
        return rng.choice([b"0", b"-0", b"0.0", b"-0.0", b"1e400", b"-1e400", b"1e-400", b"4.9e-324", b"1e5", b"1E5", b"1e+5",
                           b"2.5e-3", b"0e0", b"1.7976931348623157e308", b"2.2250738585072014e-308"])
    d = digits(rng, rng.choice([15, 17, 19, 19, 20]))
    at = rng.randrange(0, len(d) + 1)
    text = d if at == len(d) else (d[:at] or "0") + "." + d[at:]
    if rng.random() < 0.5:
        text += rng.choice(["e%d", "E%d", "e%+d"]) % rng.randrange(-30, 30)
    return (rng.choice(["", "-"]) + text).encode()


def i64_string(rng):
    r = rng.random()
    if r < 0.5:
        return b'"%d"' % (rng.choice(EDGES) if rng.random() < 0.5 else rng.randrange(-2**63, 2**63))
    if r < 0.7:
        return b'"%s"' % (rng.choice(["", "-"]) + digits(rng, rng.choice([18, 19, 20]))).encode()
    return rng.choice([b'" 12"', b'"12 "', b'"+12"', b'"12a"', b'""', b'"-"', b'"0x10"', b'"1e3"', b'"1.5"', b'"007"', b'"-0"',
                       b'"\\t12"', b'"1\\/2"', b'"\xff"'])


def string(rng):
    out = bytearray(b'"')
    for _ in range(rng.randrange(0, 30)):
        r = rng.random()
        if r < 0.04:
            out += rng.choice(ESCAPES)
        elif r < 0.1:
            out += rng.choice([b"\xc3\xa9", b"\xe4\xb8\xad", b"\x80", b"\xff", b"\x7f"])
        else:
            out.append(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789 _-/{}[]:,'"))
    return bytes(out + b'"')


def any_value(rng):
    """Every JSON type."""
    return rng.choice([lambda: b"null", lambda: b"true", lambda: b"false", lambda: number(rng), lambda: string(rng),
                       lambda: i64_string(rng), lambda: b"[1,2]", lambda: b"[]", lambda: b'{"a":1}', lambda: b"{}"])()


def right_value(rng, t):
    if t == ac.BOOL:
        return rng.choice([b"true", b"false"])
    if t == ac.STR:
        return string(rng)
    if t == ac.I64:
        return i64_string(rng) if rng.random() < 0.7 else number(rng)
    if t == ac.I32 and rng.random() < 0.6:
        return b"%d" % rng.randrange(-2**30, 2**30)
    return number(rng)


def near_miss(rng, name):
    return rng.choice([name.upper(), name + b" ", b" " + name, name + name, name[:-1], name + b"\xc3\xa9", b"params"])


def hostile_span(rng, m):
    r = rng.random()
    if r < 0.04:
        return rng.choice([b"[1,2]", b"null", b'"x"', b"12", b"true", b"[]", b"-1.5e3", b'[{"a":1}]', None])
    members = []
    for name, t in ac.IDL_METHODS[m][1]:
        r = rng.random()
        if r < 0.04:
            continue  # absent
        value = any_value(rng) if r < 0.14 else right_value(rng, t)
        members.append((name, value))
        if rng.random() < 0.08:  # a duplicate, before or behind
            members.insert(rng.randrange(len(members) + 1), (name, any_value(rng) if rng.random() < 0.5 else right_value(rng, t)))
        if rng.random() < 0.08:
            members.insert(rng.randrange(len(members) + 1), (near_miss(rng, name), right_value(rng, t)))
    if rng.random() < 0.2:  # nested extras, with the parameters' own names inside
        extra = rng.choice([b'{"a":9,"q":[1,{"a":2,"s":"x"}]}', b'[{"n":1},[[]],"a"]', b'{"x":"1","b":{"b":2}}', b"[[[[1]]]]"])
        members.insert(rng.randrange(len(members) + 1), (rng.choice([b"z", b"extra", b"q"]), extra))
    if rng.random() < 0.5:
        rng.shuffle(members)
    wsp = rng.choice([0, 0, 0, 0.3])
    gap = lambda: bytes(rng.choice(b" \t\n\r") for _ in range(rng.randrange(1, 3))) if rng.random() < wsp else b""  # noqa: E731
    span = b"{" + gap() + (b"," + gap()).join(b'"' + k + b'"' + gap() + b":" + gap() + v + gap() for k, v in members) + b"}"
    if rng.random() < 0.12:  # 2 to 4 byte edits
        b = bytearray(span)
        for _ in range(rng.randrange(2, 5)):
            at = rng.randrange(len(b)) if b else 0
            how = rng.randrange(3)
            if not b or how == 0:
                b.insert(at, rng.choice(EDIT_POOL))
            elif how == 1:
                b[at] = rng.choice(EDIT_POOL)
            else:
                del b[at]
        span = bytes(b)
    return span


def overflows(row):
    """Is this an add_i32 request the rules decode and whose a + b leaves int32?"""
    if row.method != A or row.span is None:
        return False
    status, slots = ac.args_span(row.span, 0, ac.IDL_METHODS[A][1])
    return status == ac.OK and not -2**31 <= s64(slots[0]) + s64(slots[1]) < 2**31


@functools.lru_cache(maxsize=None)
def corpus(seed, count=12000):
    """`count` rows, canonical and hostile in turn.  Cached: the callers share it and leave it
    unchanged."""
    rng = random.Random(seed)
    rows = []
    while len(rows) < count:
        k = len(rows)
        m = rng.randrange(7)
        rid = rng.choice([0, 1, 4294967295]) if rng.random() < 0.05 else rng.randrange(0, 2**32)
        row = Row(True, m, hostile_span(rng, m), rid) if k % 2 else Row(False, m, ac.canonical_span(rng, m), rid)
        if not overflows(row):
            rows.append(row)
    return rows


def bodies_of(rows):
    return [ac.request(ac.IDL_METHODS[r.method][0], r.span, r.rid)[0] for r in rows]


def entries_of(rows, nul=1, pad_front=0):
    """The rows' bodies back to back and their entries (args_cases.args_entries' form) as the
    route's plain rules give them: a body whose edits broke the whole request is no CALL, and the
    args never see it."""
    buf, entries = bytearray(b"#" * pad_front), []
    for body in bodies_of(rows):
        kind, method, _, po, pl = rc.route_body(body)
        entries.append((len(buf), len(body), kind, method, po, pl))
        buf += body + b"\0" * nul
    return bytes(buf), entries


@functools.lru_cache(maxsize=None)
def ruled(seed, count=12000):
    """The plain rules' (status, reply_status, slots) of every row (cached)."""
    buf, entries = entries_of(corpus(seed, count))
    return ac.args_entries(buf, entries)


@functools.lru_cache(maxsize=None)
def answers(seed, count=12000):
    """The reference's reply to every row's body (cached)."""
    import route_fuzz as rf
    return rf.reference(bodies_of(corpus(seed, count)))


# ---- the claims -----------------------------------------------------------------------------
def s64(v):
    return v - (1 << 64) if v >> 63 else v


def f64(v):
    import struct
    return struct.unpack("<d", struct.pack("<Q", v))[0]


def handler_value(m, slots):
    """The value text the reference's handler and cJSON print for the decoded parameters
    (rpc_server_impl.c; print_number for the numbers)."""
    if m == P:
        return b'"pong"'
    if m == E:
        return b'"%d"' % s64(slots[0])
    if m == A:
        return ac.print_number(float(s64(slots[0]) + s64(slots[1])))
    if m == M:
        return ac.print_number(f64(slots[0]) * f64(slots[1]))
    if m == N:
        return b"true" if s64(slots[0]) % 2 == 0 else b"false"
    if m == S:
        return b"%d" % (slots[0] >> 32)
    text = "a=%d,b=%.2f,ok=%s" % (s64(slots[0]), f64(slots[1]), "true" if slots[2] else "false")
    return b'"' + text[:127].encode() + b'"'  # (the handler's buffer holds 128 bytes)


def hold(rows, replies, layer):
    """The three claims for one layer's (status, reply_status, slots) against the reference's
    replies.  Returns the counts per status."""
    assert len(rows) == len(replies) == len(layer)
    n = {ac.NONE: 0, ac.OK: 0, ac.INVALID: 0, ac.DEFER: 0}
    for row, reply, (status, reply_status, slots) in zip(rows, replies, layer):
        assert status in n, (row, status)
        n[status] += 1
        if status == ac.OK:
            assert reply_status == 0 and rp.result_body(row.rid, handler_value(row.method, slots)) == reply, (row, slots, reply)
        elif status == ac.INVALID:
            assert reply_status == INVALID_PARAMS
            assert rp.error_body(row.rid, INVALID_PARAMS, rp.MESSAGES[INVALID_PARAMS]) == reply, (row, reply)
    return n


def conditions(rows, rules):
    """Known before a GPU is used, on the plain rules alone: the canonical class has no DEFER and
    no INVALID; at least half of the hostile class is decided, and each status occurs often."""
    canon = [r[0] for row, r in zip(rows, rules) if not row.hostile]
    hostile = [r[0] for row, r in zip(rows, rules) if row.hostile]
    assert canon and all(s == ac.OK for s in canon), {s: canon.count(s) for s in set(canon)}
    n = {s: hostile.count(s) for s in (ac.NONE, ac.OK, ac.INVALID, ac.DEFER)}
    assert sum(n.values()) == len(hostile), n
    assert 2 * (n[ac.OK] + n[ac.INVALID]) >= len(hostile), n
    assert min(n[ac.OK], n[ac.INVALID], n[ac.DEFER]) >= len(hostile) // 20, n
    return n
