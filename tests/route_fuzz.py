"""A seeded generator of request bodies for the frame route and the frame reply, and the
properties that hold both against the reference's own dispatcher (oracle.ref_dispatch).

The generator writes JSON text by hand -- it has a serialiser of its own, so that whitespace
can go into every slot, keys can repeat, numbers can take the forms cJSON reads leniently and
strings can hold every escape -- and shares no code with rpc_amd/csrc/frames_route.h.  About
half of a corpus stays close to a valid request (a known method, a digits-only id, `params`
from route_cases.canonical_params re-serialised with random whitespace and key order), so that
the routed side of the comparison is not empty; the rest is random JSON, bodies at the limits
(nesting, tokens, length; each with its neighbour one past the limit), bodies with 2 to 4
random edits, splices of two requests, bodies with a 0 byte inside, tiny bodies and
route_cases.mutation_set.

The properties (hold_route, hold_replies) are stated once; each layer -- the plain rules, the
CPU emulators, the GPU -- supplies its own rows.  conditions() keeps the comparison from being
empty; it is decided by the plain rules and the reference alone."""
import functools
import random
from typing import NamedTuple

import reply_cases as rp
import route_cases as rc

PARSE_ERROR = rp.error_body(0, -32700, rp.MESSAGES[-32700])
WS = b" \t\n\r"
ENVELOPE = [b"jsonrpc", b"method", b"params", b"id"]
NEAR_KEYS = [b"Method", b"METHOD", b"ID", b"Id", b"method ", b" method", b"Params", b"params ", b" id", b"metho",
             b"methodd", b"i", b"idd", b"param", b"paramss", b"jsonrpc ", b"\xc3\xa9"]
NEAR_NAMES = [b"nope", b"", b"pin", b"pingg", b"PING", b"Ping", b"add_i64", b"ping ", b" ping", b"mix", b"mix33",
              b"echo", b"strlen", b"is_even\xc3\xa9", b"\xff", b"rpc.discover"]
EDGE_IDS = [0, 1, 9, 10, 4294967294, 4294967295, 4294967296, 4294967297, 42949672950, 9007199254740993,
            18446744073709551616, 99999999999999999999999999]
STRICT_NUMBERS = [b"0", b"-0", b"7", b"-12", b"1.5", b"0.0", b"2e3", b"1E+2", b"-1.25e-7", b"10", b"2147483648",
                  b"-2147483649", b"9007199254740993", b"1e20", b"123456.789"]
LENIENT_NUMBERS = [b"1.", b"+1", b"01", b"1e", b"1e999", b"-1e999", b"-", b".5", b"1e+", b"0x10", b"NaN", b"Infinity",
                   b"-Infinity", b"00", b"1.e2", b"--1", b"1.5.5", b"1e5e5", b"-01"]
LENIENT_LITERALS = [b"True", b"nul", b"truefalse", b"NULL", b"tru", b"falsey", b"undefined"]
ESCAPES = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]
U_ESCAPES = [b"\\u0041", b"\\u00e9", b"\\u4e2d", b"\\ud83d\\ude00", b"\\u0000", b"\\ud800", b"\\u00zz", b"\\u12", b"\\U0041"]
HIGH = [b"\xc3\xa9", b"\xe4\xb8\xad", b"\xf0\x9f\x98\x80", b"\x80", b"\xff", b"\xfe\xff", b"\xc0\xaf", b"\xed\xa0\x80"]
PLAIN = b"abcdefghijklmnopqrstuvwxyz0123456789 _-/{}[]:,'"
EDIT_POOL = b'{}[],:"\\ \t\n\r0123456789-+.eEtfnu/abx\x01\x1f\x7f\x80\xff'


# ---- the serialiser ---------------------------------------------------------------------------
def gap(rng, wsp):
    """What goes into one slot between two tokens."""
    if wsp == 0 or rng.random() >= wsp:
        return b""
    return bytes(rng.choice(WS) for _ in range(rng.choice((1, 1, 1, 2, 3))))


def quoted(rng, text, lp=0.0):
    """`text` (bytes) as a JSON string: `"` and `\\` escaped, a control byte as its escape, `/`
    sometimes as `\\/`; with probability lp a byte as a \\u escape (the rules defer those)."""
    out = bytearray(b'"')
    for c in text:
        if lp and c < 0x80 and rng.random() < lp:
            out += b"\\u%04x" % c
        elif c == 0x22:
            out += b'\\"'
        elif c == 0x5C:
            out += b"\\\\"
        elif c == 0x2F and rng.random() < 0.3:
            out += b"\\/"
        elif c < 0x20:
            out += {8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t"}.get(c, b"\\u%04x" % c)
        else:
            out.append(c)
    return bytes(out + b'"')


def rand_string(rng, lp, most=24):
    """A string token written piece by piece: plain bytes, every two-byte escape, bytes >= 0x80
    (well-formed UTF-8 and not); with probability lp a \\u escape, a raw control byte or a bad
    escape."""
    out = bytearray(b'"')
    for _ in range(rng.randrange(0, most)):
        r = rng.random()
        if r < lp:
            out += rng.choice(U_ESCAPES + [b"\x01", b"\x1f", b"\t", b"\\q", b"\\x41", b"\\ "])
        elif r < 0.12 + lp:
            out += rng.choice(ESCAPES)
        elif r < 0.2 + lp:
            out += rng.choice(HIGH + [b"\x7f"])
        else:
            out.append(rng.choice(PLAIN))
    return bytes(out + b'"')


def scalar(rng, lp):
    r = rng.random()
    if r < lp:
        return rng.choice(LENIENT_NUMBERS + LENIENT_LITERALS)
    if r < 0.4:
        return rng.choice(STRICT_NUMBERS) if rng.random() < 0.5 else b"%d" % rng.randrange(-2**33, 2**33)
    if r < 0.6:
        return rng.choice((b"true", b"false", b"null"))
    return rand_string(rng, lp)


def rand_key(rng, lp):
    r = rng.random()
    if r < 0.25:
        return quoted(rng, rng.choice(ENVELOPE + NEAR_KEYS))
    if r < 0.3:
        return quoted(rng, rng.choice(ENVELOPE), lp=0.3)  # an escaped key
    if r < 0.3 + lp:
        return rng.choice((b"key", b"'k'", b"1", b"", b"null"))  # not a string
    return rand_string(rng, lp, most=8)


def rand_value(rng, lp, wsp, depth=0):
    """Random JSON text of any type, nested at most four deep."""
    r = rng.random()
    if depth >= 4 or r < 0.5:
        return scalar(rng, lp)
    n = rng.choice((0, 1, 1, 2, 3, 5))
    if r < 0.75:
        items = [rand_value(rng, lp, wsp, depth + 1) for _ in range(n)]
        return array(rng, items, wsp, lp)
    return obj(rng, [(rand_key(rng, lp), rand_value(rng, lp, wsp, depth + 1)) for _ in range(n)], wsp, lp)


def array(rng, items, wsp, lp=0.0):
    out = bytearray(b"[" + gap(rng, wsp))
    for k, v in enumerate(items):
        out += (b"," + gap(rng, wsp) if k else b"") + v + gap(rng, wsp)
    if items and lp and rng.random() < lp:
        out += b","  # a trailing comma
    return bytes(out + b"]")


def obj(rng, members, wsp, lp=0.0):
    """An object from (key text, value text) pairs, whitespace in every slot."""
    out = bytearray(b"{" + gap(rng, wsp))
    for k, (key, v) in enumerate(members):
        out += (b"," + gap(rng, wsp) if k else b"") + key + gap(rng, wsp)
        colon = b":" if not lp or rng.random() >= lp / 4 else rng.choice((b"", b"=", b"::"))
        out += colon + gap(rng, wsp) + v + gap(rng, wsp)
    if members and lp and rng.random() < lp:
        out += b","
    return bytes(out + b"}")


def dump(rng, v, wsp, lp=0.0):
    """A Python value (what route_cases.canonical_params builds) as JSON text: random key order
    and whitespace; a whole double prints as an integer, as the reference's client prints it."""
    if isinstance(v, dict):
        keys = list(v)
        rng.shuffle(keys)
        return obj(rng, [(quoted(rng, k.encode()), dump(rng, v[k], wsp, lp)) for k in keys], wsp)
    if isinstance(v, list):
        return array(rng, [dump(rng, x, wsp, lp) for x in v], wsp)
    if isinstance(v, bool):
        return b"true" if v else b"false"
    if v is None:
        return b"null"
    if isinstance(v, str):
        return quoted(rng, v.encode(), lp)
    if isinstance(v, float) and v == int(v) and abs(v) < 1e15:
        return b"%d" % int(v)
    return repr(v).encode()


# ---- requests close to valid ----------------------------------------------------------------
def method_value(rng, m, lp):
    r = rng.random()
    if r < 0.74:
        return quoted(rng, rc.METHODS[m], lp / 4)
    if r < 0.9:
        return quoted(rng, rng.choice(NEAR_NAMES))
    if r < 0.97:
        return rng.choice((b"5", b"null", b"true", b"{}", b'["ping"]', b'{"method":"ping"}', b"0"))
    return None  # absent


def id_value(rng, lp):
    r = rng.random()
    if r < 0.55:
        return b"%d" % rng.randrange(0, 2**32)
    if r < 0.72:
        return b"%d" % rng.choice(EDGE_IDS)
    if r < 0.82:
        return None
    if r < 0.94:
        return rng.choice((b'"12"', b'""', b"null", b"true", b"false", b'{"id":4}', b"[7]", b"[]", b'"a\\"b"'))
    return rng.choice((b"-1", b"1.5", b"1e3", b"-0", b"1.0", b"007", b"1.", b"4294967295.5", b"1e999", b"0.0",
                       b"4294967295.0", b"12e0", b"-1e-400"))


def params_value(rng, m, wsp, lp):
    """The text of a `params` value, or None for a request without one."""
    r = rng.random()
    if r < 0.46:
        return dump(rng, rc.canonical_params(rng, m), wsp, lp / 4)
    if r < 0.58:
        return None
    if r < 0.68:  # another method's
        return dump(rng, rc.canonical_params(rng, rng.randrange(7)), wsp)
    if r < 0.76:  # one field replaced or dropped
        p = rc.canonical_params(rng, m)
        if p:
            k = rng.choice(list(p))
            if rng.random() < 0.4:
                del p[k]
            else:
                p[k] = rng.choice([None, True, "7", 7, 2.5, [1], {"a": 1}, -2**31, 2**31, 1e300, "x" * 40, "", "12a"])
        return dump(rng, p, wsp)
    r = rng.random()
    if r < 0.25:
        return array(rng, [rand_value(rng, lp, wsp, 2) for _ in range(rng.randrange(0, 5))], wsp)
    if r < 0.5:
        return rand_string(rng, lp)
    if r < 0.7:
        return rng.choice(STRICT_NUMBERS) if rng.random() > lp else rng.choice(LENIENT_NUMBERS)
    if r < 0.85:
        return rng.choice((b"true", b"false", b"null"))
    return rand_value(rng, lp, wsp, 1)


def request_members(rng, wsp, lp, params=True):
    """The (key text, value text) pairs of a request close to valid: the envelope, then
    duplicated keys, near-miss keys and other members, then perhaps another order."""
    m = rng.randrange(7)
    makers = {b"jsonrpc": lambda: rng.choice((b'"2.0"', b'"2.0"', b'"2.0"', b'"1.0"', b"2", b"null"))
              if rng.random() < 0.85 else None,
              b"method": lambda: method_value(rng, m, lp),
              b"params": lambda: params_value(rng, m, wsp, lp) if params else None,
              b"id": lambda: id_value(rng, lp)}
    members = []
    for key in ENVELOPE:
        v = makers[key]()
        if v is not None:
            members.append((quoted(rng, key), v))
    if rng.random() < 0.16:  # a duplicated key: a second value, made afresh, before or behind the first
        for _ in range(rng.choice((1, 1, 2))):
            key = rng.choice(ENVELOPE[1:])
            v = makers[key]()
            if v is not None:
                members.insert(rng.randrange(len(members) + 1), (quoted(rng, key), v))
    if rng.random() < 0.14:  # a key that is nearly one of the envelope's, with a value that would count
        key = rng.choice(NEAR_KEYS)
        v = rng.choice((quoted(rng, rng.choice(rc.METHODS)), b"%d" % rng.randrange(1, 1000), b'{"n":2}', b"[1,2]"))
        members.insert(rng.randrange(len(members) + 1), (quoted(rng, key), v))
    if lp and rng.random() < lp / 2:  # an escaped key: cJSON reads it as the key it spells
        members.insert(rng.randrange(len(members) + 1), (quoted(rng, rng.choice(ENVELOPE), lp=0.3), scalar(rng, 0)))
    if rng.random() < 0.2:
        for _ in range(rng.choice((1, 1, 2, 3))):
            at = rng.randrange(len(members) + 1)
            members.insert(at, (rand_string(rng, lp / 2, most=8), rand_value(rng, lp / 2, wsp, 2)))
    if rng.random() < 0.5:
        rng.shuffle(members)
    return members


def assemble(rng, members, wsp, lp=0.0):
    """The members as a root object, with whitespace around it and, leniently, bytes behind it."""
    body = gap(rng, wsp) + obj(rng, members, wsp) + gap(rng, wsp)
    if lp and rng.random() < lp:
        body += rng.choice((b"x", b"{}", b",", b" 1", b"}", b"]", b"\x0c", b"\x0b", b"//"))
    return body


def pick_wsp(rng):
    return rng.choice((0, 0, 0, 0.1, 0.4, 1.0))


def request(rng, lp=0.03):
    wsp = pick_wsp(rng)
    return assemble(rng, request_members(rng, wsp, lp), wsp, lp)


# ---- the other classes ----------------------------------------------------------------------
def grammar(rng):
    """Random JSON: mostly an object at the root, with the envelope's keys among its keys."""
    wsp, lp = pick_wsp(rng), rng.choice((0, 0.05, 0.15))
    if rng.random() < 0.1:
        return gap(rng, wsp) + rand_value(rng, lp, wsp) + gap(rng, wsp)
    members = [(rand_key(rng, lp), rand_value(rng, lp, wsp, 1)) for _ in range(rng.randrange(0, 7))]
    if rng.random() < 0.6:
        members.insert(rng.randrange(len(members) + 1), (b'"method"', method_value(rng, rng.randrange(7), lp) or b"1"))
    return assemble(rng, members, wsp, lp)


def edited(rng):
    """A request with 2 to 4 random edits."""
    b = bytearray(request(rng))
    for _ in range(rng.randrange(2, 5)):
        at = rng.randrange(len(b)) if b else 0
        how = rng.randrange(6)
        if not b or how == 0:
            b.insert(at, rng.choice(EDIT_POOL))
        elif how == 1:
            b[at] = rng.choice(EDIT_POOL)
        elif how == 2:
            del b[at]
        elif how == 3:
            b[at] ^= 1 << rng.randrange(8)
        elif how == 4:
            del b[at:at + rng.randrange(1, 12)]
        else:
            b[at:at] = b[at:at + rng.randrange(1, 12)]
    return bytes(b) or b"{"


def splice(rng):
    a, b = request(rng), request(rng)
    return a[:rng.randrange(len(a) + 1)] + b[rng.randrange(len(b) + 1):] or b"}"


def with_nul(rng):
    """A 0 byte inside: the reference reads the C string up to it."""
    b = request(rng, lp=0)
    r = rng.random()
    if r < 0.4:
        return b + b"\0" + rng.choice((b"", b"x", b"}", request(rng, lp=0)))
    at = rng.randrange(len(b) + 1)
    return b[:at] + b"\0" + b[at:]


def tiny(rng):
    if rng.random() < 0.5:
        return rng.choice((b"{}", b"[]", b"0", b'""', b"{", b"}", b" ", b"null", b"{ }", b'{"":0}', b'{"id":1}', b"\xff",
                           b"-"))
    return bytes(rng.choice(EDIT_POOL) for _ in range(rng.randrange(1, 5)))


def _nest(rng, levels, wsp):
    """JSON text that nests exactly `levels` deep (levels >= 1), arrays and objects mixed, with
    shallow siblings on the way down."""
    text = rng.choice((b"[]", b"{}"))
    for _ in range(levels - 1):
        side = [scalar(rng, 0) for _ in range(rng.choice((0, 0, 1)))]
        if rng.random() < 0.6:
            text = array(rng, side + [text], wsp)
        else:
            text = obj(rng, [(rand_string(rng, 0, most=4), v) for v in side + [text]], wsp)
    return text


def _with_params(rng, wsp, value):
    members = request_members(rng, wsp, 0, params=False)
    members = [kv for kv in members if kv[0] != b'"params"']
    members.insert(rng.randrange(len(members) + 1), (b'"params"', value))
    return members


def deep_pair(seed, depth):
    """A request whose `params` nests to exactly `depth` (the root object is depth 1), and the
    same request one level deeper."""
    out = []
    for d in (depth, depth + 1):
        rng = random.Random(seed)
        wsp = rng.choice((0, 0, 0.2))
        head = _with_params(rng, wsp, b"@")
        inner = _nest(rng, d - 1, wsp)
        out.append(assemble(rng, [(k, inner if v == b"@" else v) for k, v in head], wsp))
    return out


def one_token(rng):
    return rng.choice((b"1", b"-2.5", b"true", b"null", b'"s"', b"0", b'"\\n"'))


def tokens_pair(seed, count):
    """A request of exactly `count` tokens and one of count + 1: `params` is an array of scalars
    (2k + 1 tokens for k of them), and a member "a":[] (five tokens) mends the parity.  The
    count is measured with the plain rules' own token counter."""
    for attempt in range(100):
        out = []
        for want in (count, count + 1):
            rng = random.Random(seed * 1000 + attempt)
            wsp = rng.choice((0, 0, 0.2))
            members = [kv for kv in request_members(rng, wsp, 0, params=False) if kv[0] != b'"params"']
            at, fill = rng.randrange(len(members) + 1), random.Random(rng.getrandbits(32))
            tail = random.Random(rng.getrandbits(32))
            try:
                base = rc.Strict(obj(random.Random(0), members, 0)).tokens
            except rc.Defer:
                break
            extra = [] if (want - base) % 2 == 0 else [(b'"a"', b"[]")]
            k = (want - base - 4 - 5 * len(extra)) // 2
            if k < 1 or not members:
                break
            value = array(fill, [one_token(fill) for _ in range(k)], wsp)
            full = members[:at] + [(b'"params"', value)] + members[at:] + extra
            out.append(assemble(tail, full, wsp))
        if len(out) == 2 and rc.Strict(out[0]).tokens == count:
            return out
    raise AssertionError("no request of %d tokens" % count)


def long_pair(seed, length):
    """A request of exactly `length` bytes and one of length + 1: padded inside a string (a
    member of the root or the string of strlen_s) or with whitespace behind the root."""
    for attempt in range(100):
        out = []
        for want in (length, length + 1):
            rng = random.Random(seed * 1000 + attempt)
            wsp = rng.choice((0, 0, 0.3))
            how = rng.randrange(3)
            ch = rng.choice((b"x", b"\xc3\xa9"[:1], b" ", b"\\\\"))
            members = request_members(rng, wsp, 0, params=how != 1)
            if how == 1:
                members = [kv for kv in members if kv[0] != b'"params"']
            asm = rng.getrandbits(32)

            def build(pad):
                if how == 0:
                    ms = members + [(b'"pad"', b'"' + pad + b'"')]
                elif how == 1:
                    ms = [(b'"params"', b'{"s":"' + pad + b'"}')] + members
                else:
                    return assemble(random.Random(asm), members, wsp) + b" " * len(pad)
                return assemble(random.Random(asm), ms, wsp)

            room = want - len(build(b""))
            if room < 0:
                break
            pad = ch * (room // len(ch)) + b"y" * (room % len(ch))
            out.append(build(pad))
        if len(out) == 2 and len(out[0]) == length and len(out[1]) == length + 1:
            return out
    raise AssertionError("no request of %d bytes" % length)


# ---- the corpus -----------------------------------------------------------------------------
class Corpus(NamedTuple):
    bodies: list
    pairs: list  # (limit's name, index of the body at the limit, index of its neighbour one past it)


#: (class, share of the corpus)
SHARES = [(request, 0.47), (grammar, 0.14), (edited, 0.14), (splice, 0.07), (with_nul, 0.04), (tiny, 0.01)]
LIMIT_SHARE, MUTATION_SHARE = 0.06, 0.07


@functools.lru_cache(maxsize=None)
def corpus(seed, count=34000):
    """`count` bodies of 1 to 1025 bytes, the classes shuffled into one another (so that a prefix
    is a smaller corpus of the same mix).  Cached: the callers share it and leave it unchanged."""
    rng = random.Random(seed)
    bodies, pairs = [], []
    for make, share in SHARES:
        for _ in range(int(count * share)):
            bodies.append(make(rng))
    for k in range(int(count * LIMIT_SHARE) // 2):
        what = ("depth", "tokens", "length")[k % 3]
        if what == "depth":
            pair = deep_pair(rng.getrandbits(32), rc.MAX_DEPTH - (k // 3) % 2 * rng.randrange(1, 4))
        elif what == "tokens":
            pair = tokens_pair(rng.getrandbits(32), rc.MAX_TOKENS - (k // 3) % 2 * rng.randrange(1, 4))
        else:
            pair = long_pair(rng.getrandbits(32), rc.MAX_BODY - (k // 3) % 2 * rng.randrange(1, 4))
        pairs.append((what, len(bodies), len(bodies) + 1))
        bodies += pair
    bodies += rc.mutation_set(seed ^ 0xF022, int(count * MUTATION_SHARE))
    while len(bodies) < count:
        bodies.append(request(rng))
    bodies = [b if 1 <= len(b) <= rc.MAX_BODY + 1 else b[:rc.MAX_BODY + 1] or b"{" for b in bodies]
    perm = list(range(len(bodies)))
    rng.shuffle(perm)  # perm[new] = old
    new_of = {old: new for new, old in enumerate(perm)}
    return Corpus([bodies[old] for old in perm], [(w, new_of[a], new_of[b]) for w, a, b in pairs])


# ---- the reference --------------------------------------------------------------------------
def reference(bodies):
    """oracle.ref_dispatch, or a failed test with the build hint when the binary is missing."""
    import pytest
    from oracle import oracle
    replies = oracle.ref_dispatch(bodies)
    if replies is None:
        pytest.fail("oracle/_ref/ref_dispatch missing: build it with `make -C oracle dispatch` (needs the reference tree)")
    assert len(replies) == len(bodies) and all(r is not None for r in replies)
    return replies


@functools.lru_cache(maxsize=None)
def answers(seed, count=34000):
    """The reference's reply to every body of corpus(seed, count) (cached)."""
    return reference(corpus(seed, count).bodies)


@functools.lru_cache(maxsize=None)
def ruled(seed, count=34000):
    """The plain rules' row of every body of corpus(seed, count) (cached)."""
    return [rc.route_body(b) for b in corpus(seed, count).bodies]


# ---- the properties -------------------------------------------------------------------------
def request_of(row, body):
    """B': the canonical request that says what a CALL row says -- the table's name for the
    method, the span's bytes as they are, the id."""
    _, m, rid, po, pl = row
    params = b'"params":' + bytes(body[po:po + pl]) + b"," if pl else b""
    return b'{"jsonrpc":"2.0","method":"%s",%s"id":%d}' % (rc.METHODS[m], params, rid)


def handler_output(rid, reply):
    """(status, value) a handler would hand back, cut from the reference's reply to B': the text
    between `"result":` and the final `}`, or the error's code."""
    head = b'{"jsonrpc":"2.0","id":%d,' % rid
    assert reply.startswith(head) and reply.endswith(b"}"), reply
    rest = reply[len(head):]
    if rest.startswith(b'"result":'):
        return 0, rest[len(b'"result":'):-1]
    assert rest.startswith(b'"error":{"code":'), reply
    return int(rest[len(b'"error":{"code":'):rest.index(b",")]), b""


def hold_route(bodies, replies, rows):
    """Properties a, b and c for one layer's rows (kind, method, id, params_off, params_len)
    against the reference's replies.  Returns the handlers' (status, value) per entry -- for a
    DEFER row the reference's whole reply, to go through the reply as a RAW value."""
    assert len(bodies) == len(replies) == len(rows)
    calls = [i for i, row in enumerate(rows) if row[0] == rc.CALL]
    for i in calls:
        _, m, _, po, pl = rows[i]
        assert m < len(rc.METHODS) and po + pl <= len(bodies[i]) and (pl or not po), (bodies[i], rows[i])
    again = dict(zip(calls, reference([request_of(rows[i], bodies[i]) for i in calls])))
    handled = []
    for i, (body, reply, row) in enumerate(zip(bodies, replies, rows)):
        kind, _, rid = row[:3]
        assert kind in (rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER), (body, row)
        if reply == PARSE_ERROR:  # a
            assert kind == rc.DEFER, (body, reply, row)
        if kind == rc.DEFER:
            handled.append((0, reply))
        elif kind == rc.CALL:  # c
            assert again[i] == reply != PARSE_ERROR, (body, row, request_of(row, body), again[i], reply)
            handled.append(handler_output(rid, again[i]))
        else:  # b
            code = -32601 if kind == rc.NOT_FOUND else -32600
            assert rp.error_body(rid, code, rp.MESSAGES[code]) == reply, (body, reply, row)
            handled.append((0, b""))
    return handled


def reply_case(rows, handled, front=b"~"):
    """The reply's inputs from a route's rows and the handlers' outputs (property d)."""
    values, ents = bytearray(front), []
    for row, (status, value) in zip(rows, handled):
        ents.append((rp.DATA, row[0], row[2], status, len(values), len(value)))
        values += value
    return rp.Case("fuzz", bytes(values), ents, [0, len(ents)], typed=False)


def hold_replies(bodies, replies, offs, lens, out):
    """Property d: every built body is the reference's reply, byte for byte."""
    assert len(replies) == len(offs) == len(lens)
    for body, reply, at, ln in zip(bodies, replies, offs, lens):
        assert out[at:at + ln] == reply, (body, reply, out[at:at + ln])


# ---- what keeps the comparison from being empty ---------------------------------------------
def spaced(body):
    """Whitespace outside the strings of a body of the strict subset."""
    inside, k = False, 0
    while k < len(body):
        c = body[k]
        if inside:
            k += c == 0x5C
            inside = c != 0x22
        elif c == 0x22:
            inside = True
        elif c in WS:
            return True
        k += 1
    return False


def depth_of(body):
    """The deepest nesting of a body that is well-formed JSON (the root is depth 1)."""
    inside, k, d, most = False, 0, 0, 0
    while k < len(body):
        c = body[k]
        if inside:
            k += c == 0x5C
            inside = c != 0x22
        elif c == 0x22:
            inside = True
        elif c in b"[{":
            d += 1
            most = max(most, d)
        elif c in b"]}":
            d -= 1
        k += 1
    return most


def tokens_of(body):
    """The tokens of a body that is well-formed JSON: brackets, commas, colons, strings, and
    numbers and literals as one each."""
    inside, k, n, run = False, 0, 0, False
    while k < len(body):
        c = body[k]
        if inside:
            k += c == 0x5C
            inside = c != 0x22
        elif c == 0x22 or c in b"[]{},:":
            inside, run, n = c == 0x22, False, n + 1
        elif c in WS:
            run = False
        else:
            n, run = n + (not run), True
        k += 1
    return n


def code_of(reply):
    """The code of an error reply."""
    at = reply.index(b'"error":{"code":') + len(b'"error":{"code":')
    return int(reply[at:reply.index(b",", at)])


def conditions(made, replies, rules):
    """The corpus reaches both sides of the comparison and every class named below; decided by
    the plain rules (`rules`: route_body's rows) and the reference's replies alone.  Returns the
    counts."""
    bodies = made.bodies
    assert all(1 <= len(b) <= rc.MAX_BODY + 1 for b in bodies)
    assert {len(b) for b in bodies} >= {1, 2, rc.MAX_BODY - 1, rc.MAX_BODY, rc.MAX_BODY + 1}
    n = {k: 0 for k in ("accepted", "routed", "parse errors", "results", -32602, -32601, -32600, "spans", "no params",
                        "whitespace", "order", "duplicate", "backslash", "nul", "nul accepted", "object", "array", "string",
                        "number", "literal")}
    offsets = set()
    for body, reply, row in zip(bodies, replies, rules):
        nul = 0 in body
        n["nul"] += nul
        if reply == PARSE_ERROR:
            n["parse errors"] += 1
            assert row[0] == rc.DEFER, (body, row)
            continue
        n["accepted"] += 1
        n["nul accepted"] += nul
        if nul:
            assert row[0] == rc.DEFER, (body, row)
        if row[0] == rc.DEFER:
            continue
        n["routed"] += 1
        if b'"result":' in reply[:48]:
            n["results"] += 1
        else:
            n[code_of(reply)] += 1
        members = rc.Strict(body).members
        keys = [m[0] for m in members]
        first = [k for j, k in enumerate(keys) if k in ENVELOPE and k not in keys[:j]]
        n["whitespace"] += spaced(body)
        n["order"] += first != [k for k in ENVELOPE if k in first]
        n["duplicate"] += len(set(keys)) < len(keys)
        n["backslash"] += any(b"\\" in body[m[3]:m[4]] for m in members)
        if row[0] == rc.CALL:
            if row[4]:
                n["spans"] += 1
                offsets.add(row[3])
                n[next(m[2] for m in members if m[0] == b"params")] += 1
            else:
                n["no params"] += 1
    assert 2 * n["routed"] >= n["accepted"], n
    assert n["parse errors"] >= 5000, n
    assert min(n["results"], n[-32602], n[-32601], n[-32600]) >= 500, n
    assert n["spans"] >= 2000 and len(offsets) >= 100 and n["no params"] >= 200, (n, len(offsets))
    for what in ("whitespace", "order", "duplicate", "backslash", "object", "array", "string", "number", "literal"):
        assert n[what] >= 100, (what, n)
    assert n["nul"] >= 100 and n["nul accepted"] >= 20, n
    # the limits: a routed body exactly at each, and its neighbour one past it defers
    at_limit = {"depth": 0, "tokens": 0, "length": 0}
    for what, a, b in made.pairs:
        measure = {"depth": depth_of, "tokens": tokens_of, "length": len}[what]
        limit = {"depth": rc.MAX_DEPTH, "tokens": rc.MAX_TOKENS, "length": rc.MAX_BODY}[what]
        if rules[a][0] == rc.DEFER or measure(bodies[a]) != limit:
            continue
        at_limit[what] += 1
        assert what != "tokens" or rc.Strict(bodies[a]).tokens == limit  # (the rules' own count)
        assert measure(bodies[b]) == limit + 1, (what, bodies[b])
        assert rules[b][0] == rc.DEFER and replies[b] != PARSE_ERROR, (what, bodies[b])
    assert min(at_limit.values()) >= 1, at_limit
    n["offsets"], n["at a limit"] = len(offsets), at_limit
    return n
