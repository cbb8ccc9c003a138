"""The frame args' rules (include/rpccrc.h, rpc_frames_args_device) in plain Python, and the
cases the emulator and the GPU are held against.

The strict subset is the route's hand-written descent (route_cases.Strict) started on any value;
the values come from Python's float() and int().  Nothing here shares code with
rpc_amd/csrc/frames_args.h."""
import math
import random
import re
import struct
from typing import NamedTuple

import route_cases as rc

NONE, OK, INVALID, DEFER, RANGE, BAD_SCHEMA = range(6)
I32, I64, F64, BOOL, STR = range(5)
MAX_PARAMS, MAX_SCHEMA_PARAMS, MAX_NAME_BYTES = 8, 1024, 4096
REPLY = {OK: 0, INVALID: -32602}  # everything else: -32603
M64 = (1 << 64) - 1

#: the IDL's seven methods with their parameters, in the order of route_cases.METHODS
IDL_METHODS = [
    (b"ping", []),
    (b"echo_i64", [(b"x", I64)]),
    (b"add_i32", [(b"a", I32), (b"b", I32)]),
    (b"mul_double", [(b"a", F64), (b"b", F64)]),
    (b"is_even", [(b"n", I32)]),
    (b"strlen_s", [(b"s", STR)]),
    (b"mix3", [(b"a", I32), (b"b", F64), (b"ok", BOOL)]),
]


class Schema(NamedTuple):
    first: list   # nmethods + 1 words (broken words are allowed: BAD_SCHEMA)
    types: list   # nparams
    noff: list    # nparams + 1 words
    names: bytes

    @property
    def nmethods(self):
        return len(self.first) - 1 if self.first else 0


def schema_of(methods):
    first, types, noff, names = [0], [], [0], bytearray()
    for _, params in methods:
        for name, t in params:
            types.append(t)
            names += name
            noff.append(len(names))
        first.append(len(types))
    return Schema(first, types, noff, bytes(names))


IDL = schema_of(IDL_METHODS)


class Span(rc.Strict):
    """route_cases.Strict started on any value with nothing around it.  ``kind`` is the value's
    type; for an object ``members`` are its depth-1 members.  The span's outermost container is
    depth 1 and the limit is MAX_DEPTH - 1: the walk starts one level down."""

    def __init__(self, b):
        self.b, self.i, self.tokens = b, 0, 0
        self.members = None
        if b[:1] == b"{":
            self.kind, self.members = "object", self.obj(2, True)
        else:
            self.kind = self.value(1)[0]
        if self.i != len(b):
            raise rc.Defer("bytes behind the value")


def bits_of(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def f64_of(text):
    """Rule 10, F64: the double's bits, or None for DEFER."""
    mant = re.split(rb"[eE]", text.lstrip(b"-"))[0].replace(b".", b"").lstrip(b"0")
    f = float(text)
    if not mant:
        return bits_of(f)  # every digit is 0: +-0
    if len(mant) > 19 or f == 0 or math.isinf(f) or abs(f) < 2.0 ** -1022:
        return None
    return bits_of(f)


def convert(t, vt, text, esc, off):
    """Rule 10 for one value the type takes: the slot, or None for DEFER.  ``text``: a number's
    bytes, or a string's bytes between the quotes, which lie at ``off`` in the body."""
    if t == BOOL:
        return 1 if text == b"true" else 0
    if t == STR:
        return None if esc else off | len(text) << 32
    if vt == "string":  # I64, the strtoll path
        if esc or not re.fullmatch(rb"-?[0-9]{1,19}", text) or not -2**63 <= int(text) < 2**63:
            return None
        return int(text) & M64
    bits = f64_of(text)
    if bits is None or t == F64:
        return bits
    d = float(text)
    inside = -2147483649 < d < 2147483648 if t == I32 else -2.0**63 <= d < 2.0**63
    return int(d) & M64 if inside else None


def takes(t, vt, text):
    if vt == "number":
        return t in (I32, I64, F64)
    if vt == "string":
        return t in (STR, I64)
    return vt == "literal" and text in (b"true", b"false") and t == BOOL


def args_span(span, base, params):
    """Rules 5-10 for one span that lies inside its body, for a method with parameters
    ``params`` [(name, type), ...] (at least one): (status, slots in declaration order)."""
    none = [0] * len(params)
    if len(span) == 0:
        return INVALID, none
    if len(span) > rc.MAX_BODY:
        return DEFER, none
    try:
        s = Span(bytes(span))
    except rc.Defer:
        return DEFER, none
    if s.kind != "object":
        return INVALID, none
    if any(kesc for _, kesc, *_ in s.members):
        return DEFER, none
    first = {}
    for m in s.members:
        first.setdefault(m[0], m)
    if any(name not in first or not takes(t, first[name][2], span[first[name][3]:first[name][4]]) for name, t in params):
        return INVALID, none
    slots = []
    for name, t in params:
        _, _, vt, vs, ve, vesc = first[name]
        slots.append(convert(t, vt, bytes(span[vs:ve]), vesc, base + vs))
    if any(v is None for v in slots):
        return DEFER, none
    return OK, slots


def args_entries(buf, entries, schema=IDL, width=MAX_PARAMS):
    """Rules 1-10 over entries (body_off, body_len, kind, method, params_off, params_len) of
    ``buf``: (status, reply_status, the `width` slots) per entry."""
    out = []
    nparams = len(schema.types)
    for boff, blen, kind, method, poff, plen in entries:
        status, slots = None, []
        if kind != rc.CALL:
            status = NONE
        elif method >= schema.nmethods:
            status = BAD_SCHEMA
        else:
            a, b = schema.first[method], schema.first[method + 1]
            if not a <= b <= nparams or b - a > width or any(
                    schema.types[p] > STR or not schema.noff[p] <= schema.noff[p + 1] <= len(schema.names)
                    for p in range(a, b)):
                status = BAD_SCHEMA
            elif not (boff <= len(buf) and blen <= len(buf) - boff and poff <= blen and plen <= blen - poff):
                status = RANGE
            elif a == b:
                status = OK
            else:
                params = [(schema.names[schema.noff[p]:schema.noff[p + 1]], schema.types[p]) for p in range(a, b)]
                status, slots = args_span(buf[boff + poff:boff + poff + plen], poff, params)
        slots = (list(slots) if status == OK else []) + [0] * width
        out.append((status, REPLY.get(status, -32603), tuple(slots[:width])))
    return out


# ---- requests and their entries ---------------------------------------------------------------
def request(method, span, rid=1, front=b""):
    """A request body with ``span`` as its `params` (None: no `params`) and its entry fields
    (method index is the caller's): (body, params_off, params_len)."""
    head = front + b'{"jsonrpc":"2.0","method":"' + method + b'",'
    if span is None:
        return head + b'"id":%d}' % rid, 0, 0
    head += b'"params":'
    return head + span + b',"id":%d}' % rid, len(head), len(span)


def back_to_back(reqs, methods=IDL_METHODS, pad_front=0, nul=1):
    """(method index, span) requests as the unpack leaves their bodies, with CALL entries."""
    buf, entries = bytearray(b"#" * pad_front), []
    for k, (m, span) in enumerate(reqs):
        body, po, pl = request(methods[m][0], span, rid=k)
        entries.append((len(buf), len(body), rc.CALL, m, po, pl))
        buf += body + b"\0" * nul
    return bytes(buf), entries


def f64(x):
    return bits_of(float(x))


def i(x):
    return x & M64


P, E, A, M, N, S, X = range(7)  # ping echo_i64 add_i32 mul_double is_even strlen_s mix3
_nest31 = b'{"n":1,"z":' + b"[" * 30 + b"]" * 30 + b"}"
_nest32 = b'{"n":1,"z":' + b"[" * 31 + b"]" * 31 + b"}"


def _tok(count):
    """{"n":1,"z":[1,1,...]} with exactly `count` tokens (count odd, >= 11): 10 around k numbers
    and k - 1 commas."""
    k = (count - 9) // 2
    return b'{"n":1,"z":[' + b",".join([b"1"] * k) + b"]}"


#: (name, method, span or None, status, slots or None) -- written down by hand from the rules
CASES = [
    # rule 4: a method without parameters takes anything
    ("ping {}", P, b"{}", OK, []),
    ("ping absent", P, None, OK, []),
    ("ping array", P, b"[1,2]", OK, []),
    # rule 5
    ("absent params", A, None, INVALID, None),
    # rule 6
    ("leading blank", N, b' {"n":1}', DEFER, None),
    ("trailing blank", N, b'{"n":1} ', DEFER, None),
    ("inner blanks", N, b'{ "n" :\t1\r\n}', OK, [1]),
    ("leading zero", N, b'{"n":01}', DEFER, None),
    ("wrong type but not strict", N, b'{"n":"x","z":01}', DEFER, None),
    ("u escape", S, b'{"s":"\\u0041"}', DEFER, None),
    ("control byte", S, b'{"s":"a\x01"}', DEFER, None),
    ("ends in a string", S, b'{"s":"abc', DEFER, None),
    ("ends in a number", N, b'{"n":12', DEFER, None),
    ("two values", N, b'{"n":1}{"n":2}', DEFER, None),
    ("trailing comma", N, b'{"n":1,}', DEFER, None),
    ("depth 31", N, _nest31, OK, [1]),
    ("depth 32", N, _nest32, DEFER, None),
    ("tokens 255", N, _tok(255), OK, [1]),
    ("tokens 256", N, _tok(251)[:-1] + b',"y":[]}', OK, [1]),
    ("tokens 257", N, _tok(257), DEFER, None),
    ("span 1024", S, b'{"s":"' + b"x" * 1016 + b'"}', OK, None),
    ("span 1025", S, b'{"s":"' + b"x" * 1017 + b'"}', DEFER, None),
    # rule 7: the issue's probes
    ("array", A, b"[1,2]", INVALID, None),
    ("null", A, b"null", INVALID, None),
    ("string", A, b'"a"', INVALID, None),
    ("number", A, b"12", INVALID, None),
    ("number with exponent", A, b"-1.5e+3", INVALID, None),
    ("true", A, b"true", INVALID, None),
    ("empty array", A, b"[]", INVALID, None),
    ("bad root number", A, b"1.", DEFER, None),
    ("bad literal", A, b"nul", DEFER, None),
    # rule 8
    ("escaped key", N, b'{"n":1,"a\\/b":2}', DEFER, None),
    ("escaped key wins over a wrong type", N, b'{"n":null,"a\\/b":2}', DEFER, None),
    ("escaped key nested", N, b'{"n":1,"z":{"a\\/b":2}}', OK, [1]),
    ("first key wins", A, b'{"a":1,"a":5,"b":2}', OK, [1, 2]),
    ("case matters", A, b'{"A":1,"a":3,"b":2}', OK, [3, 2]),
    ("extras and nesting", A, b'{"a":1,"b":2,"c":{"a":9}}', OK, [1, 2]),
    ("nested first", A, b'{"c":{"a":9,"b":9},"b":2,"a":1}', OK, [1, 2]),
    ("prefix and longer keys", A, b'{"aa":7,"":8,"a":1,"b":2}', OK, [1, 2]),
    ("first key wrong, second right", A, b'{"a":"x","a":5,"b":2}', INVALID, None),
    # rule 9
    ("absent parameter", A, b'{"a":1}', INVALID, None),
    ("empty object", A, b"{}", INVALID, None),
    ("0 for a bool", X, b'{"a":1,"b":2,"ok":0}', INVALID, None),
    ("null for a number", A, b'{"a":null,"b":2}', INVALID, None),
    ("null for a string", S, b'{"s":null}', INVALID, None),
    ("null for an i64", E, b'{"x":null}', INVALID, None),
    ("null for a bool", X, b'{"a":1,"b":2,"ok":null}', INVALID, None),
    ("string for an i32", A, b'{"a":"1","b":2}', INVALID, None),
    ("string for a double", M, b'{"a":"1","b":2}', INVALID, None),
    ("number for a string", S, b'{"s":5}', INVALID, None),
    ("bool for an i32", N, b'{"n":true}', INVALID, None),
    ("bool for an i64", E, b'{"x":false}', INVALID, None),
    ("object for an i32", N, b'{"n":{"n":1}}', INVALID, None),
    ("array for a string", S, b'{"s":["a"]}', INVALID, None),
    ("invalid wins over defer", A, b'{"a":1e400,"b":"x"}', INVALID, None),
    ("invalid wins over defer, absent", A, b'{"a":2147483648}', INVALID, None),
    # rule 10: F64
    ("doubles", M, b'{"a":0.5,"b":-1.25}', OK, [f64(0.5), f64(-1.25)]),
    ("-0.0", M, b'{"a":-0.0,"b":0}', OK, [0x8000000000000000, 0]),
    ("zero with an exponent", M, b'{"a":0e999,"b":-0.000e-999}', OK, [0, 0x8000000000000000]),
    ("exponent forms", M, b'{"a":1E+2,"b":2.5e-3}', OK, [f64(100.0), f64(0.0025)]),
    ("19 digits", M, b'{"a":1234567890123456789,"b":0.0001234567890123456789}', OK,
     [f64(1234567890123456789), f64("0.0001234567890123456789")]),
    ("20 digits", M, b'{"a":12345678901234567890,"b":1}', DEFER, None),
    ("20 digits, trailing zeros", M, b'{"a":1.0000000000000000000,"b":1}', DEFER, None),
    ("1e400", M, b'{"a":1e400,"b":1}', DEFER, None),
    ("1e-400", M, b'{"a":1,"b":1e-400}', DEFER, None),
    ("subnormal", M, b'{"a":1,"b":4.9e-324}', DEFER, None),
    ("just below the smallest normal", M, b'{"a":1,"b":2.225073858507201136e-308}', DEFER, None),
    ("rounds up to the smallest normal", M, b'{"a":1,"b":2.225073858507201137e-308}', OK, [f64(1), 1 << 52]),
    ("largest double", M, b'{"a":1.7976931348623157e308,"b":1}', OK, [0x7FEFFFFFFFFFFFFF, f64(1)]),
    ("overflows", M, b'{"a":1.7976931348623159e308,"b":1}', DEFER, None),
    ("a tie the table's e >= -27 branch decides", M, b'{"a":63863781979156355e-1,"b":9007199254740993}', OK,
     [f64("63863781979156355e-1"), f64(9007199254740992)]),
    ("huge exponent digits", M, b'{"a":1e99999999999999999999,"b":1}', DEFER, None),
    # I32
    ("i32 truncates", A, b'{"a":1.9,"b":-1.9}', OK, [1, i(-1)]),
    ("i32 exponent", A, b'{"a":1e3,"b":-0.0}', OK, [1000, 0]),
    ("i32 edges", A, b'{"a":2147483647,"b":-2147483648}', OK, [2147483647, i(-2147483648)]),
    ("i32 fractions at the edges", A, b'{"a":2147483647.9,"b":-2147483648.9}', OK, [2147483647, i(-2147483648)]),
    ("i32 above", A, b'{"a":2147483648,"b":1}', DEFER, None),
    ("i32 below", A, b'{"a":1,"b":-2147483649}', DEFER, None),
    ("i32 far out", N, b'{"n":1e300}', DEFER, None),
    ("i32 tiny", N, b'{"n":1e-300}', OK, [0]),
    ("i32 from a subnormal", N, b'{"n":1e-320}', DEFER, None),
    # I64
    ("i64 string", E, b'{"x":"-9223372036854775808"}', OK, [i(-2**63)]),
    ("i64 string max", E, b'{"x":"9223372036854775807"}', OK, [2**63 - 1]),
    ("i64 string over", E, b'{"x":"9223372036854775808"}', DEFER, None),
    ("i64 string under", E, b'{"x":"-9223372036854775809"}', DEFER, None),
    ("i64 string 19 nines", E, b'{"x":"9999999999999999999"}', DEFER, None),
    ("i64 string 20 digits", E, b'{"x":"00000000000000000001"}', DEFER, None),
    ("i64 string leading zeros", E, b'{"x":"-007"}', OK, [i(-7)]),
    ("i64 string -0", E, b'{"x":"-0"}', OK, [0]),
    ("i64 string blank", E, b'{"x":" 12"}', DEFER, None),
    ("i64 string plus", E, b'{"x":"+12"}', DEFER, None),
    ("i64 string junk", E, b'{"x":"12a"}', DEFER, None),
    ("i64 string empty", E, b'{"x":""}', DEFER, None),
    ("i64 string minus", E, b'{"x":"-"}', DEFER, None),
    ("i64 string escape", E, b'{"x":"1\\/2"}', DEFER, None),
    ("i64 number", E, b'{"x":9007199254740993}', OK, [9007199254740992]),
    ("i64 number truncates", E, b'{"x":-2.5e3}', OK, [i(-2500)]),
    ("i64 number -2^63", E, b'{"x":-9223372036854775808}', OK, [i(-2**63)]),
    ("i64 number 2^63", E, b'{"x":9223372036854775808}', DEFER, None),
    ("i64 number below 2^63", E, b'{"x":9223372036854774784}', OK, [9223372036854774784]),
    # BOOL and STR
    ("mix3", X, b'{"ok":false,"b":2.5,"a":-7}', OK, [i(-7), f64(2.5), 0]),
    ("mix3 true", X, b'{"a":1,"b":2,"ok":true}', OK, [1, f64(2), 1]),
    ("string", S, b'{"s":"hello"}', OK, None),
    ("empty string", S, b'{"s":""}', OK, None),
    ("string with high bytes", S, b'{"s":"\xc3\xa9\xff"}', OK, None),
    ("string with an escape", S, b'{"s":"a\\nb"}', DEFER, None),
    ("long string", S, b'{"s":"' + b"abcdefg" * 40 + b'"}', OK, None),
]


def case_entries(pad_front=3):
    """The table as one buffer and its entries, with entries of the other statuses among them:
    (buf, entries)."""
    buf, entries = back_to_back([(m, span) for _, m, span, _, _ in CASES], pad_front=pad_front)
    buf = bytearray(buf)
    body, po, pl = request(b"is_even", b'{"n":4}')
    at = len(buf)
    buf += body  # (the buffer ends with this body's last byte)
    entries += [(at, len(body), k, N, po, pl) for k in (rc.NONE, rc.NOT_FOUND, rc.INVALID, rc.DEFER, rc.RANGE, 6, 255)]
    entries += [
        (1 << 62, 5, rc.NONE, 0xFFFF, 1 << 31, 1 << 31),   # rule 1: nothing else is looked at
        (at, len(body), rc.CALL, 7, po, pl),               # rule 2: no such method
        (at, len(body), rc.CALL, 0xFFFF, po, pl),
        (at + 1, len(body), rc.CALL, N, po, pl),           # rule 3: the body leaves the buffer by a byte
        (len(buf) + 1, 0, rc.CALL, N, 0, 0),               # starts behind the end
        (2**64 - 2, 8, rc.CALL, N, 0, 4),                  # would wrap
        (at, len(body), rc.CALL, N, po, len(body) - po + 1),  # the span leaves the body by a byte
        (at, len(body), rc.CALL, N, len(body) + 1, 0),     # starts behind the body
        (at, len(body), rc.CALL, N, 0xFFFFFFFF, 2),        # would wrap in 32 bits
        (1 << 62, 5, rc.CALL, P, 0, 0),                    # rule 3 comes before rule 4
        (at, len(body), rc.CALL, N, po, pl),               # a span that ends two bytes before the buffer does
        (at, len(body), rc.CALL, S, len(body) - 1, 1),     # ... and one on its last byte: "}" alone
        (at, len(body), rc.CALL, N, len(body), 0),         # empty at the body's end: inside, rule 5
    ]
    return bytes(buf), entries


# ---- canonical and mutated params -----------------------------------------------------------
def print_number(d):
    """cJSON's print_number, as the reference prints an i32 or a double."""
    if math.isinf(d) or math.isnan(d):
        return b"null"
    if d == int(d) and abs(d) < 2**31:
        return b"%d" % int(d)
    s = "%1.15g" % d
    if abs(float(s) - d) > max(abs(float(s)), abs(d)) * 2.0 ** -52:  # (cJSON's compare_double)
        s = "%1.17g" % d
    return s.encode()


def rand_double(rng):
    r = rng.random()
    if r < 0.3:
        return rng.choice([0.5, -1.25, 3.0, 1e20, 2.5e-7, 12345.678, 0.1, -0.0, 1e300, 1e-300, 5e-324 * 2**60])
    if r < 0.6:
        return rng.uniform(-1e6, 1e6)
    return struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64) & ~(0x7FF << 52) | rng.randrange(1, 0x7FF) << 52))[0]


def canonical_span(rng, m):
    """`params` of IDL method m as the reference client's stubs print it (rpc_client_gen.c):
    numbers through print_number, an i64 as a decimal string, strings with nothing to escape."""
    i32 = lambda: b"%d" % rng.choice([rng.randrange(-2**31, 2**31), rng.randrange(-100, 100), -2**31, 2**31 - 1])  # noqa: E731
    dbl = lambda: print_number(rand_double(rng))  # noqa: E731
    if m == P:
        return b"{}"
    if m == E:
        return b'{"x":"%d"}' % rng.choice([rng.randrange(-2**63, 2**63), rng.randrange(-1000, 1000), -2**63, 2**63 - 1])
    if m == A:
        return b'{"a":%s,"b":%s}' % (i32(), i32())
    if m == M:
        return b'{"a":%s,"b":%s}' % (dbl(), dbl())
    if m == N:
        return b'{"n":%s}' % i32()
    if m == S:
        alphabet = "abcdefghijklmnopqrstuvwxyz0123456789 _-/é中{}[]:,"
        return b'{"s":"%s"}' % "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 60))).encode()
    return b'{"a":%s,"b":%s,"ok":%s}' % (i32(), dbl(), rng.choice([b"true", b"false"]))


def canonical_set(seed, count):
    rng = random.Random(seed)
    return [(k % 7, canonical_span(rng, k % 7)) for k in range(count)]


def mutation_set(seed, count):
    """Canonical params with one byte flipped, inserted or deleted, or truncated."""
    rng = random.Random(seed)
    base = [(m, s) for m, s in canonical_set(seed ^ 0x5EED, 96) if m != P]
    pool = b'{}[],:"\\ \t\n\r0123456789-+.eEtfnu/abnsxok\x00\x01\x1f\x7f\x80\xff'
    out = []
    for _ in range(count):
        m, s = rng.choice(base)
        b = bytearray(s)
        at = rng.randrange(len(b))
        how = rng.randrange(4)
        if how == 0:
            b[at] = rng.choice(pool) if rng.random() < 0.8 else b[at] ^ (1 << rng.randrange(8))
        elif how == 1:
            b.insert(at, rng.choice(pool))
        elif how == 2:
            del b[at]
        else:
            del b[at:]
        out.append((m, bytes(b)))
    return out


# ---- other schemas --------------------------------------------------------------------------
def schema_cases():
    """(name, schema, width, buf, entries, wanted statuses or None): a method with 0 and one with
    8 parameters, width 1, the empty name, a repeated name, and every BAD_SCHEMA cause of a
    schema's own words (each beside methods that stay sound)."""
    out = []
    eight = [(b"none", []), (b"eight", [(b"p%d" % k, (I32, I64, F64, BOOL, STR)[k % 5]) for k in range(8)])]
    reqs = [(0, b'{"p0":1}'), (1, b'{"p7":1.5,"p6":"2","p5":3,"p4":"s","p3":true,"p2":0.25,"p1":"-5","p0":7}'),
            (1, b'{"p0":7,"p1":"-5","p2":0.25,"p3":true,"p4":"s","p5":3,"p6":"2"}'), (0, None)]
    buf, entries = back_to_back(reqs, eight)
    out.append(("0 and 8 parameters", schema_of(eight), 8, buf, entries, [OK, OK, INVALID, OK]))
    buf, entries = back_to_back([(N, b'{"n":5}'), (A, b'{"a":1,"b":2}'), (P, b"{}"), (S, b'{"s":"x"}')])
    out.append(("width 1", IDL, 1, buf, entries, [OK, BAD_SCHEMA, OK, OK]))
    named = [(b"m", [(b"", I32), (b"a", I32)])]
    buf, entries = back_to_back([(0, b'{"":1,"a":2}'), (0, b'{"a":2}'), (0, b'{"a":2,"b":3,"":4,"":5}')], named)
    out.append(("empty name", schema_of(named), 2, buf, entries, [OK, INVALID, OK]))
    twice = [(b"m", [(b"a", I32), (b"a", F64), (b"b", I64)])]
    buf, entries = back_to_back([(0, b'{"a":1.5,"b":"3","a":9}'), (0, b'{"a":"1","b":"3"}'), (0, b'{"b":4,"a":1e10}')], twice)
    out.append(("repeated name", schema_of(twice), 3, buf, entries, [OK, INVALID, DEFER]))
    three = [(b"m%d" % k, [(b"a", I32)]) for k in range(3)]
    buf, entries = back_to_back([(k, b'{"a":%d}' % (k + 1)) for k in range(3)], three)
    sound = schema_of(three)
    for name, broken, want in [
        ("CSR word runs backwards", sound._replace(first=[0, 2, 1, 3]), [OK, BAD_SCHEMA, OK]),
        ("CSR word leaves nparams", sound._replace(first=[0, 1, 2, 9]), [OK, OK, BAD_SCHEMA]),
        ("unknown type", sound._replace(types=[0, 5, 0]), [OK, BAD_SCHEMA, OK]),
        ("type 255", sound._replace(types=[255, 0, 0]), [BAD_SCHEMA, OK, OK]),
        ("name word runs backwards", sound._replace(noff=[0, 1, 0, 1]), [OK, BAD_SCHEMA, OK]),
        ("name word leaves the names", sound._replace(noff=[0, 1, 2, 4000]), [OK, OK, BAD_SCHEMA]),
    ]:
        out.append((name, broken, 2, buf, entries, want))
    return out
