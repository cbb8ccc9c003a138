"""Rows for holding the frame values against the live reference (tests/test_values_fuzz.py) and
for the golden fixture (tests/golden/make_values_golden.py).

RESULT form: a request whose handler returns a value we know as a typed slot --
mul_double(a=repr(d), b=1) returns d, add_i32(a, 0) returns a, echo_i64 its argument, is_even a
bool, mix3 and ping escape-free strings, strlen_s a length -- so the reference's reply carries
print_number(d), %d, the quoted %lld, true / false and the quoted string, and the value text of
the rules, wrapped by the reply's rule, must be that reply byte for byte.

PARAMS form: a params object built by the rules from typed values goes through the reference
client's encoder (tests/request_ref.py), which prints cJSON_PrintUnformatted of the parsed
params: the print must be the object itself.  (Not claimed for a double above
1.797693134862315e308: its text reads back as infinity, which cJSON prints as null.)"""
import random
import struct
from typing import NamedTuple

import args_cases as ac
import reply_cases as rp
import values_cases as vc
import values_numbers as vn
from args_cases import A, E, M, N, P, S, X

#: the result type each method's handler value has here (mix3 and ping return strings)
RESULT_TYPES = {P: vc.STR, E: vc.I64, A: vc.I32, M: vc.F64, N: vc.BOOL, S: vc.I32, X: vc.STR}
WORDS = [b"", b"a", b"hello", b"caf\xc3\xa9", b"x" * 40, b"with blanks and ~tilde", b"0123456789"]


class Row(NamedTuple):
    method: int
    span: object  # the `params` text, or None
    rid: int
    slot: int     # the typed result (a STR slot points into the batch's strings)


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def rows(seed, count):
    """(rows, strings): the requests and the string bytes their STR results point into."""
    rng = random.Random(seed)
    pool = [b for label, bs in vn.corpus().items() if label not in ("subnormals",) for b in bs]
    strings = bytearray(b"pong")
    out = []
    for k in range(count):
        m = rng.choice([M] * 8 + [A, E, N, X, P, S])
        rid = rng.getrandbits(32) if rng.random() < 0.2 else k + 1
        if m == M:
            bits = rng.choice(pool) if rng.random() < 0.8 else rng.getrandbits(64)
            if (bits >> 52) & 0x7FF == 0x7FF:
                bits &= ~(1 << 62)
            out.append(Row(M, b'{"a":%s,"b":1}' % repr(f64(bits)).encode(), rid, bits))
        elif m == A:
            a = rng.choice([0, 1, -1, 2**31 - 1, -2**31, rng.randrange(-2**31, 2**31)])
            out.append(Row(A, b'{"a":%d,"b":0}' % a, rid, a & vc.M64))
        elif m == E:
            x = rng.choice([0, -1, 2**63 - 1, -2**63, rng.randrange(-2**63, 2**63), rng.randrange(-10**6, 10**6)])
            out.append(Row(E, b'{"x":"%d"}' % x, rid, x & vc.M64))
        elif m == N:
            n = rng.randrange(-2**31, 2**31)
            out.append(Row(N, b'{"n":%d}' % n, rid, 1 if n % 2 == 0 else 0))
        elif m == S:
            w = rng.choice(WORDS)
            out.append(Row(S, b'{"s":"%s"}' % w, rid, len(w)))
        elif m == P:
            out.append(Row(P, None, rid, 0 | 4 << 32))
        else:
            a, b, ok = rng.randrange(-2**31, 2**31), rng.choice([0.5, -1.25, 12345.678, 1e5, 0.005, 3.0]), rng.random() < 0.5
            text = ("a=%d,b=%.2f,ok=%s" % (a, b, "true" if ok else "false")).encode()
            out.append(Row(X, b'{"a":%d,"b":%r,"ok":%s}' % (a, b, b"true" if ok else b"false"), rid, len(strings) | len(text) << 32))
            strings += text
    return out, bytes(strings)


def bodies_of(rs):
    return [ac.request(ac.IDL_METHODS[r.method][0], r.span, r.rid)[0] for r in rs]


def entries_of(rs):
    """The rows as RESULT-form entries: a method table of the seven IDL methods with RESULT_TYPES."""
    return [RESULT_TYPES[m] for m in range(7)], [vc.Entry(vc.MODE_ENCODE, 0, r.method, (r.slot,)) for r in rs]


def hold(rs, replies, layer, strings):
    """layer: (status, text) per row.  An OK row's text, wrapped by the reply's rule, is the
    reference's reply byte for byte; nothing but a subnormal defers.  Returns counts per status."""
    n = {vc.OK: 0, vc.DEFER: 0}
    for r, reply, (st, text) in zip(rs, replies, layer):
        assert st in n, (r, st)
        n[st] += 1
        if st == vc.OK:
            assert rp.result_body(r.rid, text) == reply, (r, text, reply)
        else:
            assert r.method == M and vc.f64_text(r.slot) is None, r
    return n


# ---- PARAMS form ------------------------------------------------------------------------------
def params_rows(seed, count):
    """(entries over the IDL's schema at width 3, strings)."""
    rng = random.Random(seed)
    pool = [b for label, bs in vn.corpus().items() if label not in ("subnormals", "above_max15") for b in bs]
    strings = b'plain words caf\xc3\xa9 ~!#$%&()*+,-./:;<=>?@[]^_`{|} and "quoted" back\\slash \x01 end'
    clean = [(strings.index(w), len(w)) for w in (b"plain", b"plain words", b"caf\xc3\xa9", b"~!#$%&()*+,-./:;<=>?@[]^_`{|}", b"")]
    dirty = [(strings.index(w), len(w)) for w in (b'"quoted"', b"back\\slash", b"\x01")]
    es = []
    for _ in range(count):
        m = rng.randrange(0, 7)
        slots = []
        for p in range(ac.IDL.first[m], ac.IDL.first[m + 1]):
            t = ac.IDL.types[p]
            if t == vc.STR:
                at, ln = rng.choice(clean * 4 + dirty)
                slots.append(at | ln << 32)
            elif t == vc.F64:
                b = rng.choice(pool)
                slots.append(b if vc.double_of(b & ~vn.SIGN) <= 1.797693134862315e308 else vc.bits_of(1.5))
            else:
                slots.append(rng.getrandbits(64))
        es.append(vc.Entry(vc.MODE_ENCODE, 0, m, tuple(slots) + (0,) * (3 - len(slots))))
    return es, strings
