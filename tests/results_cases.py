"""The frame results' rules (include/rpccrc.h, rpc_frames_results_device) in plain Python, and the
cases the emulator and the GPU are held against.

The strict subset, the type matrix and the conversions are the args' (args_cases.Span, takes,
convert, args_span: imported, not copied); the precedence, the two members, the per-slot part
and the count are written out here.  Nothing shares code with rpc_amd/csrc/frames_results.h."""
import random
from typing import NamedTuple

import args_cases as ac
import resolve_cases as rv
import route_cases as rc

NONE, OK, ABSENT, MISMATCH, DEFER, RANGE, BAD_SCHEMA = range(7)
STATUS_NAMES = ["NONE", "OK", "ABSENT", "MISMATCH", "DEFER", "RANGE", "BAD_SCHEMA"]
I32, I64, F64, BOOL, STR = ac.I32, ac.I64, ac.F64, ac.BOOL, ac.STR
M64 = ac.M64
ERROR_PARAMS = [(b"code", I32), (b"message", STR)]

#: the method table of the cases: method m has result type m, methods 5 and 6 a broken type
TYPES = [I32, I64, F64, BOOL, STR, 5, 255]


class Row(NamedTuple):
    status: int
    value: int          # 64-bit pattern
    error_status: int
    error_code: int     # signed 32-bit
    error_message: int  # offset | length << 32


def plain(status):
    return Row(status, 0, ABSENT, 0, 0)


def value_of(span, base, t):
    """Rules 4-7 for a `result` span inside a body of at most MAX_BODY bytes: (status, value)."""
    if len(span) == 0:
        return ABSENT, 0
    try:
        s = ac.Span(bytes(span))
    except rc.Defer:
        return DEFER, 0
    vt = s.kind
    if vt == "object" and any(kesc for _, kesc, *_ in s.members):
        return DEFER, 0  # (the args' rule 8 rides along: the walk is the args')
    if vt == "string":
        text, esc, at = span[1:-1], b"\\" in span, base + 1
    else:
        text, esc, at = span, False, base
    if not ac.takes(t, vt, text):
        return MISMATCH, 0
    v = ac.convert(t, vt, bytes(text), esc, at)
    return (DEFER, 0) if v is None else (OK, v)


def error_of(span, base):
    """The `error` member: (status, code, message)."""
    if len(span) == 0:
        return ABSENT, 0, 0
    st, slots = ac.args_span(span, base, ERROR_PARAMS)
    if st == ac.OK:
        code = slots[0] & 0xFFFFFFFF
        return OK, code - (1 << 32) if code >> 31 else code, slots[1]
    return (MISMATCH if st == ac.INVALID else DEFER), 0, 0


def results_entries(buf, entries, pending_method, types=TYPES):
    """Rules 1-7 and the error's over entries (body_off, body_len, kind, slot, result_off,
    result_len, error_off, error_len): one Row per entry."""
    out = []
    for boff, blen, kind, slot, roff, rlen, eoff, elen in entries:
        if kind != rv.MATCHED:
            out.append(plain(NONE))
        elif slot >= len(pending_method) or pending_method[slot] >= len(types) or types[pending_method[slot]] > STR:
            out.append(plain(BAD_SCHEMA))
        elif not (boff <= len(buf) and blen <= len(buf) - boff) or \
                (rlen and not (roff <= blen and rlen <= blen - roff)) or \
                (elen and not (eoff <= blen and elen <= blen - eoff)):
            out.append(plain(RANGE))
        elif blen > rc.MAX_BODY:
            out.append(Row(DEFER if rlen else ABSENT, 0, DEFER if elen else ABSENT, 0, 0))
        else:
            body = buf[boff:boff + blen]
            st, v = value_of(body[roff:roff + rlen], roff, types[pending_method[slot]])
            out.append(Row(st, v, *error_of(body[eoff:eoff + elen], eoff)))
    return out


def results_slots(entries, rows, slot_entry):
    """The per-slot part: (status, value, error_status, error_code, str_base) per slot."""
    out = []
    for s, e in enumerate(slot_entry):
        if e < len(entries) and entries[e][2] == rv.MATCHED and entries[e][3] == s:
            out.append((rows[e].status, rows[e].value, rows[e].error_status, rows[e].error_code, entries[e][0]))
        else:
            out.append((0, 0, 0, 0, 0))
    return out


def ndefer(rows):
    return sum(1 for r in rows if DEFER in (r.status, r.error_status))


# ---- replies and their entries -------------------------------------------------------------
def reply(rid, result=None, error=None, error_first=False):
    """A reply body with the given member spans (None: absent): (body, result_off, result_len,
    error_off, error_len), the spans 0 / 0 when absent."""
    body = b'{"jsonrpc":"2.0","id":%d' % rid
    at = {}
    members = [(b"result", result), (b"error", error)]
    for name, span in reversed(members) if error_first else members:
        if span is not None:
            body += b',"' + name + b'":'
            at[name] = (len(body), len(span))
            body += span
    body += b"}"
    return (body, *at.get(b"result", (0, 0)), *at.get(b"error", (0, 0)))


def back_to_back(replies, pad_front=0, nul=1):
    """(type, result span, error span) replies as the unpack leaves their bodies, entry k MATCHED
    to slot k: (buf, entries, pending_method, slot_entry)."""
    buf, entries = bytearray(b"#" * pad_front), []
    for k, (t, result, error) in enumerate(replies):
        body, *spans = reply(k, result, error, error_first=k % 3 == 1)
        entries.append((len(buf), len(body), rv.MATCHED, k, *spans))
        buf += body + b"\0" * nul
    return bytes(buf), entries, [t for t, _, _ in replies], list(range(len(replies)))


def f64(x):
    return ac.bits_of(float(x))


def i(x):
    return x & M64


def err(code, message=b'"m"'):
    return b'{"code":%s,"message":%s}' % (code, message)


_tok256 = b"[" + b"1," * 126 + b"[]]"
_tok257 = b"[" + b",".join([b"1"] * 128) + b"]"

#: (name, type, result span or None, error span or None, status, value or None (a STR slot,
#: checked against the bytes), error status, error code) -- written down by hand from the rules
CASES = [
    # rule 4 and the error alone
    ("no member at all", I32, None, None, ABSENT, 0, ABSENT, 0),
    ("error alone", F64, None, err(b"-32601", b'"Method not found"'), ABSENT, 0, OK, -32601),
    ("both members", I32, b"7", err(b"5"), OK, 7, OK, 5),
    ("both, the value mismatched", STR, b"null", err(b"-32603"), MISMATCH, 0, OK, -32603),
    # rule 5
    ("leading blank", I32, b" 1", None, DEFER, 0, ABSENT, 0),
    ("trailing blank", I32, b"1 ", None, DEFER, 0, ABSENT, 0),
    ("leading zero", I32, b"01", None, DEFER, 0, ABSENT, 0),
    ("bad literal", BOOL, b"tru", None, DEFER, 0, ABSENT, 0),
    ("not strict wins over a mismatch", STR, b"[01]", None, DEFER, 0, ABSENT, 0),
    ("control byte", STR, b'"a\x01"', None, DEFER, 0, ABSENT, 0),
    ("u escape", STR, b'"\\u0041"', None, DEFER, 0, ABSENT, 0),
    ("ends in a string", STR, b'"abc', None, DEFER, 0, ABSENT, 0),
    ("depth 31", I32, b"[" * 31 + b"]" * 31, None, MISMATCH, 0, ABSENT, 0),
    ("depth 32", I32, b"[" * 32 + b"]" * 32, None, DEFER, 0, ABSENT, 0),
    ("tokens 256", F64, _tok256, None, MISMATCH, 0, ABSENT, 0),
    ("tokens 257", F64, _tok257, None, DEFER, 0, ABSENT, 0),
    # rule 6: every row of the matrix
    ("number for i32", I32, b"12", None, OK, 12, ABSENT, 0),
    ("number for i64", I64, b"12", None, OK, 12, ABSENT, 0),
    ("number for f64", F64, b"12", None, OK, f64(12), ABSENT, 0),
    ("number for bool", BOOL, b"1", None, MISMATCH, 0, ABSENT, 0),
    ("number for str", STR, b"5", None, MISMATCH, 0, ABSENT, 0),
    ("string for i32", I32, b'"1"', None, MISMATCH, 0, ABSENT, 0),
    ("string for i64", I64, b'"-5"', None, OK, i(-5), ABSENT, 0),
    ("string for f64", F64, b'"1.5"', None, MISMATCH, 0, ABSENT, 0),
    ("string for bool", BOOL, b'"true"', None, MISMATCH, 0, ABSENT, 0),
    ("string for str", STR, b'"hello"', None, OK, None, ABSENT, 0),
    ("true for bool", BOOL, b"true", None, OK, 1, ABSENT, 0),
    ("false for bool", BOOL, b"false", None, OK, 0, ABSENT, 0),
    ("true for i32", I32, b"true", None, MISMATCH, 0, ABSENT, 0),
    ("false for i64", I64, b"false", None, MISMATCH, 0, ABSENT, 0),
    ("true for f64", F64, b"true", None, MISMATCH, 0, ABSENT, 0),
    ("true for str", STR, b"true", None, MISMATCH, 0, ABSENT, 0),
    ("null for i32", I32, b"null", None, MISMATCH, 0, ABSENT, 0),
    ("null for i64", I64, b"null", None, MISMATCH, 0, ABSENT, 0),
    ("null for f64 (the server's NaN)", F64, b"null", None, MISMATCH, 0, ABSENT, 0),
    ("null for bool", BOOL, b"null", None, MISMATCH, 0, ABSENT, 0),
    ("null for str", STR, b"null", None, MISMATCH, 0, ABSENT, 0),
    ("object for i32", I32, b'{"a":1}', None, MISMATCH, 0, ABSENT, 0),
    ("object for str", STR, b"{}", None, MISMATCH, 0, ABSENT, 0),
    ("array for f64", F64, b"[1.5]", None, MISMATCH, 0, ABSENT, 0),
    ("array for bool", BOOL, b"[true]", None, MISMATCH, 0, ABSENT, 0),
    ("array for i64", I64, b'["1"]', None, MISMATCH, 0, ABSENT, 0),
    ("mismatch wins over defer", BOOL, b"1e400", None, MISMATCH, 0, ABSENT, 0),
    # rule 7: I32
    ("i32 truncates", I32, b"1.9", None, OK, 1, ABSENT, 0),
    ("i32 truncates up", I32, b"-1.9", None, OK, i(-1), ABSENT, 0),
    ("i32 max", I32, b"2147483647", None, OK, 2147483647, ABSENT, 0),
    ("i32 min", I32, b"-2147483648", None, OK, i(-2147483648), ABSENT, 0),
    ("i32 above", I32, b"2147483648", None, DEFER, 0, ABSENT, 0),
    ("i32 below", I32, b"-2147483649", None, DEFER, 0, ABSENT, 0),
    ("i32 exponent", I32, b"1e3", None, OK, 1000, ABSENT, 0),
    ("i32 20 digits", I32, b"12345678901234567890e-15", None, DEFER, 0, ABSENT, 0),
    ("object with an escaped key", I32, b'{"a\\/b":1}', None, DEFER, 0, ABSENT, 0),
    ("object with an escaped key below", I32, b'{"a":{"a\\/b":1}}', None, MISMATCH, 0, ABSENT, 0),
    # I64
    ("i64 string min", I64, b'"-9223372036854775808"', None, OK, i(-2**63), ABSENT, 0),
    ("i64 string max", I64, b'"9223372036854775807"', None, OK, 2**63 - 1, ABSENT, 0),
    ("i64 string over", I64, b'"9223372036854775808"', None, DEFER, 0, ABSENT, 0),
    ("i64 string blank", I64, b'" 12"', None, DEFER, 0, ABSENT, 0),
    ("i64 string empty", I64, b'""', None, DEFER, 0, ABSENT, 0),
    ("i64 string escape", I64, b'"1\\/2"', None, DEFER, 0, ABSENT, 0),
    ("i64 number through the double", I64, b"9007199254740993", None, OK, 9007199254740992, ABSENT, 0),
    ("i64 number 2^63", I64, b"9223372036854775808", None, DEFER, 0, ABSENT, 0),
    ("i64 number -2^63", I64, b"-9223372036854775808", None, OK, i(-2**63), ABSENT, 0),
    # F64
    ("f64", F64, b"-1.25", None, OK, f64(-1.25), ABSENT, 0),
    ("f64 -0.0", F64, b"-0.0", None, OK, 1 << 63, ABSENT, 0),
    ("f64 19 digits", F64, b"1234567890123456789", None, OK, f64(1234567890123456789), ABSENT, 0),
    ("f64 20 digits", F64, b"12345678901234567890", None, DEFER, 0, ABSENT, 0),
    ("f64 largest", F64, b"1.7976931348623157e308", None, OK, 0x7FEFFFFFFFFFFFFF, ABSENT, 0),
    ("f64 overflows", F64, b"1.7976931348623159e308", None, DEFER, 0, ABSENT, 0),
    ("f64 subnormal", F64, b"4.9e-324", None, DEFER, 0, ABSENT, 0),
    ("f64 through cJSON's 17 digits", F64, b"0.10000000000000001", None, OK, f64(0.1), ABSENT, 0),
    # STR
    ("empty string", STR, b'""', None, OK, None, ABSENT, 0),
    ("string with high bytes", STR, b'"\xc3\xa9\xff\x80"', None, OK, None, ABSENT, 0),
    ("string with a backslash", STR, b'"a\\nb"', None, DEFER, 0, ABSENT, 0),
    ("string with JSON inside", STR, b'"{[1,true]}"', None, OK, None, ABSENT, 0),
    # the error member
    ("error not an object", I32, None, b'"boom"', ABSENT, 0, MISMATCH, 0),
    ("error null", I32, b"1", b"null", OK, 1, MISMATCH, 0),
    ("error without code", I32, None, b'{"message":"m"}', ABSENT, 0, MISMATCH, 0),
    ("error without message", I32, None, b'{"code":1}', ABSENT, 0, MISMATCH, 0),
    ("error with Code", I32, None, b'{"Code":1,"message":"m"}', ABSENT, 0, MISMATCH, 0),
    ("error code a string", I32, None, b'{"code":"1","message":"m"}', ABSENT, 0, MISMATCH, 0),
    ("error message a number", I32, None, b'{"code":1,"message":2}', ABSENT, 0, MISMATCH, 0),
    ("error, members swapped and extras", I32, None, b'{"data":[1],"message":"m","code":-7}', ABSENT, 0, OK, -7),
    ("error code truncates", I32, None, err(b"-32600.9"), ABSENT, 0, OK, -32600),
    ("error code out of i32", I32, None, err(b"2147483648"), ABSENT, 0, DEFER, 0),
    ("error message escaped", I32, None, err(b"1", b'"a\\"b"'), ABSENT, 0, DEFER, 0),
    ("error not strict", I32, None, b'{"code":1,"message":"m",}', ABSENT, 0, DEFER, 0),
    ("error key escaped", I32, None, b'{"code":1,"message":"m","a\\/b":1}', ABSENT, 0, DEFER, 0),
    ("value defers, error decodes", F64, b"1e400", err(b"3"), DEFER, 0, OK, 3),
    ("value decodes, error defers", F64, b"2.5", b"{,}", OK, f64(2.5), DEFER, 0),
    ("both defer: counted once", STR, b'"\\n"', b"[", DEFER, 0, DEFER, 0),
]


def bare_entries(buf, spans, first_slot):
    """Each span as a body of its own with the span as its `result` (what no resolve produces,
    but what alone puts 1,024 bytes of value into a body that is staged): the limits of rule 5."""
    buf, entries = bytearray(buf), []
    for k, span in enumerate(spans):
        entries.append((len(buf), len(span), rv.MATCHED, first_slot + k, 0, len(span), 0, 0))
        buf += span + b"\0"
    return bytes(buf), entries


#: (type, span, status): rule 5's length limit on the span and on the body
BARE = [
    (STR, b'"' + b"x" * 1022 + b'"', OK),
    (STR, b'"' + b"x" * 1023 + b'"', DEFER),
    (F64, b"[" + b"1," * 510 + b"12]", DEFER),  # 1,024 bytes but 1,023 tokens
    (I32, b"7", OK),
]


def case_entries(pad_front=3):
    """The table as one buffer with the entries of the other statuses behind it: (buf, entries,
    pending_method, slot_entry).  Entry k of the table is MATCHED to slot k."""
    buf, entries, pm, se = back_to_back([(t, r, e) for _, t, r, e, *_ in CASES], pad_front=pad_front)
    nb = len(entries)
    buf, bare = bare_entries(buf, [s for _, s, _ in BARE], nb)
    entries += bare
    pm += [t for t, _, _ in BARE]
    se += list(range(nb, nb + len(BARE)))
    buf = bytearray(buf)
    body, ro, rl, eo, el = reply(9, b"41", err(b"2"))
    at = len(buf)
    buf += body  # (the buffer ends with this body's last byte)
    s0 = len(pm)
    pm += [I32, 5, 255, 7, 0xFFFF, I32]  # slots s0 .. s0 + 5
    ok = (at, len(body), rv.MATCHED, s0, ro, rl, eo, el)
    first = len(entries)
    entries += [(at, len(body), k, s0, ro, rl, eo, el) for k in (rv.NONE, rv.UNKNOWN, rv.DUPLICATE, rv.INVALID, rv.DEFER,
                                                                 rv.RANGE, 7, 255)]
    entries += [
        (1 << 62, 5, rv.UNKNOWN, 0xFFFFFFFF, 1 << 31, 1 << 31, 1 << 31, 1 << 31),  # rule 1: nothing else is looked at
        ok,                                                          # the last body of the buffer, decoded
        ok[:3] + (s0 + 1,) + ok[4:],                                 # rule 2: type 5
        ok[:3] + (s0 + 2,) + ok[4:],                                 # type 255
        ok[:3] + (s0 + 3,) + ok[4:],                                 # method 7 of 7
        ok[:3] + (s0 + 4,) + ok[4:],                                 # method 0xFFFF
        ok[:3] + (s0 + 6,) + ok[4:],                                 # slot == npending
        ok[:3] + (0xFFFFFFFF,) + ok[4:],                             # NO_SLOT
        (1 << 62, 5, rv.MATCHED, s0 + 1, 0, 0, 0, 0),                # rule 2 comes before rule 3
        (at + 1, len(body), rv.MATCHED, s0 + 5, ro, rl, eo, el),     # rule 3: the body leaves the buffer by a byte
        (len(buf) + 1, 0, rv.MATCHED, s0 + 5, 0, 0, 0, 0),           # starts behind the end
        (2**64 - 2, 8, rv.MATCHED, s0 + 5, 0, 4, 0, 0),              # would wrap
        (at, len(body), rv.MATCHED, s0 + 5, ro, len(body) - ro + 1, eo, el),  # `result` leaves the body by a byte
        (at, len(body), rv.MATCHED, s0 + 5, 0xFFFFFFFF, 2, eo, el),  # would wrap in 32 bits
        (at, len(body), rv.MATCHED, s0 + 5, ro, rl, len(body), 1),   # `error` starts behind the body
        (at, len(body), rv.MATCHED, s0 + 5, ro, rl, eo, len(body) - eo + 1),
        (at, len(body), rv.MATCHED, s0 + 5, 0xFFFFFFFF, 0, 0xFFFFFFF0, 0),  # empty spans are not checked: ABSENT twice
        (at, len(body), rv.MATCHED, s0 + 5, len(body) - 1, 1, eo, el),      # "}" alone on the buffer's last byte
        (at, len(body), rv.MATCHED, s0 + 5, ro, rl, 0, 0),
    ]
    se += [first + 9, first + 10, first + 11, first + 12, first + 13, len(entries) - 1]
    return bytes(buf), entries, pm, se


# ---- the per-slot cases ----------------------------------------------------------------------
def slot_cases():
    """(buf, entries, pending_method, slot_entry): open slots, a slot_entry word on an entry that
    is not MATCHED, on one that names another slot, past n, and two MATCHED entries naming one
    slot (what no resolve produces)."""
    bodies = [reply(k, b"%d" % (100 + k), err(b"%d" % k) if k % 2 else None) for k in range(6)]
    buf, entries = bytearray(), []
    kinds = [rv.MATCHED, rv.DUPLICATE, rv.MATCHED, rv.MATCHED, rv.MATCHED, rv.UNKNOWN]
    slots = [0, 0, 2, 3, 3, rv.NO_SLOT]  # entries 3 and 4 both name slot 3
    for (body, *spans), kind, slot in zip(bodies, kinds, slots):
        entries.append((len(buf), len(body), kind, slot, *spans))
        buf += body + b"\0"
    pm = [I32] * 8
    #            0  1: on a DUPLICATE  2  3: the later of the two  4: on slot 3's entry  5: open  6: past n  7: == n
    se = [0, 1, 2, 4, 3, rv.NO_SLOT, 1000, 6]
    return bytes(buf), entries, pm, se


# ---- bodies placed anywhere (tests/stage_cases.py) ---------------------------------------------
def placed_entries(buf, spans):
    """Reply bodies at ``spans`` of ``buf`` as entries that all reach the staging rounds when
    stage_cases.walked says so: entry k is MATCHED to slot k of type k % 5, its member spans are
    the resolve's rules' where the body decodes to any, and the whole body as `result` where it
    does not (so that a body the resolve would defer is walked all the same).  Returns (entries,
    pending_method, slot_entry)."""
    entries = []
    for k, (off, ln) in enumerate(spans):
        members = (0, ln, 0, 0)
        if off <= len(buf) and ln <= len(buf) - off:
            row = rv.decode_body(buf[off:off + ln])
            if row[0] == rv.UNKNOWN and (row[3] or row[5]):
                members = row[2:]
        entries.append((off, ln, rv.MATCHED, k, *members))
    return entries, [k % 5 for k in range(len(spans))], list(range(len(spans)))


# ---- canonical and mutated replies -----------------------------------------------------------
def canonical_result(rng, t):
    """A `result` of type t as the reference server prints it (rpc_server_skeleton.c): numbers
    through cJSON's print_number, an i64 as a decimal string, strings with nothing to escape."""
    if t == I32:
        return b"%d" % rng.choice([rng.randrange(-2**31, 2**31), rng.randrange(-100, 100), -2**31, 2**31 - 1])
    if t == I64:
        return b'"%d"' % rng.choice([rng.randrange(-2**63, 2**63), rng.randrange(-1000, 1000), -2**63, 2**63 - 1])
    if t == F64:
        return ac.print_number(ac.rand_double(rng))
    if t == BOOL:
        return rng.choice([b"true", b"false"])
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789 _-/é中{}[]:,"
    return b'"%s"' % "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 60))).encode()


def canonical_set(seed, count):
    """(type, result span, error span): five in six a result, one in six an error."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        t = k % 5
        if rng.randrange(6) == 0:
            code, msg = rng.choice([(-32700, "Parse error"), (-32600, "Invalid Request"), (-32601, "Method not found"),
                                    (-32602, "Invalid params"), (-32603, "Internal error")])
            out.append((t, None, err(b"%d" % code, b'"%s"' % msg.encode())))
        else:
            out.append((t, canonical_result(rng, t), None))
    return out


def mutation_set(seed, count):
    """Canonical members with one byte flipped, inserted or deleted, or truncated."""
    rng = random.Random(seed)
    base = canonical_set(seed ^ 0x5EED, 120)
    pool = b'{}[],:"\\ \t\n\r0123456789-+.eEtfnu/acdegmos\x00\x01\x1f\x7f\x80\xff'
    out = []
    for _ in range(count):
        t, r, e = rng.choice(base)
        b = bytearray(r if e is None else e)
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
        if not b:
            b = bytearray(b"0")
        out.append((t, bytes(b), None) if e is None else (t, None, bytes(b)))
    return out
