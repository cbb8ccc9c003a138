"""The frame values' rules (include/rpccrc.h, rpc_frames_values_device) in plain Python, and the
cases the emulator and the GPU are held against.

A double's text is literally ``"%.15g" % d``, ``float()`` of it and ``"%.17g" % d``: the pin of
cJSON's print_number.  Nothing here shares code with rpc_amd/csrc/frames_values.h."""
import math
import struct
from typing import NamedTuple

import args_cases as ac

NONE, OK, TEXT, DEFER, RANGE, BAD_SCHEMA, NO_ROOM = range(7)
MODE_NONE, MODE_ENCODE, MODE_TEXT = range(3)
FORM_RESULT, FORM_PARAMS = 0, 1
I32, I64, F64, BOOL, STR = ac.I32, ac.I64, ac.F64, ac.BOOL, ac.STR
INTERNAL = -32603
M64 = (1 << 64) - 1
EPS = 2.0 ** -52

#: the result type of each of the IDL's seven methods (rpc_server_skeleton.c:162-257), in the
#: order of args_cases.IDL_METHODS: ping and mix3 return strings
IDL_RESULTS = [STR, I64, I32, F64, BOOL, I32, STR]


def bits_of(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits & M64))[0]


def f64_text(bits):
    """print_number of the double with these bits, or None: a subnormal (DEFER)."""
    d = double_of(bits)
    if math.isnan(d) or math.isinf(d):
        return b"null"
    if d == math.floor(d) and -2147483648 <= d <= 2147483647:
        return b"%d" % int(d)
    if abs(d) < 2.0 ** -1022:
        return None
    t15 = "%.15g" % d
    r = float(t15)
    if abs(r - d) <= max(abs(r), abs(d)) * EPS:
        return t15.encode()
    return ("%.17g" % d).encode()


ESCAPED = bytes(range(0x20)) + b'"\\'


def needs_escape(b):
    return len(bytes(b).translate(None, ESCAPED)) != len(b)


class Entry(NamedTuple):
    mode: int
    status: int
    method: int
    slots: tuple       # up to width words
    str_base: int = 0
    text_off: int = 0
    text_len: int = 0


def value_text(t, slot, base, strings):
    """One slot's text: (status, bytes)."""
    slot &= M64
    if t == I32:
        v = slot & 0xFFFFFFFF
        return OK, b"%d" % (v - (1 << 32) if v >> 31 else v)
    if t == I64:
        return OK, b'"%d"' % (slot - (1 << 64) if slot >> 63 else slot)
    if t == BOOL:
        return OK, b"true" if slot else b"false"
    if t == F64:
        x = f64_text(slot)
        return (DEFER, b"") if x is None else (OK, x)
    at, ln = base + (slot & 0xFFFFFFFF), slot >> 32
    s = strings[at:at + ln]
    return (DEFER, b"") if needs_escape(s) else (OK, b'"' + s + b'"')


def str_in_range(slot, base, nstrings):
    at, ln = base + (slot & 0xFFFFFFFF), (slot & M64) >> 32
    return at <= M64 and at <= nstrings and ln <= nstrings - at


def values_entry(e, form, schema, result_types, width, strings, texts, have_texts=True):
    """(status, text) of one entry before the capacity check; ``schema``: args_cases.Schema."""
    if e.status != 0 or e.mode not in (MODE_ENCODE, MODE_TEXT):
        return NONE, b""
    if e.mode == MODE_TEXT:
        if not have_texts or not (e.text_off <= len(texts) and e.text_len <= len(texts) - e.text_off):
            return RANGE, b""
        return TEXT, texts[e.text_off:e.text_off + e.text_len]
    nmethods = len(result_types) if form == FORM_RESULT else schema.nmethods
    if e.method >= nmethods:
        return BAD_SCHEMA, b""
    if form == FORM_RESULT:
        if result_types[e.method] > STR:
            return BAD_SCHEMA, b""
        params = [(None, result_types[e.method])]
    else:
        a, b = schema.first[e.method], schema.first[e.method + 1]
        if a > b or b > len(schema.types) or b - a > width:
            return BAD_SCHEMA, b""
        params = []
        for p in range(a, b):
            x, y = schema.noff[p], schema.noff[p + 1]
            if x > y or y > len(schema.names) or schema.types[p] > STR:
                return BAD_SCHEMA, b""
            if needs_escape(schema.names[x:y]):
                return BAD_SCHEMA, b""
            params.append((schema.names[x:y], schema.types[p]))
    for k, (_, t) in enumerate(params):
        if t == STR and not str_in_range(e.slots[k], e.str_base, len(strings)):
            return RANGE, b""
    # the entry's size from the slots alone, before any string byte is read: a value that has no
    # text counts no bytes, nor does what stands around it
    size, defer = (0 if params else 2), False  # ({} for a method without parameters)
    for k, (name, t) in enumerate(params):
        if t == STR:
            n = 2 + ((e.slots[k] & M64) >> 32)
        else:
            st, txt = value_text(t, e.slots[k], e.str_base, strings)
            if st != OK:
                defer = True
                continue
            n = len(txt)
        if form == FORM_PARAMS:  # `{` or `,` in front, "name": and `}` behind the last
            n += 1 + len(name) + 3 + (k + 1 == len(params))
        size += n
    if size > 0xFFFFFFFF:
        return RANGE, b""
    if defer:
        return DEFER, b""
    parts = []
    for k, (name, t) in enumerate(params):
        st, txt = value_text(t, e.slots[k], e.str_base, strings)
        if st != OK:
            return st, b""
        parts.append(txt if name is None else b'"' + name + b'":' + txt)
    out = parts[0] if form == FORM_RESULT else b"{" + b",".join(parts) + b"}"
    assert len(out) == size, (len(out), size)
    return OK, out


def values_batch(entries, form, schema, result_types, width, strings, texts, out_cap=None, have_texts=True):
    """Per entry (status, reply_status, offset, length) and the output bytes (None where not
    written), the total and the DEFER count."""
    rows, at, ndefer = [], 0, 0
    chunks = []
    for e in entries:
        st, txt = values_entry(e, form, schema, result_types, width, strings, texts, have_texts)
        if txt and out_cap is not None and at + len(txt) > out_cap:
            st = NO_ROOM
        ndefer += st == DEFER
        rs = e.status if st in (NONE, OK, TEXT) else INTERNAL
        rows.append((st, rs, at, len(txt)))
        chunks.append((at, txt if st in (OK, TEXT) else None, len(txt)))
        at += len(txt)
    return rows, chunks, at, ndefer


# ---- the case table ------------------------------------------------------------------------
STRINGS = b'hello\x00wor"ld back\\slash caf\xc3\xa9 \x1f ' + bytes(range(0x20, 0x22)) + b"0123456789abcdef" * 3 + b"Z"
TEXTS = b'{"a":[1,2]}null"q"  \t'


def s_slot(needle, extra=0):
    """The STR slot of ``needle`` inside STRINGS."""
    at = STRINGS.index(needle)
    return at | (len(needle) + extra) << 32


def d(x):
    return bits_of(x)


#: (name, type, slot, status, text) for the RESULT form: every rule, every example of the header
RESULT_CASES = [
    ("i32 zero", I32, 0, OK, b"0"),
    ("i32 max", I32, 2147483647, OK, b"2147483647"),
    ("i32 min", I32, 0x80000000, OK, b"-2147483648"),
    ("i32 reads the low word", I32, 0xDEADBEEF00000007, OK, b"7"),
    ("i32 -1", I32, M64, OK, b"-1"),
    ("i64 zero", I64, 0, OK, b'"0"'),
    ("i64 max", I64, (1 << 63) - 1, OK, b'"9223372036854775807"'),
    ("i64 min", I64, 1 << 63, OK, b'"-9223372036854775808"'),
    ("i64 -1", I64, M64, OK, b'"-1"'),
    ("i64 beyond a double", I64, 9007199254740993, OK, b'"9007199254740993"'),
    ("bool 0", BOOL, 0, OK, b"false"),
    ("bool 1", BOOL, 1, OK, b"true"),
    ("bool any", BOOL, 1 << 63, OK, b"true"),
    ("str plain", STR, s_slot(b"hello"), OK, b'"hello"'),
    ("str empty", STR, 3, OK, b'""'),
    ("str utf-8", STR, s_slot(b"caf\xc3\xa9"), OK, b'"caf\xc3\xa9"'),
    ("str long", STR, s_slot(b"0123456789abcdef" * 3), OK, b'"' + b"0123456789abcdef" * 3 + b'"'),
    ("str last byte", STR, s_slot(b"Z"), OK, b'"Z"'),
    ("str nul", STR, s_slot(b"hello", 1), DEFER, b""),
    ("str quote", STR, s_slot(b'wor"ld'), DEFER, b""),
    ("str backslash", STR, s_slot(b"back\\slash"), DEFER, b""),
    ("str control", STR, s_slot(b"\x1f"), DEFER, b""),
    ("str 0x20 is plain", STR, s_slot(b"\x20"), OK, b'" "'),
    ("str past the end", STR, s_slot(b"Z", 1), RANGE, b""),
    ("str offset past the end", STR, len(STRINGS) + 1, RANGE, b""),
    ("str huge length", STR, 0xFFFFFFFF << 32, RANGE, b""),
    ("str empty at the end", STR, len(STRINGS), OK, b'""'),
    ("f64 nan", F64, 0x7FF8000000000000, OK, b"null"),
    ("f64 inf", F64, d(math.inf), OK, b"null"),
    ("f64 -inf", F64, d(-math.inf), OK, b"null"),
    ("f64 +0", F64, 0, OK, b"0"),
    ("f64 -0", F64, 1 << 63, OK, b"0"),
    ("f64 int", F64, d(1000.0), OK, b"1000"),
    ("f64 int max", F64, d(2147483647.0), OK, b"2147483647"),
    ("f64 int min", F64, d(-2147483648.0), OK, b"-2147483648"),
    ("f64 saturated valueint", F64, d(2147483648.0), OK, b"2147483648"),
    ("f64 below int min", F64, d(-2147483649.0), OK, b"-2147483649"),
    ("f64 half", F64, d(0.5), OK, b"0.5"),
    ("f64 2.5", F64, d(2.5), OK, b"2.5"),
    ("f64 0.1", F64, d(0.1), OK, b"0.1"),
    ("f64 0.1+0.2 keeps 15 digits", F64, d(0.1 + 0.2), OK, b"0.3"),
    ("f64 third takes 17", F64, d(1.0 / 3.0), OK, b"0.33333333333333331"),
    ("f64 1e-5 scientific", F64, d(1e-5), OK, b"1e-05"),
    ("f64 1e-4 fixed", F64, d(1e-4), OK, b"0.0001"),
    ("f64 1e15 scientific", F64, d(1e15), OK, b"1e+15"),
    ("f64 1e14 fixed", F64, d(123456789012345.0), OK, b"123456789012345"),
    ("f64 1e22", F64, d(1e22), OK, b"1e+22"),
    ("f64 carry to 1e+23", F64, d(9.999999999999999e22), OK, b"1e+23"),
    ("f64 tie at 15, even: 17 digits", F64, d(100000000000000.5), OK, b"100000000000000.5"),
    ("f64 tie at 15, odd: 17 digits", F64, d(100000000000001.5), OK, b"100000000000001.5"),
    ("f64 tie at 17", F64, d(1000000000000000.25), OK, b"1000000000000000.2"),
    ("f64 tie at 15 above 1e15: 17 digits", F64, d(1000000000000005.0), OK, b"1000000000000005"),
    ("f64 max", F64, d(1.7976931348623157e308), OK, b"1.79769313486232e+308"),
    ("f64 min normal", F64, d(2.2250738585072014e-308), OK, b"2.2250738585072014e-308"),
    ("f64 subnormal", F64, 1, DEFER, b""),
    ("f64 largest subnormal", F64, (1 << 52) - 1, DEFER, b""),
    ("f64 -pi", F64, d(-math.pi), OK, b"-3.1415926535897931"),
    ("f64 three exponent digits", F64, d(1.5e-300), OK, b"1.5e-300"),
    ("f64 2^53+2", F64, d(9007199254740994.0), OK, b"9007199254740994"),
    ("f64 1 ulp off keeps 15 digits", F64, d(0.30000000000000004), OK, b"0.3"),
]
for _n, _t, _s, _st, _txt in RESULT_CASES:
    if _t == F64:
        assert (_st, _txt) == ((DEFER, b"") if f64_text(_s) is None else (OK, f64_text(_s))), (_n, f64_text(_s))

#: schemas beside the IDL's: 0 and 8 parameters, a repeated name, the empty name, a name that needs
#: an escape, and each broken schema word
EXTRA_METHODS = [
    (b"none", []),
    (b"eight", [(b"p%d" % k, (I32, I64, F64, BOOL, STR)[k % 5]) for k in range(8)]),
    (b"twice", [(b"a", I32), (b"a", F64)]),
    (b"noname", [(b"", I32), (b"x", BOOL)]),
    (b"quote", [(b'a"b', I32)]),
    (b"ctl", [(b"a\x01", I32)]),
    (b"bslash", [(b"a\\", I32)]),
    (b"strs", [(b"first", STR), (b"second", STR), (b"n", I32)]),
]
EXTRA = ac.schema_of(EXTRA_METHODS)


def broken_schemas():
    """(what, schema, method) triples, each BAD_SCHEMA for that method."""
    s = ac.schema_of([(b"m", [(b"a", I32), (b"b", I32)])])
    return [
        ("first words not monotone", ac.Schema([2, 0], s.types, s.noff, s.names), 0),
        ("first word leaves nparams", ac.Schema([0, 3], s.types, s.noff, s.names), 0),
        ("unknown type", ac.Schema(s.first, [I32, 5], s.noff, s.names), 0),
        ("name words not monotone", ac.Schema(s.first, s.types, [0, 2, 1], s.names), 0),
        ("name word leaves the names", ac.Schema(s.first, s.types, [0, 1, 9], s.names), 0),
    ]


def params_cases():
    """(what, schema, width, Entry) for the PARAMS form."""
    e = MODE_ENCODE
    eight = (7, M64, d(2.5), 0, s_slot(b"hello"), 0x80000000, 12, d(1e-7))
    return [
        ("ping", ac.IDL, 8, Entry(e, 0, 0, (0,) * 8)),
        ("echo_i64", ac.IDL, 8, Entry(e, 0, 1, (1 << 63,) + (0,) * 7)),
        ("add_i32", ac.IDL, 8, Entry(e, 0, 2, (1, M64) + (0,) * 6)),
        ("mul_double", ac.IDL, 8, Entry(e, 0, 3, (d(1.0), d(2.5)) + (0,) * 6)),
        ("strlen_s", ac.IDL, 8, Entry(e, 0, 5, (s_slot(b"hello"),) + (0,) * 7)),
        ("strlen_s escape", ac.IDL, 8, Entry(e, 0, 5, (s_slot(b'wor"ld'),) + (0,) * 7)),
        ("mix3", ac.IDL, 8, Entry(e, 0, 6, (5, d(0.1), 1) + (0,) * 5)),
        ("mix3 width 3", ac.IDL, 3, Entry(e, 0, 6, (5, d(0.1), 1))),
        ("mix3 too narrow", ac.IDL, 2, Entry(e, 0, 6, (5, d(0.1)))),
        ("method past the table", ac.IDL, 8, Entry(e, 0, 7, (0,) * 8)),
        ("none", EXTRA, 8, Entry(e, 0, 0, (0,) * 8)),
        ("eight", EXTRA, 8, Entry(e, 0, 1, eight)),
        ("twice", EXTRA, 8, Entry(e, 0, 2, (3, d(3.0)) + (0,) * 6)),
        ("noname", EXTRA, 8, Entry(e, 0, 3, (3, 1) + (0,) * 6)),
        ("quote in a name", EXTRA, 8, Entry(e, 0, 4, (3,) + (0,) * 7)),
        ("control byte in a name", EXTRA, 8, Entry(e, 0, 5, (3,) + (0,) * 7)),
        ("backslash in a name", EXTRA, 8, Entry(e, 0, 6, (3,) + (0,) * 7)),
        ("two strings", EXTRA, 8, Entry(e, 0, 7, (s_slot(b"hello"), s_slot(b"0123456789abcdef" * 3), 9) + (0,) * 5)),
        ("precedence: range over defer", EXTRA, 8,
         Entry(e, 0, 7, (s_slot(b'wor"ld'), s_slot(b"Z", 1), 9) + (0,) * 5)),
        ("precedence: bad schema over range", EXTRA, 8, Entry(e, 0, 4, (len(STRINGS) + 9,) + (0,) * 7)),
        ("precedence: defer", EXTRA, 8, Entry(e, 0, 7, (s_slot(b"hello"), s_slot(b"\x1f"), 9) + (0,) * 5)),
        ("status set", ac.IDL, 8, Entry(e, -32602, 2, (1, 2) + (0,) * 6)),
        ("mode none", ac.IDL, 8, Entry(MODE_NONE, 0, 2, (1, 2) + (0,) * 6)),
        ("mode unknown", ac.IDL, 8, Entry(7, 0, 2, (1, 2) + (0,) * 6)),
        ("text", ac.IDL, 8, Entry(MODE_TEXT, 0, 99, (0,) * 8, 0, 0, 11)),
        ("text empty", ac.IDL, 8, Entry(MODE_TEXT, 0, 0, (0,) * 8, 0, 4, 0)),
        ("text outside", ac.IDL, 8, Entry(MODE_TEXT, 0, 0, (0,) * 8, 0, len(TEXTS), 1)),
        ("text with a status", ac.IDL, 8, Entry(MODE_TEXT, 5, 0, (0,) * 8, 0, 0, 4)),
        ("str base", ac.IDL, 8, Entry(e, 0, 5, (0 | 5 << 32,) + (0,) * 7, STRINGS.index(b"hello"))),
        ("str base wraps", ac.IDL, 8, Entry(e, 0, 5, (8 | 1 << 32,) + (0,) * 7, M64 - 3)),
    ] + [("broken: " + w, s, 8, Entry(e, 0, m, (1, 2) + (0,) * 6)) for w, s, m in broken_schemas()]


def result_entries():
    """The RESULT table as one batch: a method per case (result_types, entries, wanted)."""
    types = [t for _, t, _, _, _ in RESULT_CASES] + [9]
    entries = [Entry(MODE_ENCODE, 0, m, (c[2],)) for m, c in enumerate(RESULT_CASES)]
    entries += [Entry(MODE_ENCODE, 0, len(RESULT_CASES), (1,)),            # unknown result type
                Entry(MODE_ENCODE, 0, len(RESULT_CASES) + 1, (1,)),        # method past the table
                Entry(MODE_ENCODE, -32603, 0, (1,)),                        # a handler's verdict
                Entry(MODE_NONE, 0, 0, (1,)),
                Entry(MODE_TEXT, 0, 0, (0,), 0, 11, 4),
                Entry(MODE_TEXT, 0, 0, (0,), 0, 15, 3),
                Entry(MODE_TEXT, 0, 0, (0,), 0, 1 << 40, 3)]
    return types, entries


def long_text_case(seed=31, tile=16384):
    """TEXT entries of a few hundred bytes and a few that cross a tile, mixed with strings of the
    same sizes and with numbers, so that one tile takes copied bytes from both sources:
    (result types, entries, strings, texts).  The texts hold any byte; they are copied verbatim."""
    import random
    rng = random.Random(seed)
    texts = bytes(rng.randrange(256) for _ in range(3 * tile + 1234))
    strings = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz 0123456789\xc3\xa9~") for _ in range(2 * tile + 777))
    types = [STR, I32, F64]
    es = []
    for i in range(260):
        r = i % 5
        if r in (0, 3):  # a text: mostly a few hundred bytes, now and then over a tile
            ln = rng.randrange(tile + 1, 2 * tile) if i % 65 == 0 else rng.choice([0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 64]) \
                if i % 7 == 0 else rng.randrange(100, 700)
            es.append(Entry(MODE_TEXT, 0, 0, (0,), 0, rng.randrange(0, len(texts) - ln + 1), ln))
        elif r in (1, 4):
            ln = rng.randrange(tile + 1, 2 * tile) if i % 66 == 0 else rng.randrange(0, 700)
            es.append(Entry(MODE_ENCODE, 0, 0, (rng.randrange(0, len(strings) - ln + 1) | ln << 32,)))
        else:
            es.append(Entry(MODE_ENCODE, 0, 1 + i % 2, (bits_of(i / 7.0) if i % 2 else i,)))
    # the first and the last bytes of the texts: a window that would leave the buffer on either side
    es += [Entry(MODE_TEXT, 0, 0, (0,), 0, 0, 200), Entry(MODE_TEXT, 0, 0, (0,), 0, len(texts) - 200, 200),
           Entry(MODE_TEXT, 0, 0, (0,), 0, 0, len(texts))]
    return types, es, strings, texts
