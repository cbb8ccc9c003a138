"""The frame route's rules (include/rpccrc.h, rpc_frames_route_device) in plain Python, and the
cases the emulator and the GPU are held against.

The strict subset is written out by hand as a recursive-descent checker: json.loads is not the
rule (it takes NaN and rejects other things).  Nothing here shares code with the automaton of
rpc_amd/csrc/frames_route.h."""
import json
import random
import re
from typing import NamedTuple

NONE, CALL, NOT_FOUND, INVALID, DEFER, RANGE = range(6)
NO_METHOD = 0xFFFF
MAX_BODY, MAX_DEPTH, MAX_TOKENS = 1024, 32, 256
MAX_METHODS, MAX_METHOD_BYTES = 256, 4096
DATA, PING, PONG, TYPE_NONE = 0, 1, 2, 0xFFFF

#: the IDL's seven methods, in the order of the reference's strcmp chain
METHODS = [b"ping", b"echo_i64", b"add_i32", b"mul_double", b"is_even", b"strlen_s", b"mix3"]


class Table(NamedTuple):
    names: bytes  # the names back to back
    offs: list    # nmethods + 1 words (a broken word is allowed: that name matches nothing)

    @property
    def nmethods(self):
        return len(self.offs) - 1 if self.offs else 0


def table_of(names):
    offs = [0]
    for n in names:
        offs.append(offs[-1] + len(n))
    return Table(b"".join(names), offs)


IDL = table_of(METHODS)


class Defer(Exception):
    pass


NUMBER = re.compile(rb"-?(?:0|[1-9][0-9]*)(?:\.[0-9]+)?(?:[eE][+-]?[0-9]+)?")
ESCAPES = b'"\\/bfnrt'


class Strict:
    """One pass over a body: raises Defer outside the strict subset (rule 3), else leaves
    ``members``: the root object's (key bytes, key has a backslash, value type, value start,
    value end, value has a backslash) in order."""

    def __init__(self, b):
        self.b, self.i, self.tokens = b, 0, 0
        self.ws()
        self.members = self.obj(1, True)
        self.ws()
        if self.i != len(b):
            raise Defer("bytes behind the root")

    def ws(self):
        while self.i < len(self.b) and self.b[self.i] in b" \t\n\r":
            self.i += 1

    def tok(self):
        self.tokens += 1
        if self.tokens > MAX_TOKENS:
            raise Defer("tokens")

    def take(self, ch):
        if self.i >= len(self.b) or self.b[self.i] != ch:
            raise Defer("expected %r at %d" % (chr(ch), self.i))
        self.tok()
        self.i += 1

    def string(self):
        """At the opening quote: returns (first byte, one past the last byte, has a backslash)."""
        self.take(0x22)
        start, esc = self.i, False
        while True:
            if self.i >= len(self.b):
                raise Defer("ends inside a string")
            c = self.b[self.i]
            if c == 0x22:
                self.i += 1
                return start, self.i - 1, esc
            if c < 0x20:
                raise Defer("control byte in a string")
            if c == 0x5C:
                esc = True
                if self.i + 1 >= len(self.b) or self.b[self.i + 1] not in ESCAPES:
                    raise Defer("escape")
                self.i += 1
            self.i += 1

    def value(self, depth):
        """Returns (type, start, end, has a backslash)."""
        if self.i >= len(self.b):
            raise Defer("ends where a value is due")
        c, start = self.b[self.i], self.i
        if c == 0x7B:
            self.obj(depth + 1, False)
            return "object", start, self.i, False
        if c == 0x5B:
            if depth + 1 > MAX_DEPTH:
                raise Defer("depth")
            self.take(0x5B)
            self.ws()
            if self.i < len(self.b) and self.b[self.i] == 0x5D:
                self.take(0x5D)
                return "array", start, self.i, False
            while True:
                self.ws()
                self.value(depth + 1)
                self.ws()
                if self.i < len(self.b) and self.b[self.i] == 0x2C:
                    self.take(0x2C)
                    continue
                self.take(0x5D)
                return "array", start, self.i, False
        if c == 0x22:
            s, e, esc = self.string()
            return "string", s, e, esc
        for lit in (b"true", b"false", b"null"):
            if self.b.startswith(lit, self.i):
                self.tok()
                self.i += len(lit)
                return "literal", start, self.i, False
        m = NUMBER.match(self.b, self.i)
        if not m:
            raise Defer("no value at %d" % self.i)
        self.tok()
        self.i = m.end()
        return "number", start, self.i, False

    def obj(self, depth, record):
        if depth > MAX_DEPTH:
            raise Defer("depth")
        self.take(0x7B)
        members = []
        self.ws()
        if self.i < len(self.b) and self.b[self.i] == 0x7D:
            self.take(0x7D)
            return members
        while True:
            self.ws()
            if self.i >= len(self.b) or self.b[self.i] != 0x22:
                raise Defer("a key is due")
            ks, ke, kesc = self.string()
            self.ws()
            self.take(0x3A)
            self.ws()
            vt, vs, ve, vesc = self.value(depth)
            if record:
                members.append((self.b[ks:ke], kesc, vt, vs, ve, vesc))
            self.ws()
            if self.i < len(self.b) and self.b[self.i] == 0x2C:
                self.take(0x2C)
                continue
            self.take(0x7D)
            return members


def route_body(body, table=IDL):
    """Rules 3-8 for one body that lies inside the buffer: (kind, method, id, params_off,
    params_len)."""
    plain = lambda kind, rid=0: (kind, NO_METHOD, rid, 0, 0)  # noqa: E731
    if len(body) == 0 or len(body) > MAX_BODY:
        return plain(DEFER)
    try:
        members = Strict(bytes(body)).members
    except Defer:
        return plain(DEFER)
    if any(kesc for _, kesc, *_ in members):  # rule 4
        return plain(DEFER)
    first = {}
    for m in members:
        first.setdefault(m[0], m)
    rid = 0
    if b"id" in first and first[b"id"][2] == "number":  # rule 5
        _, _, _, vs, ve, _ = first[b"id"]
        text = body[vs:ve]
        if not text.isdigit():
            return plain(DEFER)
        if int(text) > 0xFFFFFFFF:
            return plain(INVALID)
        rid = int(text)
    if b"method" not in first or first[b"method"][2] != "string":  # rule 6
        return plain(INVALID, rid)
    _, _, _, ms, me, mesc = first[b"method"]
    if mesc:
        return plain(DEFER)
    name = bytes(body[ms:me])
    for m in range(table.nmethods):  # rule 7
        a, b = table.offs[m], table.offs[m + 1]
        if a <= b <= len(table.names) and table.names[a:b] == name:
            if b"params" in first:  # rule 8
                _, _, vt, vs, ve, _ = first[b"params"]
                if vt == "string":  # (string() gives the span without the quotes)
                    vs, ve = vs - 1, ve + 1
                return CALL, m, rid, vs, ve - vs
            return CALL, m, rid, 0, 0
    return plain(NOT_FOUND, rid)


def route_entries(buf, entries, table=IDL, types=None):
    """Rules 1-8 over (offset, length) entries of ``buf``; ``types`` as d_reply_types."""
    out = []
    for i, (off, ln) in enumerate(entries):
        if types is not None and types[i] != DATA:
            out.append((NONE, NO_METHOD, 0, 0, 0))
        elif not (0 <= off <= len(buf) and ln <= len(buf) - off):
            out.append((RANGE, NO_METHOD, 0, 0, 0))
        else:
            out.append(route_body(buf[off:off + ln], table))
    return out


def back_to_back(bodies, nul=1):
    """Bodies as the unpack leaves them: (buffer, (offset, length) entries)."""
    buf, entries = bytearray(), []
    for b in bodies:
        entries.append((len(buf), len(b)))
        buf += b + b"\0" * nul
    return bytes(buf), entries


def groups_of(routed, nmethods):
    """(order, group_first): a Python stable sort by bucket."""
    def bucket(r):
        return {CALL: r[1], NOT_FOUND: nmethods, INVALID: nmethods + 1, DEFER: nmethods + 2}.get(r[0])
    keyed = [(bucket(r), i) for i, r in enumerate(routed) if bucket(r) is not None]
    keyed.sort(key=lambda k: k[0])
    first = [sum(1 for b, _ in keyed if b < g) for g in range(nmethods + 4)]
    return [i for _, i in keyed], first


# ---- canonical requests -------------------------------------------------------------------
def canonical(method, params, rid):
    """What rpc_codec_encode_request + cJSON_PrintUnformatted emit: jsonrpc, method, params
    (when given), id, no whitespace, bytes >= 0x80 as they are."""
    d = {"jsonrpc": "2.0", "method": method}
    if params is not None:
        d["params"] = params
    d["id"] = rid
    return json.dumps(d, separators=(",", ":"), ensure_ascii=False).encode()


def canonical_params(rng, m, pad=0):
    """Parameters of IDL method index m as the client stubs build them (rpc_client_gen.c)."""
    i32 = lambda: rng.randrange(-2**31, 2**31)  # noqa: E731
    dbl = lambda: rng.choice([0.5, -1.25, 3, 1e20, 2.5e-7, 12345.678])  # noqa: E731  (a whole double prints as 3)
    if m == 0:
        return {}
    if m == 1:
        return {"x": str(rng.randrange(-2**63, 2**63))}
    if m == 2:
        return {"a": i32(), "b": i32()}
    if m == 3:
        return {"a": dbl(), "b": dbl()}
    if m == 4:
        return {"n": i32()}
    if m == 5:
        alphabet = "abcdefghijklmnopqrstuvwxyz0123456789 _-/\\\"é中"
        return {"s": "".join(rng.choice(alphabet) for _ in range(pad if pad else rng.randrange(0, 40)))}
    return {"a": i32(), "b": dbl(), "ok": rng.random() < 0.5}


def canonical_set(seed, count):
    """Canonical requests over the seven methods, unknown methods and ids at the edges."""
    rng = random.Random(seed)
    out = []
    ids = [0, 1, 4294967295, 4294967296, 7, 65536]
    for k in range(count):
        rid = ids[k % len(ids)] if k < 4 * len(ids) else rng.randrange(0, 2**32)
        m = k % 9
        if m < 7:
            out.append(canonical(METHODS[m].decode(), canonical_params(rng, m), rid))
        elif m == 7:
            out.append(canonical(rng.choice(["nope", "", "pin", "pingg", "PING", "add_i64"]), {}, rid))
        else:
            out.append(canonical(METHODS[rng.randrange(7)].decode(), None, rid))
    return out


def mutation_set(seed, count):
    """Canonical requests with one byte flipped, inserted or deleted, or truncated."""
    rng = random.Random(seed)
    base = canonical_set(seed ^ 0x5EED, 64)
    pool = b'{}[],:"\\ \t\n\r0123456789-+.eEtfnu/abx\x00\x01\x1f\x7f\x80\xff'
    out = []
    for _ in range(count):
        b = bytearray(rng.choice(base))
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
        out.append(bytes(b))
    return out


# ---- the case table -------------------------------------------------------------------------
def _deep(depth):
    """A request whose params nest to exactly `depth` (the root object is depth 1)."""
    return b'{"method":"ping","params":' + b"[" * (depth - 1) + b"]" * (depth - 1) + b',"id":3}'


def _tokens(count):
    """A request with exactly `count` tokens: { "method" : "ping" , "params" : [ ] } is 10
    around an array of k numbers and k - 1 commas, and , "a" : [ ] is five more."""
    tail = b"" if count % 2 else b',"a":[]'
    k = (count - (9 if count % 2 else 14)) // 2
    return b'{"method":"ping","params":[' + b",".join(b"1" for _ in range(k)) + b"]" + tail + b"}"


def _long(n):
    body = canonical("strlen_s", {"s": ""}, 9)
    pad = n - len(body)
    return canonical("strlen_s", {"s": "x" * pad}, 9)


#: (name, body, the kind it must read, written down by hand from include/rpccrc.h)
CASES = [
    ("ping", b'{"jsonrpc":"2.0","method":"ping","params":{},"id":1}', CALL),
    ("add", b'{"jsonrpc":"2.0","method":"add_i32","params":{"a":1,"b":-2},"id":4294967295}', CALL),
    ("whitespace", b' \t\r\n{ "method" : "mix3" , "params" : { "a" : 1 , "b" : 2.5e-3 , "ok" : true } , "id" : 12 }\n', CALL),
    ("unknown method", b'{"method":"nope","id":5}', NOT_FOUND),
    ("empty method", b'{"method":"","id":5}', NOT_FOUND),
    ("prefix of a name", b'{"method":"pin","id":5}', NOT_FOUND),
    ("name plus a byte", b'{"method":"pingg","id":5}', NOT_FOUND),
    # the lenient parser's examples: each defers
    ("trailing garbage", b'{"method":"ping"} trailing garbage', DEFER),
    ("leading zero", b'{"method":"ping","x":01}', DEFER),
    ("trailing dot", b'{"method":"ping","x":5.}', DEFER),
    ("id 007", b'{"method":"ping","id":007}', DEFER),
    ("control byte in a string", b'{"method":"ping","x":"a\x01b"}', DEFER),
    ("BOM", b'\xef\xbb\xbf{"method":"ping"}', DEFER),
    ("byte <= 32 as whitespace", b'{"method":"ping",\x0b"x":1}', DEFER),
    ("top-level array", b"[1,2,3]", DEFER),
    ("NaN", b'{"method":"ping","x":NaN}', DEFER),
    ("0 byte", b'{"method":"ping"}\x00', DEFER),
    ("u escape", b'{"method":"ping","x":"\\u0041"}', DEFER),
    ("u escape 0000", b'{"method":"ping","x":"\\u0000"}', DEFER),
    ("bad escape", b'{"method":"ping","x":"\\q"}', DEFER),
    ("bytes >= 0x80", b'{"method":"ping","x":"\xff\xfe\x80"}', CALL),
    # duplicate keys: the first wins
    ("duplicate method", b'{"method":"ping","method":"nope","id":1}', CALL),
    ("duplicate method 2", b'{"method":7,"method":"ping","id":1}', INVALID),
    ("duplicate id", b'{"id":"x","id":9,"method":"ping"}', CALL),
    ("duplicate params", b'{"method":"ping","params":[1],"params":{"a":2}}', CALL),
    # id forms
    ("id absent", b'{"method":"ping"}', CALL),
    ("id string", b'{"method":"ping","id":"12"}', CALL),
    ("id null", b'{"method":"ping","id":null}', CALL),
    ("id 0", b'{"method":"ping","id":0}', CALL),
    ("id max", b'{"method":"ping","id":4294967295}', CALL),
    ("id max + 1", b'{"method":"ping","id":4294967296}', INVALID),
    ("id huge", b'{"id":99999999999999999999999999,"method":"ping"}', INVALID),
    ("id 42949672950", b'{"id":42949672950,"method":"ping"}', INVALID),
    ("id -1", b'{"method":"ping","id":-1}', DEFER),
    ("id 1.9", b'{"method":"ping","id":1.9}', DEFER),
    ("id 1e3", b'{"method":"ping","id":1e3}', DEFER),
    ("id -0", b'{"id":-0}', DEFER),
    ("id object", b'{"method":"nope","id":{"id":4}}', NOT_FOUND),
    ("big id before a bad method", b'{"id":4294967296,"method":"a\\/b"}', INVALID),
    ("big id behind a bad method", b'{"method":"a\\/b","id":4294967296}', INVALID),
    # method forms
    ("method absent", b'{"id":77}', INVALID),
    ("method number", b'{"method":5,"id":78}', INVALID),
    ("method null", b'{"id":79,"method":null}', INVALID),
    ("method with an escape", b'{"method":"a\\/b","id":1}', DEFER),
    ("escaped key", b'{"me\\/thod":"ping","id":1}', DEFER),
    ("escaped key inside", b'{"method":"ping","params":{"a\\/b":1},"id":1}', CALL),
    ("empty object", b"{}", INVALID),
    # nested method and id do not count
    ("nested method and id", b'{"params":{"method":"ping","id":5},"id":6}', INVALID),
    ("nested first", b'{"x":{"method":"nope","id":5},"method":"is_even","params":{"n":2},"id":6}', CALL),
    ("nested in an array", b'{"x":[{"id":5,"method":"nope"}],"method":"ping"}', CALL),
    # params forms
    ("params object", b'{"method":"is_even","params":{"n":4},"id":1}', CALL),
    ("params array", b'{"method":"is_even","params":[1,[2,{"a":"]"}]],"id":1}', CALL),
    ("params number", b'{"method":"ping","params":-12.5e+3,"id":1}', CALL),
    ("params number last", b'{"method":"ping","params":12 }', CALL),
    ("params string", b'{"method":"ping","params":"a\\"}b","id":1}', CALL),
    ("params literal", b'{"params":false,"method":"ping"}', CALL),
    ("params empty array", b'{"params":[ ],"method":"ping"}', CALL),
    ("params absent", b'{"method":"strlen_s","id":1}', CALL),
    # limits
    ("depth 32", _deep(32), CALL),
    ("depth 33", _deep(33), DEFER),
    ("tokens 256", _tokens(256), CALL),
    ("tokens 255", _tokens(255), CALL),
    ("tokens 257", _tokens(257), DEFER),
    ("tokens 258", _tokens(258), DEFER),
    ("length 1024", _long(1024), CALL),
    ("length 1025", _long(1025), DEFER),
    # a body that ends inside a token
    ("ends in a string", b'{"method":"ping","x":"abc', DEFER),
    ("ends in an escape", b'{"method":"ping","x":"abc\\', DEFER),
    ("ends in a literal", b'{"method":"ping","x":tru', DEFER),
    ("ends in a number", b'{"method":"ping","x":12', DEFER),
    ("ends after the colon", b'{"method":', DEFER),
    ("ends in a key", b'{"meth', DEFER),
    ("one byte", b"{", DEFER),
    ("whitespace only", b"  ", DEFER),
    # grammar
    ("trailing comma", b'{"method":"ping",}', DEFER),
    ("array trailing comma", b'{"method":"ping","x":[1,]}', DEFER),
    ("missing colon", b'{"method" "ping"}', DEFER),
    ("mismatched closer", b'{"method":"ping","x":[1}}', DEFER),
    ("unquoted key", b'{method:"ping"}', DEFER),
    ("plus sign", b'{"method":"ping","x":+1}', DEFER),
    ("lone minus", b'{"method":"ping","x":-}', DEFER),
    ("exponent without digits", b'{"method":"ping","x":1e}', DEFER),
    ("exponent sign without digits", b'{"method":"ping","x":1e+}', DEFER),
    ("dot first", b'{"method":"ping","x":.5}', DEFER),
    ("literal glued", b'{"method":"ping","x":truefalse}', DEFER),
    ("capital literal", b'{"method":"ping","x":True}', DEFER),
    ("good numbers", b'{"method":"ping","x":[0,-0,0.0,-1.5e-10,1E+2,10,9007199254740993]}', CALL),
    ("two roots", b'{"method":"ping"}{"method":"ping"}', DEFER),
    ("form feed", b'{"method":"ping"}\x0c', DEFER),
]
# long strings (the walk steps over four plain bytes at a time): a control byte, an escape, a
# bad escape and the closing quote at every position of a word, bytes >= 0x80 all through
for _k in range(4):
    _a = b"a" * (9 + _k)
    CASES += [
        ("long string, control byte %d" % _k, b'{"method":"ping","x":"' + _a + b'\x1f' + b"b" * 9 + b'"}', DEFER),
        ("long string, 0x7f %d" % _k, b'{"method":"ping","x":"' + _a + b'\x7f\x20!#[]' + b"b" * 9 + b'"}', CALL),
        ("long string, escapes %d" % _k, b'{"method":"ping","x":"' + _a + b'\\"' + _a + b'\\\\' + b"b" * 9 + b'"}', CALL),
        ("long string, bad escape %d" % _k, b'{"method":"ping","x":"' + _a + b'\\x' + b"b" * 9 + b'"}', DEFER),
        ("long string, high bytes %d" % _k, b'{"method":"ping","x":"' + _a + b'\x80\xff\xa2\xdc' * 5 + b'"}', CALL),
        ("long key %d" % _k, b'{"' + _a + b'method":"nope","method":"ping","' + _a + b'\x05":1}', DEFER),
        ("long method %d" % _k, b'{"method":"' + _a + b'ping","id":%d}' % _k, NOT_FOUND),
    ]


def case_entries(pad_front=3):
    """The table as one buffer of bodies back to back (a few other bytes in front and between)
    and its (offset, length) entries, with entries of the other kinds among them."""
    buf = bytearray(b"#" * pad_front)
    entries, types = [], []
    for k, (_, body, _) in enumerate(CASES):
        entries.append((len(buf), len(body)))
        types.append(DATA)
        buf += body
        if k % 7 == 3:
            buf += b"\0"  # the unpack's NUL: never looked at
    ping = b'{"method":"ping"}'
    at = len(buf)
    buf += ping
    extra = [((at, len(ping)), PING), ((at, len(ping)), PONG), ((at, len(ping)), TYPE_NONE),
             ((1 << 62, 5), TYPE_NONE),               # rule 1: the offset is not looked at
             ((len(buf) - 3, 4), DATA),               # leaves the buffer by one byte
             ((len(buf) + 1, 0), DATA),               # starts behind the end
             ((2**64 - 2, 8), DATA),                  # would wrap
             ((len(buf), 0), DATA),                   # empty at the end: inside, and DEFER (len 0)
             ((at, len(ping)), DATA), ((at, len(ping)), DATA)]  # the same bytes twice
    for e, t in extra:
        entries.append(e)
        types.append(t)
    return bytes(buf), entries, types


#: tables beside the IDL's: (name, table, bodies) -- 0 methods, 256 methods, duplicate names,
#: one name a prefix of another, a broken offset word, the empty name
def table_cases():
    bodies = [b'{"method":"ping","id":1}', b'{"method":"pin","id":2}', b'{"method":"","id":3}',
              b'{"method":"m255","id":4}', b'{"method":"m0","id":5}', b'{"method":"m25","id":6}',
              b'{"method":"pingping","id":7}', b'{"id":8}']
    many = table_of([b"m%d" % k for k in range(256)])
    broken = table_of([b"pin", b"ping", b"m0"])
    non_monotone = Table(broken.names, [0, 7, 3, 7])   # "pinping", a name that runs backwards, then "ping"
    leaves = Table(broken.names, [0, 3, 7, 4000])      # the last name leaves method_bytes
    return [
        ("no methods", Table(b"", [0]), bodies),
        ("256 methods", many, bodies),
        ("duplicate names", table_of([b"ping", b"ping", b"m0"]), bodies),
        ("prefix first", table_of([b"pin", b"ping", b"pingping"]), bodies),
        ("prefix last", table_of([b"pingping", b"ping", b"pin"]), bodies),
        ("empty name", table_of([b"ping", b"", b"m0"]), bodies),
        ("non-monotone word", non_monotone, bodies),
        ("word leaves the names", leaves, bodies),
    ]
