"""The frame resolve's rules (include/rpccrc.h, rpc_frames_resolve_device) in plain Python, and
the cases the emulator and the GPU are held against.

The strict subset is route_cases' hand-written checker (rule 3 is the route's word for word);
everything else is written out here.  Nothing shares code with rpc_amd/csrc/frames_resolve.h:
the join below is a dictionary and two loops, not a hash table."""
import json
import random
from typing import NamedTuple

import numpy as np

from route_cases import MAX_BODY, MAX_DEPTH, MAX_TOKENS, Defer, Strict  # noqa: F401

NONE, MATCHED, UNKNOWN, DUPLICATE, INVALID, DEFER, RANGE = range(7)
NO_SLOT = 0xFFFFFFFF
MAX_PENDING = 1 << 24
DATA, PING, PONG = 0, 1, 2
KIND_NAMES = ["NONE", "MATCHED", "UNKNOWN", "DUPLICATE", "INVALID", "DEFER", "RANGE"]

#: the multiplicative hash of rpc_amd/csrc/frames_resolve.h (restated: tests build collisions with it)
HASH_MUL = 2654435761


def table_bits(npending):
    bits = 1
    while (1 << bits) < 2 * npending:
        bits += 1
    return bits


def hash_cell(rid, bits):
    return ((rid * HASH_MUL) & 0xFFFFFFFF) >> (32 - bits)


def colliding_ids(count, npending, cell=None):
    """``count`` distinct ids whose hash cell in the table of ``npending`` slots is ``cell`` (default:
    the last cell, so that the run wraps)."""
    bits = table_bits(npending)
    cell = (1 << bits) - 1 if cell is None else cell
    out, rid = [], 1
    while len(out) < count:
        if hash_cell(rid, bits) == cell:
            out.append(rid)
        rid += 1
    return out


def decode_body(body):
    """Rules 3-7 for one body that lies inside the buffer: (kind, id, result_off, result_len,
    error_off, error_len) with kind DEFER, INVALID or UNKNOWN (decoded; the join goes on)."""
    plain = lambda kind: (kind, 0, 0, 0, 0, 0)  # noqa: E731
    if len(body) == 0 or len(body) > MAX_BODY:
        return plain(DEFER)
    try:
        members = Strict(bytes(body)).members
    except Defer:
        return plain(DEFER)
    if any(kesc for _, kesc, *_ in members):  # rule 4
        return plain(DEFER)
    first = {}
    for m in members:  # rule 5: ASCII case folded, the first wins
        first.setdefault(m[0].lower(), m)
    if b"id" not in first or first[b"id"][2] != "number":  # rule 6
        return plain(INVALID)
    _, _, _, vs, ve, _ = first[b"id"]
    text = bytes(body[vs:ve])
    if not text.isdigit() or int(text) > 0xFFFFFFFF:
        return plain(DEFER)
    spans = []
    for name in (b"result", b"error"):  # rule 7
        if name in first:
            _, _, vt, vs, ve, _ = first[name]
            if vt == "string":  # (string() gives the span without the quotes)
                vs, ve = vs - 1, ve + 1
            spans += [vs, ve - vs]
        else:
            spans += [0, 0]
    return (UNKNOWN, int(text), *spans)


class Resolved(NamedTuple):
    kind: list
    id: list
    result_off: list
    result_len: list
    error_off: list
    error_len: list
    slot: list
    slot_entry: list
    open: list  # the open slots, ascending (nopen is its length)


def resolve(buf, offs, lens, types, pending) -> Resolved:
    """Rules 1-9 over a whole call.  ``types`` may be None."""
    n = len(offs)
    rows = []
    for i in range(n):
        if types is not None and types[i] != DATA:
            rows.append((NONE, 0, 0, 0, 0, 0))
        elif not (offs[i] <= len(buf) and lens[i] <= len(buf) - offs[i]):
            rows.append((RANGE, 0, 0, 0, 0, 0))
        else:
            rows.append(decode_body(bytes(buf[offs[i]:offs[i] + lens[i]])))
    lowest = {}
    for s, rid in enumerate(pending):
        lowest.setdefault(int(rid), s)
    kind = [r[0] for r in rows]
    slot = [NO_SLOT] * n
    slot_entry = [NO_SLOT] * len(pending)
    for i in range(n):  # pending_take in arrival order
        if kind[i] != UNKNOWN or rows[i][1] not in lowest:
            continue
        s = lowest[rows[i][1]]
        slot[i] = s
        if slot_entry[s] == NO_SLOT:
            slot_entry[s], kind[i] = i, MATCHED
        else:
            kind[i] = DUPLICATE
    return Resolved(kind, *[[r[k] for r in rows] for k in range(1, 6)], slot, slot_entry,
                    [s for s in range(len(pending)) if slot_entry[s] == NO_SLOT])


# ---- the case table ------------------------------------------------------------
def reply(rid, result=None, error=None):
    d = {"jsonrpc": "2.0"}
    if result is not None:
        d["result"] = result
    if error is not None:
        d["error"] = error
    d["id"] = rid
    return json.dumps(d, separators=(",", ":")).encode()


def _cased(word):
    return [word.lower(), word.upper(), word.capitalize(), word[:-1].lower() + word[-1].upper()]


#: name -> body: what a client may receive, friendly and hostile
CASES = {
    "result": reply(7, result=42),
    "error": reply(8, error={"code": -32601, "message": "Method not found"}),
    "both": b'{"id":9,"result":1,"error":{"code":1}}',
    "neither": b'{"jsonrpc":"2.0","id":10}',
    "null_result": b'{"result":null,"id":11}',
    "null_error": b'{"id":12,"error":null,"result":null}',
    "id_zero": reply(0, result="z"),
    "id_max": reply(4294967295, result=[1, 2]),
    "id_over": b'{"id":4294967296,"result":1}',
    "id_over_long": b'{"id":99999999999999999999,"result":1}',
    "id_9digits": b'{"id":429496729,"result":1}',
    "id_edge_lo": b'{"id":4294967290,"result":1}',
    "id_edge_hi": b'{"id":4294967299,"result":1}',
    "id_signed": b'{"id":-1,"result":1}',
    "id_neg_zero": b'{"id":-0,"result":1}',
    "id_fraction": b'{"id":1.0,"result":1}',
    "id_exponent": b'{"id":1e2,"result":1}',
    "id_leading_zero": b'{"id":01,"result":1}',
    "id_string": b'{"id":"5","result":1}',
    "id_null": b'{"id":null,"result":1}',
    "id_true": b'{"id":true,"result":1}',
    "id_array": b'{"id":[5],"result":1}',
    "id_object": b'{"id":{"id":5},"result":1}',
    "id_absent": b'{"result":1}',
    "empty_object": b"{}",
    "wrong_type_id_first": b'{"ID":"x","id":5,"result":1}',
    "good_id_first": b'{"id":5,"ID":"x","result":1}',
    "first_result_wins": b'{"id":13,"RESULT":1,"result":[2,3]}',
    "first_error_wins": b'{"id":14,"error":"a","Error":{"b":1}}',
    "nested_id_ignored": b'{"result":{"id":99,"error":1},"id":15}',
    "nested_only": b'{"result":{"id":99}}',
    "near_miss_keys": b'{"i":1,"idd":2,"resul":3,"results":4,"erro":5,"errors":6,"id":16}',
    "near_miss_bytes": b'{"i\xc4":1,"re\xd3ult":2,"id":17,"@d":3,"iD":4}',
    "key_backslash": b'{"i\\u0064":5,"id":5,"result":1}',
    "key_backslash_other": b'{"a\\nb":1,"id":5,"result":1}',
    "nested_key_backslash": b'{"result":{"a\\nb":1},"id":18}',
    "string_result_escapes": b'{"id":19,"result":"a\\"b\\\\c\\/\\b\\f\\n\\r\\t"}',
    "string_result_u": b'{"id":19,"result":"\\u0041"}',
    "string_result_high": b'{"id":20,"result":"\xc3\xa9\xff\x80"}',
    "string_result_control": b'{"id":20,"result":"a\x01b"}',
    "zero_byte": b'{"id":21,\x00"result":1}',
    "zero_byte_in_string": b'{"id":21,"result":"a\x00b"}',
    "whitespace": b' \t\n\r{ "id" \t:\n 22 , "result" : [ 1 , { "a" : null } ] \r\n, "error" : false } \n',
    "number_results": b'{"id":23,"result":-1.5e+10,"error":0}',
    "literal_results": b'{"result":true,"error":false,"id":24}',
    "empty_containers": b'{"result":{},"error":[],"id":25}',
    "empty_string_result": b'{"result":"","id":26}',
    "value_then_id_last": b'{"result":"x","id":27}',
    "array_root": b'[{"id":1,"result":1}]',
    "scalar_root": b"5",
    "string_root": b'"id"',
    "trailing_garbage": b'{"id":28,"result":1}x',
    "trailing_object": b'{"id":28,"result":1}{}',
    "truncated": b'{"id":29,"result":',
    "truncated_in_string": b'{"id":29,"result":"abc',
    "truncated_number": b'{"id":29',
    "single_quotes": b"{'id':30}",
    "bare_key": b'{id:30}',
    "trailing_comma": b'{"id":30,}',
    "double_comma": b'{"id":30,,"result":1}',
    "missing_colon": b'{"id" 30}',
    "bad_literal": b'{"id":31,"result":nul}',
    "bad_literal_case": b'{"id":31,"result":True}',
    "bad_number": b'{"id":31,"result":1.}',
    "bad_escape": b'{"id":31,"result":"\\x"}',
    "form_feed_ws": b'{"id":31,\x0c"result":1}',
    "depth_ok": b'{"id":32,"result":' + b"[" * (MAX_DEPTH - 1) + b"]" * (MAX_DEPTH - 1) + b"}",
    "depth_over": b'{"id":32,"result":' + b"[" * MAX_DEPTH + b"]" * MAX_DEPTH + b"}",
    # { "id" : 33 , "result" : [ ... ] }: 10 tokens around the elements, 2k - 1 for k scalar elements
    # (an odd sum: the [] among the elements makes it 256; 124 scalars make it 257)
    "tokens_ok": b'{"id":33,"result":[' + b",".join([b"1"] * 122 + [b"[]"]) + b"]}",
    "tokens_over": b'{"id":33,"result":[' + b",".join([b"1"] * 124) + b"]}",
    "len_max": b'{"id":34,"result":"' + b"x" * (MAX_BODY - 21) + b'"}',
    "len_over": b'{"id":34,"result":"' + b"x" * (MAX_BODY - 20) + b'"}',
    "long_plain_then_quote": b'{"id":35,"result":"' + b"abcdefg" * 40 + b'","error":"' + b"h" * 33 + b'"}',
}
for _w in ("id", "result", "error"):
    for _k, _v in enumerate(_cased(_w)):
        _keys = {"id": "id", "result": "result", "error": "error", _w: _v}
        CASES["case_%s_%d" % (_w, _k)] = ('{"%s":%d,"%s":{"a":[1]},"%s":"e"}' % (
            _keys["id"], 100 + _k, _keys["result"], _keys["error"])).encode()
assert len(CASES["len_max"]) == MAX_BODY and len(CASES["len_over"]) == MAX_BODY + 1
assert Strict(CASES["tokens_ok"]).tokens == MAX_TOKENS


class Call(NamedTuple):
    """One call's inputs as the library takes them."""
    buf: bytes
    offs: list
    lens: list
    types: object  # list or None
    pending: list

    def expect(self):
        return resolve(self.buf, self.offs, self.lens, self.types, self.pending)


def pack_bodies(bodies, nul=1, gap=0):
    """Bodies back to back as the unpack leaves them (a NUL behind each with ``nul``)."""
    buf, offs, lens = bytearray(), [], []
    for b in bodies:
        offs.append(len(buf))
        lens.append(len(b))
        buf += b + b"\0" * nul + b"\xee" * gap
    return bytes(buf), offs, lens


def case_call(nul=1):
    """The whole case table in one call, against a pending table that holds most of its ids, one of
    them twice, with strangers in between."""
    names = sorted(CASES)
    buf, offs, lens = pack_bodies([CASES[k] for k in names], nul=nul)
    ids = []
    for k in names:
        row = decode_body(CASES[k])
        if row[0] == UNKNOWN and row[1] not in ids and row[1] % 5 != 0:
            ids.append(row[1])
    random.Random(7).shuffle(ids)
    pending = ids[:3] + [777777] + ids[3:9] + [ids[3]] + ids[9:] + [888888]
    return names, Call(buf, offs, lens, None, pending)


def as_arrays(call):
    """numpy arrays for the library's arguments."""
    return (np.frombuffer(call.buf, dtype=np.uint8).copy(), np.asarray(call.offs, dtype=np.uint64),
            np.asarray(call.lens, dtype=np.uint32),
            None if call.types is None else np.asarray(call.types, dtype=np.uint16),
            np.asarray(call.pending, dtype=np.uint32))


# ---- generated bodies ----------------------------------------------------------------
def _value(rng, depth=0):
    k = rng.randrange(8 if depth < 2 else 6)
    if k == 0:
        return rng.randrange(-1000, 1000)
    if k == 1:
        return rng.random() * 1e6
    if k == 2:
        return "".join(rng.choice('ab "\\/\n\té') for _ in range(rng.randrange(12)))
    if k == 3:
        return rng.choice([True, False, None])
    if k == 4:
        return "x" * rng.randrange(40)
    if k == 5:
        return rng.randrange(1 << 40)
    if k == 6:
        return [_value(rng, depth + 1) for _ in range(rng.randrange(4))]
    return {"k%d" % j: _value(rng, depth + 1) for j in range(rng.randrange(3))}


def canonical_set(seed, count):
    """Replies as a JSON library prints them (json.dumps, ASCII-escaped non-ASCII aside: the strict
    subset defers \\u, so ensure_ascii is off), keys shuffled, every id in 0 .. 2^32 - 1."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        items = [("jsonrpc", "2.0"), ("id", rng.choice([rng.randrange(1 << 32), rng.randrange(1000)]))]
        which = rng.randrange(4)
        if which & 1:
            items.append(("result", _value(rng)))
        if which & 2:
            items.append(("error", {"code": -rng.randrange(33000), "message": "m" * rng.randrange(20)}))
        rng.shuffle(items)
        out.append(json.dumps(dict(items), separators=(",", ":"), ensure_ascii=False).encode())
    return out


def mutation_set(seed, count):
    """Canonical replies and case-table bodies with one byte flipped, inserted or deleted, or cut
    short."""
    rng = random.Random(seed)
    base = canonical_set(seed ^ 0x5EED, 200) + [b for b in CASES.values() if len(b) < 200]
    pool = b'{}[]",:\\ \t\n0123456789-+.eEtfnIiDdRrEe\x00\x7f\x80'
    out = []
    for _ in range(count):
        b = bytearray(rng.choice(base))
        how, at = rng.randrange(4), rng.randrange(len(b))
        if how == 0:
            b[at] = rng.choice(pool)
        elif how == 1:
            b.insert(at, rng.choice(pool))
        elif how == 2:
            del b[at]
        else:
            del b[at:]
        out.append(bytes(b))
    return out


def join_calls():
    """name -> Call: the shapes at which the join can go wrong."""
    rng = random.Random(11)
    calls = {}
    # 64 pending ids in one hash cell, the last: the run wraps past the table's end
    ids = colliding_ids(64, 64)
    assert table_bits(64) == 7 and {hash_cell(i, 7) for i in ids} == {127}
    order = ids + [ids[5], 123456789]  # every slot answered, one of them twice, and a stranger
    rng.shuffle(order)
    calls["collide_wrap"] = Call(*pack_bodies([reply(i, result=i) for i in order]), None, ids)
    # an id held by slots 3 and 9
    pend = [10, 11, 12, 500, 13, 14, 15, 16, 17, 500, 18, 19]
    calls["id_in_two_slots"] = Call(*pack_bodies([reply(500, result="a"), reply(19, error={"code": 1}),
                                                  reply(500, result="b")]), None, pend)
    # three replies to one id at entries 1, 255 and 256 (two workgroups)
    rids = list(range(1000, 1257))
    rids[1] = rids[255] = rids[256] = 4242
    pend = sorted(set(rids), key=lambda i: (i * 7919) % 1009)
    calls["three_replies"] = Call(*pack_bodies([reply(i, result=[i]) for i in rids]), None, pend)
    for npending in (0, 1, 2, 257):
        pend = [rng.randrange(1 << 32) for _ in range(npending)]
        if npending:
            pend[-1] = 0
        if npending > 1:
            pend[0] = 4294967295
        bodies = [reply(i, result=None, error=None) for i in pend[::2]] + [reply(0, result=0), reply(4294967295, error=1),
                                                                          reply(31337, result=1)]
        rng.shuffle(bodies)
        calls["npending_%d" % npending] = Call(*pack_bodies(bodies), None, pend)
    calls["no_entries"] = Call(b"", [], [], None, [5, 6, 7])
    calls["nothing"] = Call(b"", [], [], None, [])
    # non-DATA entries with garbage offsets, spans outside the buffer, an offset near 2^64
    buf, offs, lens = pack_bodies([reply(1, result=1), reply(2, result=2), reply(3, result=3), reply(4, result=4)], nul=0)
    offs2 = [offs[0], 0xDEADBEEFCAFE, offs[2], len(buf) - 3, (1 << 64) - 8, len(buf) + 1, offs[3], len(buf)]
    lens2 = [lens[0], 0xFFFFFFFF, lens[2], 4, 16, 1, lens[3], 0]
    types2 = [DATA, PING, DATA, DATA, DATA, DATA, DATA, PONG]
    calls["types_and_ranges"] = Call(buf, offs2, lens2, types2, [4, 3, 2, 1])
    calls["ranges_all_data"] = Call(buf, offs2, lens2, None, [4, 3, 2, 1])
    return calls


def big_bodies_call():
    """40 bodies of exactly 1,024 B: two staging rounds in one workgroup."""
    bodies = []
    for i in range(40):
        head = b'{"id":%d,"result":"' % (7000 + i)
        tail = b'","error":[%d]}' % i
        bodies.append(head + bytes([0x61 + i % 26]) * (MAX_BODY - len(head) - len(tail)) + tail)
    assert all(len(b) == MAX_BODY for b in bodies)
    return Call(*pack_bodies(bodies, nul=1), None, [7000 + i for i in range(39, -1, -1)])
