"""A seeded corpus of reply bodies for the frame resolve, in the manner of tests/route_fuzz.py
(whose serialiser it uses): what a client may receive from a server that is not the reference's.

  canonical  replies as cJSON prints them: jsonrpc, id, result or error, no whitespace
  reply      id / result / error / jsonrpc members with cased, shuffled, duplicated and near-miss
             keys, whitespace in every slot, every JSON type as each member's value, cJSON's
             lenient number forms as ids, ids around 2^32, every escape, \\u, bytes >= 0x80
  limits     the three limits with their neighbours (length, depth, tokens)
  roots      array and scalar roots, trailing garbage, a 0 byte inside
  edited     a canonical or reply body with 2-4 random edits
"""
import json
import random
from typing import NamedTuple

import resolve_cases as rc
import route_fuzz as rf

ID_KEYS = [b"id", b"ID", b"Id", b"iD"]
RESULT_KEYS = [b"result", b"RESULT", b"Result", b"resulT", b"rEsUlT"]
ERROR_KEYS = [b"error", b"ERROR", b"Error", b"erroR", b"eRrOr"]
NEAR_KEYS = [b"i", b"idd", b" id", b"id ", b"i\xc4", b"resul", b"results", b"result ", b"re\xd3ult", b"erro", b"errors",
             b"err0r", b"", b"jsonrpc", b"method", b"@d", b"iD "]
EDGE_IDS = [0, 1, 9, 10, 99, 4294967294, 4294967295, 4294967296, 4294967297, 42949672950, 9007199254740993,
            18446744073709551616, 429496729, 4294967289, 4294967299, 1000000000, 3999999999]
LENIENT_IDS = [b"1.", b"+1", b"01", b"1e", b"1e999", b"-", b".5", b"1e+", b"0x10", b"NaN", b"-1", b"-0", b"1.0", b"1.5",
               b"1e2", b"1E+2", b"2.5e-1", b"007", b"4294967295.0", b"4.294967295e9", b"1e0"]


class Corpus(NamedTuple):
    bodies: list
    classes: list  # the class name of each body


def canonical(rng):
    rid = rng.choice([rng.randrange(1 << 32), rng.randrange(1000), rng.choice(EDGE_IDS[:7])])
    if rng.random() < 0.8:
        v = rng.choice(["pong", str(rng.randrange(-2**62, 2**62)), rng.randrange(-2**31, 2**31), 1.5 * rng.randrange(99),
                        True, False, rng.randrange(1025), "a=%d,b=2.50,ok=true" % rng.randrange(99), None, [1, "a"],
                        {"k": {"id": 5}}, "sl/ash \"q\" \\ \n\t é"])
        return json.dumps({"jsonrpc": "2.0", "id": rid, "result": v}, separators=(",", ":"), ensure_ascii=False).encode()
    code = rng.choice([-32700, -32600, -32601, -32602, -32603, -7])
    return json.dumps({"jsonrpc": "2.0", "id": rid, "error": {"code": code, "message": "Method not found"}},
                      separators=(",", ":")).encode()


def id_text(rng, lp):
    r = rng.random()
    if r < lp:
        return rng.choice(LENIENT_IDS)
    if r < 0.55:
        return b"%d" % rng.choice([rng.randrange(1 << 32), rng.randrange(1000)])
    if r < 0.8:
        return b"%d" % rng.choice(EDGE_IDS)
    return rf.rand_value(rng, lp / 4, 0.1)  # any type


def reply(rng, lp=0.06):
    wsp = rf.pick_wsp(rng)
    members = []
    for keys, p in ((ID_KEYS, 0.95), (RESULT_KEYS, 0.6), (ERROR_KEYS, 0.4)):
        if rng.random() >= p:
            continue
        key = keys[0] if rng.random() < 0.6 else rng.choice(keys)
        value = id_text(rng, lp) if keys is ID_KEYS else rf.rand_value(rng, lp / 4, wsp)
        members.append((rf.quoted(rng, key, lp=0.02 if rng.random() < 0.1 else 0.0), value))
        if rng.random() < 0.12:  # the key again, in some case, with another value
            members.append((rf.quoted(rng, rng.choice(keys)), id_text(rng, lp) if keys is ID_KEYS else rf.scalar(rng, 0.0)))
    if rng.random() < 0.7:
        members.append((b'"jsonrpc"', b'"2.0"'))
    for _ in range(rng.choice((0, 0, 1, 2))):
        members.append((rf.quoted(rng, rng.choice(NEAR_KEYS)), rf.rand_value(rng, lp / 4, wsp)))
    rng.shuffle(members)
    return rf.gap(rng, wsp) + rf.obj(rng, members, wsp, lp / 2) + rf.gap(rng, wsp)


def limits(rng):
    which, near = rng.randrange(3), rng.choice((-1, 0, 1))
    rid = rng.randrange(1 << 32)
    if which == 0:  # length
        head = b'{"id":%d,"result":"' % rid
        return head + b"y" * (rc.MAX_BODY + near - len(head) - 2) + b'"}'
    if which == 1:  # depth: the root is 1
        d = rc.MAX_DEPTH - 1 + near
        return b'{"id":%d,"error":' % rid + b"[" * d + b"]" * d + b"}"
    k = 123 + near  # tokens: 10 around the elements, 2k - 1 for k scalars, one more for a [] among them
    items = [b"1"] * (k - 1) + [rng.choice((b"[]", b"1"))]
    return b'{"id":%d,"result":[' % rid + b",".join(items) + b"]}"


def roots(rng):
    body = canonical(rng) if rng.random() < 0.5 else reply(rng, 0.0)
    r = rng.randrange(5)
    if r == 0:
        return b"[" + body + b"]"
    if r == 1:
        return rng.choice([b"5", b'"id"', b"null", b"true", b"[]", b"", b" ", b"-", b"{"])
    if r == 2:
        return body + rng.choice([b"x", b"{}", b",", b"}", b"\x00", b' "id":1', b"//"])
    at = rng.randrange(len(body) + 1)  # a 0 byte inside
    return body[:at] + b"\x00" + body[at:]


def edited(rng):
    b = bytearray(canonical(rng) if rng.random() < 0.5 else reply(rng, 0.0))
    for _ in range(rng.randrange(2, 5)):
        how, at = rng.randrange(3), rng.randrange(len(b)) if b else 0
        if not b:
            break
        if how == 0:
            b[at] = rng.choice(rf.EDIT_POOL)
        elif how == 1:
            b.insert(at, rng.choice(rf.EDIT_POOL))
        else:
            del b[at]
    return bytes(b)


SHARES = [("canonical", canonical, 0.2), ("reply", reply, 0.5), ("limits", limits, 0.04), ("roots", roots, 0.08),
          ("edited", edited, 0.18)]


def corpus(seed, count=6000) -> Corpus:
    rng = random.Random(seed)
    bodies, classes = [], []
    for name, make, share in SHARES:
        for _ in range(int(count * share)):
            b = make(rng)
            if len(b) <= rc.MAX_BODY + 1:
                bodies.append(b)
                classes.append(name)
    order = list(range(len(bodies)))
    rng.shuffle(order)
    return Corpus([bodies[i] for i in order], [classes[i] for i in order])


def call_of(c: Corpus, seed=1):
    """The corpus as one call: the pending table holds half of the ids the rules decode (some
    twice) and as many strangers."""
    rng = random.Random(seed)
    ids = [row[1] for row in map(rc.decode_body, c.bodies) if row[0] == rc.UNKNOWN]
    pending = [i for i in ids if rng.random() < 0.5] + [rng.randrange(1 << 32) for _ in range(len(ids) // 2)]
    rng.shuffle(pending)
    return rc.Call(*rc.pack_bodies(c.bodies, nul=1), None, pending)


def rebuilt(body, row):
    """{"id":<id>[,"result":<span bytes>][,"error":<span bytes>]} of a decoded body: the reference
    prints the same members from it as from the body iff the spans are the members' values."""
    _, rid, ro, rl, eo, el = row
    out = b'{"id":%d' % rid
    if rl:
        out += b',"result":' + body[ro:ro + rl]
    if el:
        out += b',"error":' + body[eo:eo + el]
    return out + b"}"
