"""A seeded corpus of (name, params text or None, id) triples for the frame request
(tests/test_request_fuzz.py).  The generator emits only forms that cJSON reprints unchanged --
integers below 2^31 in magnitude, halves such as 2.5, true / false / null, strings of printable
ASCII without `"` or `\\` plus the escape \\n, arrays and objects to depth 4, no whitespace -- so
that the reference's encoder, which parses the params and prints them again, must give exactly
the bytes the device call copies."""
import random
from typing import NamedTuple

import route_cases as rtc

COUNT = 4000
IDS = (0, 9, 10, 2147483647, 2147483648, 4294967295)
ALPHABET = [chr(c) for c in range(0x20, 0x7F) if chr(c) not in '"\\']
EXTRA_NAMES = [b"", b"x", b"a.b", b"rpc.discover", b"caf\xc3\xa9", b"name with spaces", b"m" * 64, b"Z" * 255]


class Corpus(NamedTuple):
    names: list    # the method table: the IDL's seven names, then EXTRA_NAMES
    triples: list  # [(method index, params text or None, id)]


def string(rng):
    chars = [rng.choice(ALPHABET) if rng.random() < 0.93 else "\\n" for _ in range(rng.randrange(0, 24))]
    return '"%s"' % "".join(chars)


def number(rng):
    k = rng.randrange(4)
    if k == 0:
        return str(rng.randrange(-9, 10))
    if k == 1:
        return str(rng.randrange(-(2 ** 31) + 1, 2 ** 31))
    if k == 2:
        return "%d.5" % rng.randrange(0, 100000) if rng.random() < 0.5 else "-%d.5" % rng.randrange(0, 100000)
    return str(rng.randrange(-100000, 100000))


def value(rng, depth):
    k = rng.randrange(8 if depth < 4 else 5)
    if k < 2:
        return number(rng)
    if k == 2:
        return rng.choice(["true", "false", "null"])
    if k < 5:
        return string(rng)
    n = rng.randrange(0, 5)
    if k == 5:
        return "[%s]" % ",".join(value(rng, depth + 1) for _ in range(n))
    return "{%s}" % ",".join("%s:%s" % (string(rng), value(rng, depth + 1)) for _ in range(n))


def corpus(seed, count=COUNT):
    rng = random.Random(seed)
    names = list(rtc.METHODS) + EXTRA_NAMES
    triples = []
    for k in range(count):
        m = rng.randrange(len(names))
        rid = IDS[k % len(IDS)] if k < 60 else rng.randrange(0, 2 ** 32)
        r = rng.random()
        if r < 0.08:
            text = None
        elif r < 0.75:  # what a stub sends: an object or an array at the top
            text = value(rng, 1)
            while text[0] not in "[{":
                text = value(rng, 1)
        else:
            text = value(rng, 1)
        triples.append((m, None if text is None else text.encode(), rid))
    return Corpus(names, triples)
