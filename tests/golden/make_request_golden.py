#!/usr/bin/env python3
"""Regenerates tests/golden/request_golden.json: (name, params text, id) triples, each encoded by
the reference client's own rpc_codec_encode_request behind tests/dropin/ref_encode.c (compiled
with the reference's rpc_codec.c and cJSON.c in place, into a temporary directory:
tests/request_ref.py).

    python tests/golden/make_request_golden.py            rewrite the fixture
    python tests/golden/make_request_golden.py --check    exit 1 if it would change
"""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import request_ref  # noqa: E402
import route_cases as rtc  # noqa: E402

PATH = os.path.join(HERE, "request_golden.json")
IDS = (0, 9, 10, 2147483648, 4294967295)
MIN_REBUILT = 60

HOW = ("Each entry is [name, params, id, printed, request] (each byte as the character of that code; null: not "
       "there): the name and the params text, each NUL-terminated, given to the driver tests/dropin/ref_encode.c, "
       "which runs cJSON_Parse on the params and then the reference's own rpc_codec_encode_request "
       "(client/rpc_codec.c with third_party/cJSON.c); printed is cJSON_PrintUnformatted of the parsed params alone, "
       "request what the encoder returned. The IDL's seven methods with the params the stubs of "
       "client/gen/rpc_client_gen.c build, at five ids; each method without params; {} and []; nested arrays and "
       "objects; strings with \\n and with bytes >= 0x80; params the reference reprints differently; the empty name; "
       "names that need an escape. tests/golden/make_request_golden.py writes this file, and "
       "tests/test_request_golden.py holds the rules, the emulator and the GPU against it.")

EXTRA_PARAMS = [b"{}", b"[]", b"[1,2,3]", b"[[],[[]],{}]", b'{"a":{"b":{"c":[1,{"d":null}]}}}', b'[true,false,null]',
                b'{"s":"line one\\nline two"}', b'"\\n"', '{"s":"grüße 世界"}'.encode(), b'"caf\xc3\xa9"',
                b"-7", b"2.5", b'"plain"', b'[{"k":[1,[2,[3,[4]]]]},"x"]',
                # what the reference reprints differently: not rebuilt from the text
                b'{ "a" : 1 }', b"[1.0]", b'"\\u0041"', b"1e2", b'"a\\/b"']
ESCAPED_NAMES = [b'say"hi', b"back\\slash", b"two\nlines", b"unit\x1fsep", b"tab\there"]


def needs_escape(name):
    return any(c < 0x20 or c in b'"\\' for c in name)


def triples():
    rng = random.Random(0x5EED)
    out = []
    for m, name in enumerate(rtc.METHODS):
        for rid in IDS:
            text = json.dumps(rtc.canonical_params(rng, m), separators=(",", ":"), ensure_ascii=False).encode()
            out.append((name, text, rid))
    for m, name in enumerate(rtc.METHODS):
        out.append((name, None, IDS[m % len(IDS)]))
    for k, text in enumerate(EXTRA_PARAMS):
        out.append((rtc.METHODS[k % 7], text, IDS[k % len(IDS)]))
    out += [(b"", None, 1), (b"", b"{}", 4294967295), (b"", b"[0]", 0)]
    out += [("café".encode(), b'{"x":1}', 77), ("世界".encode(), None, 123456789)]
    for k, name in enumerate(ESCAPED_NAMES):
        out.append((name, b"{}" if k % 2 else None, IDS[k % len(IDS)]))
    return out


def rebuilt(entry):
    """Is the entry one that the device call must give back byte for byte?"""
    name, params, _, printed, _ = entry
    return printed == params and not needs_escape(name.encode("latin-1"))


def dumps(doc):
    """The fixture's layout: compact, one entry per line."""
    head = '{"how":%s,"entries":[' % json.dumps(doc["how"])
    return head + ",\n".join(json.dumps(e, separators=(",", ":")) for e in doc["entries"]) + "]}"


def main():
    tr = triples()
    with tempfile.TemporaryDirectory() as d:
        exe = request_ref.build(d)
        if exe is None:
            sys.exit("the reference tree (%s) is absent" % request_ref.ref_dir())
        got = request_ref.run(exe, tr)
    text = lambda m: None if m is None else m.decode("latin-1")  # noqa: E731
    new = {"how": HOW, "entries": [[text(name), text(params), rid, text(g.printed), text(g.request)]
                                   for (name, params, rid), g in zip(tr, got)]}
    assert all(e[4] is not None for e in new["entries"])
    assert sum(1 for e in new["entries"] if rebuilt(e)) >= MIN_REBUILT
    assert any(not rebuilt(e) and not needs_escape(e[0].encode("latin-1")) for e in new["entries"])
    out = dumps(new)
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(PATH) and out == open(PATH).read() else 1)
    open(PATH, "w").write(out)
    print("wrote %s: %d entries, %d rebuilt" % (PATH, len(new["entries"]), sum(1 for e in new["entries"] if rebuilt(e))))


if __name__ == "__main__":
    main()
