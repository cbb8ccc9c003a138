#!/usr/bin/env python3
"""Regenerates tests/golden/resolve_golden.json: reply bodies, each answered by the reference
client's own rpc_codec_decode_response behind tests/dropin/ref_decode.c (compiled with the
reference's rpc_codec.c and cJSON.c in place, into a temporary directory: tests/resolve_ref.py).
Class c holds the reply strings recorded in route_golden.json, class h the case table of
tests/resolve_cases.py.

    python tests/golden/make_resolve_golden.py            rewrite the fixture
    python tests/golden/make_resolve_golden.py --check    exit 1 if it would change
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resolve_cases as rc  # noqa: E402
import resolve_ref  # noqa: E402

PATH = os.path.join(HERE, "resolve_golden.json")
ROUTE = os.path.join(HERE, "route_golden.json")

HOW = ("Bodies (each byte as the character of that code): class c is every reply string recorded in route_golden.json "
       "(what the reference's dispatcher sends: what a client receives); class h (hostile) is the case table of "
       "tests/resolve_cases.py in name order. Each entry is [class, body, return code, id, result, error]: the body, "
       "NUL-terminated, given to the reference's own rpc_codec_decode_response (client/rpc_codec.c with "
       "third_party/cJSON.c) by the driver tests/dropin/ref_decode.c; result and error are cJSON_PrintUnformatted of "
       "the two members (null: not there); id, result and error are 0 / null when the code is -1. "
       "tests/golden/make_resolve_golden.py writes this file, and tests/test_resolve_golden.py holds the rules, the "
       "emulator and the GPU against it.")


def bodies():
    c = [reply.encode("latin-1") for _, _, reply in json.load(open(ROUTE))["entries"]]
    return [("c", b) for b in c] + [("h", rc.CASES[k]) for k in sorted(rc.CASES)]


def dumps(doc):
    """The fixture's layout: compact, one entry per line."""
    head = '{"how":%s,"entries":[' % json.dumps(doc["how"])
    return head + ",\n".join(json.dumps(e, separators=(",", ":")) for e in doc["entries"]) + "]}"


def main():
    pairs = bodies()
    with tempfile.TemporaryDirectory() as d:
        exe = resolve_ref.build(d)
        if exe is None:
            sys.exit("the reference tree (%s) is absent" % resolve_ref.ref_dir())
        got = resolve_ref.run(exe, [b for _, b in pairs])
    text = lambda m: None if m is None else m.decode("latin-1")  # noqa: E731
    new = {"how": HOW, "entries": [[cls, b.decode("latin-1"), g.rc, g.id, text(g.result), text(g.error)]
                                   for (cls, b), g in zip(pairs, got)]}
    out = dumps(new)
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(PATH) and out == open(PATH).read() else 1)
    open(PATH, "w").write(out)
    print("wrote %s: %d entries" % (PATH, len(new["entries"])))


if __name__ == "__main__":
    main()
