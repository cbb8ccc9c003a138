#!/usr/bin/env python3
"""Regenerates tests/golden/route_golden.json: the fixture's own bodies (and those of EXTRA
that it does not hold yet), each answered by the reference's rpc_server_dispatch through
oracle/_ref/ref_dispatch (oracle/ref_dispatch.c; `make -C oracle dispatch` builds it where the
reference tree is present).  Classes, bodies and their order stay; only the replies and the
`how` text are written anew.

    python tests/golden/make_route_golden.py            rewrite the fixture
    python tests/golden/make_route_golden.py --check    exit 1 if it would change
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle  # noqa: E402

PATH = os.path.join(HERE, "route_golden.json")

HOW = ("Bodies (each byte as the character of that code): class c (canonical) is the output of the reference's "
       "rpc_codec_encode_request + cJSON_PrintUnformatted for the IDL's seven methods and unknown methods (ids above "
       "4294967295 and missing / wrong-type `method` written by hand in the same form); class h (hostile) is the "
       "lenient-parser, duplicate-key and id cases of tests/route_cases.py, mutation_set(0xBADC0DE, 20000) survivors "
       "(bodies the reference did not reject) and some it rejected. Replies: each body, NUL-terminated, given to the "
       "reference's own rpc_server_dispatch (server/gen/rpc_server_skeleton.c with rpc_server_helpers.c, "
       "rpc_server_impl.c and third_party/cJSON.c) by the kept driver oracle/ref_dispatch.c (length-prefixed bodies in, "
       "the returned strings out; oracle/Makefile builds it as oracle/_ref/ref_dispatch, oracle.ref_dispatch runs it); "
       "tests/golden/make_route_golden.py writes this file from its own bodies, and tests/test_route_golden.py asks "
       "today's reference for every recorded reply.")

#: (class, body) pairs to add behind the recorded ones: bodies on which the rules and the
#: reference were once found to disagree (none so far)
EXTRA = []


def dumps(doc):
    """The fixture's layout: compact, one entry per line."""
    s = json.dumps
    head = '{"how":%s,"methods":%s,"entries":[' % (s(doc["how"]), s(doc["methods"], separators=(",", ":")))
    return head + ",\n".join(s(e, separators=(",", ":")) for e in doc["entries"]) + "]}"


def main():
    doc = json.load(open(PATH))
    pairs = [(cls, body) for cls, body, _ in doc["entries"]]
    pairs += [(cls, body.decode("latin-1")) for cls, body in EXTRA if body.decode("latin-1") not in {b for _, b in pairs}]
    replies = oracle.ref_dispatch([body.encode("latin-1") for _, body in pairs])
    if replies is None:
        sys.exit("oracle/_ref/ref_dispatch missing: build it with `make -C oracle dispatch` (needs the reference tree)")
    new = {"how": HOW, "methods": doc["methods"],
           "entries": [[cls, body, reply.decode("latin-1")] for (cls, body), reply in zip(pairs, replies)]}
    text = dumps(new)
    if "--check" in sys.argv[1:]:
        sys.exit(0 if text == open(PATH).read() else 1)
    open(PATH, "w").write(text)
    print("wrote %s: %d entries" % (PATH, len(new["entries"])))


if __name__ == "__main__":
    main()
