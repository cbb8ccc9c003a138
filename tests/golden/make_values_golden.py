#!/usr/bin/env python3
"""Regenerates tests/golden/values_golden.json: a few hundred rows of tests/values_fuzz.py and
the probes below, each request answered by the reference's rpc_server_dispatch through
oracle/_ref/ref_dispatch (`make -C oracle dispatch` builds it where the reference tree is
present).  Recorded results, nothing else.

    python tests/golden/make_values_golden.py            rewrite the fixture
    python tests/golden/make_values_golden.py --check    exit 1 if it would change
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle  # noqa: E402
import values_cases as vc  # noqa: E402
import values_fuzz as vf  # noqa: E402
from args_cases import M  # noqa: E402

PATH = os.path.join(HERE, "values_golden.json")
SEED, ROWS = 0xB2650, 360

HOW = ("Entries: [method index, `params` span or null (each byte as the character of that code), id, the handler's "
       "typed result as a 64-bit slot (decimal), reply]. `strings` holds the bytes a STR slot (offset | length << 32) "
       "points into. The request is args_cases.request(method name, span, id). Rows: tests/values_fuzz.py's, then the "
       "doubles probed while the frame values were specified (mul_double(a=repr(d), b=1) returns d): one ulp from its "
       "15-digit text, 17 digits, the carry to 1e+23, both sides of the %g switches, the integer edges, -0.0, a tie "
       "at 15 and at 17 digits, the largest double, the smallest normal, a subnormal. Replies: each request, "
       "NUL-terminated, given to the reference's own rpc_server_dispatch by the kept driver oracle/ref_dispatch.c; "
       "tests/golden/make_values_golden.py writes this file, and tests/test_values_golden.py asks today's reference "
       "for every recorded reply.")

PROBES = [0.1 + 0.2, 1.0 / 3.0, 9.999999999999999e22, 1e23, 1e-5, 1e-4, 9.9999999999999e-5, 1e15, 999999999999999.0, 1e16,
          1e17, 123456789012345.0, 1234567890123456.0, 2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0,
          2147483647.5, -0.0, 0.0, 100000000000000.5, 100000000000001.5, 1000000000000000.25, 1000000000000005.0,
          1.7976931348623157e308, 1.797693134862315e308, 2.2250738585072014e-308, 2.225073858507203e-308, 5e-324,
          2.2250738585072009e-308, 9007199254740993.0, 0.5, -2.5, 1e22, 1e21, 123456.789e3, 5e-5, 4.35, 0.285, 1.005]


def rows():
    rs, strings = vf.rows(SEED, ROWS)
    rs += [vf.Row(M, b'{"a":%s,"b":1}' % repr(d).encode(), 5000 + k, vc.bits_of(d)) for k, d in enumerate(PROBES)]
    return rs, strings


def main():
    rs, strings = rows()
    replies = oracle.ref_dispatch(vf.bodies_of(rs))
    if replies is None:
        sys.exit("oracle/_ref/ref_dispatch is not built: make -C oracle dispatch (needs the reference tree)")
    doc = {"how": HOW, "strings": strings.decode("latin-1"),
           "entries": [[r.method, None if r.span is None else r.span.decode("latin-1"), r.rid, str(r.slot),
                        reply.decode("latin-1")] for r, reply in zip(rs, replies)]}
    text = json.dumps(doc, indent=0, ensure_ascii=True) + "\n"
    if "--check" in sys.argv:
        sys.exit(0 if open(PATH).read() == text else 1)
    open(PATH, "w").write(text)
    print("wrote %s: %d entries" % (PATH, len(rs)))


if __name__ == "__main__":
    main()
