#!/usr/bin/env python3
"""Regenerates tests/golden/args_golden.json: a few hundred requests -- rows of
tests/args_fuzz.py's corpus and the probes below -- each answered by the reference's
rpc_server_dispatch through oracle/_ref/ref_dispatch (oracle/ref_dispatch.c; `make -C oracle
dispatch` builds it where the reference tree is present).  Recorded results, nothing else.

    python tests/golden/make_args_golden.py            rewrite the fixture
    python tests/golden/make_args_golden.py --check    exit 1 if it would change
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle  # noqa: E402
import args_cases as ac  # noqa: E402
import args_fuzz as af  # noqa: E402
from args_cases import A, E, M, N, P, S, X  # noqa: E402

PATH = os.path.join(HERE, "args_golden.json")
SEED, ROWS = 0xA2650, 360

HOW = ("Entries: [class, method index, `params` span or null (each byte as the character of that code), id, reply]. "
       "The request is args_cases.request(method name, span, id): the canonical envelope around the span. Class c "
       "(canonical) is what the reference client's stubs print, class h (hostile) tests/args_fuzz.py's other class, "
       "class p the probes run while the frame args were specified: out-of-range i32, the i64 string forms, 1e400, "
       "duplicate and wrong-case keys, non-object params, ties of the decimal conversion. Replies: each request, "
       "NUL-terminated, given to the reference's own rpc_server_dispatch by the kept driver oracle/ref_dispatch.c "
       "(oracle.ref_dispatch runs it); tests/golden/make_args_golden.py writes this file, and "
       "tests/test_args_golden.py asks today's reference for every recorded reply.")

#: (method, span): the probes.  a + b stays inside int32.
PROBES = [
    (A, b'{"a":2147483648,"b":1}'), (A, b'{"a":-2147483649,"b":1}'), (A, b'{"a":1.9,"b":-1.9}'), (A, b'{"a":1e3,"b":0}'),
    (A, b'{"a":1e400,"b":0}'), (A, b'{"a":2147483647,"b":-2147483648}'), (N, b'{"n":2147483647.9}'), (N, b'{"n":-0.0}'),
    (E, b'{"x":"9223372036854775807"}'), (E, b'{"x":"-9223372036854775808"}'), (E, b'{"x":"9223372036854775808"}'),
    (E, b'{"x":" 12"}'), (E, b'{"x":"+12"}'), (E, b'{"x":"12a"}'), (E, b'{"x":""}'), (E, b'{"x":"-007"}'),
    (E, b'{"x":9007199254740993}'), (E, b'{"x":-2.5e3}'), (E, b'{"x":9223372036854775808}'), (E, b'{"x":null}'),
    (E, b'{"x":true}'), (M, b'{"a":1e400,"b":1}'), (M, b'{"a":-0.0,"b":1}'), (M, b'{"a":63863781979156355e-1,"b":1}'),
    (M, b'{"a":9007199254740993,"b":1}'), (M, b'{"a":1.7976931348623157e308,"b":10}'), (M, b'{"a":0.1,"b":3}'),
    (M, b'{"a":"1","b":2}'), (A, b'{"a":1,"a":5,"b":2}'), (A, b'{"A":1,"a":3,"b":2}'), (A, b'{"a":1,"b":2,"c":{"a":9}}'),
    (A, b'{"a":"x","a":5,"b":2}'), (A, b"[1,2]"), (A, b"null"), (A, b'"a"'), (A, b"12"), (A, b"true"), (A, None), (A, b"{}"),
    (X, b'{"a":1,"b":2,"ok":0}'), (X, b'{"a":1,"b":2,"ok":null}'), (X, b'{"ok":false,"b":2.5,"a":-7}'),
    (X, b'{"a":1,"b":1e300,"ok":true}'), (X, b'{"a":1,"b":0.005,"ok":true}'), (S, b'{"s":null}'), (S, b'{"s":5}'),
    (S, b'{"s":""}'), (S, b'{"s":"a\\nb"}'), (S, b'{"s":"\xc3\xa9\xff"}'), (P, None), (P, b"[1,2]"), (P, b'{"x":1}'),
    (A, b'{"a":1e400,"b":"x"}'), (N, b'{"n":"1"}'), (N, b'{"n":{"n":1}}'),
]


def rows():
    out = [("h" if r.hostile else "c", r.method, r.span, r.rid) for r in af.corpus(SEED, ROWS)]
    return out + [("p", m, span, 1000 + k) for k, (m, span) in enumerate(PROBES)]


def main():
    rs = rows()
    replies = oracle.ref_dispatch([ac.request(ac.IDL_METHODS[m][0], span, rid)[0] for _, m, span, rid in rs])
    if replies is None:
        sys.exit("oracle/_ref/ref_dispatch missing: build it with `make -C oracle dispatch` (needs the reference tree)")
    entries = [[cls, m, None if span is None else span.decode("latin-1"), rid, reply.decode("latin-1")]
               for (cls, m, span, rid), reply in zip(rs, replies)]
    s = json.dumps
    text = '{"how":%s,"entries":[' % s(HOW) + ",\n".join(s(e, separators=(",", ":")) for e in entries) + "]}"
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(PATH) and text == open(PATH).read() else 1)
    open(PATH, "w").write(text)
    print("wrote %s: %d entries" % (PATH, len(entries)))


if __name__ == "__main__":
    main()
