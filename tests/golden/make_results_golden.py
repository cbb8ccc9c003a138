#!/usr/bin/env python3
"""Writes tests/golden/results_golden.json: about 400 recorded rows of (reply body, result type,
what the reference's decoder and cJSON say about its `result` and its `error`'s `code` and
`message`), for tests/test_results_golden.py.  Needs the reference tree (oracle/_ref/ref_dispatch
and tests/results_ref.py's driver); the fixture holds recorded data only.

The rows: 200 replies of the reference's live dispatcher to tests/values_fuzz.py's requests, 140
of them mutated as tests/test_results_fuzz.py mutates, and the hand-written members of
tests/results_cases.py's table wrapped as replies.

  python tests/golden/make_results_golden.py
"""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import results_cases as rs  # noqa: E402
import results_ref  # noqa: E402
import test_results_fuzz as tf  # noqa: E402


def main():
    types, replies = tf.replies_of(0xC3753)
    rng = random.Random(0x601D)
    picks = rng.sample(range(len(replies)), 340)
    rows = [(types[k], replies[k]) for k in picks[:200]] + [(types[k], tf.mutate(rng, replies[k])) for k in picks[200:]]
    rows += [(t, rs.reply(k, r, e)[0]) for k, (_, t, r, e, *_) in enumerate(rs.CASES)]
    with tempfile.TemporaryDirectory() as d:
        facts = results_ref.run(results_ref.build(d), [b for _, b in rows])
    # One row per line: [type, body, rc, result, code, message]; a node that is not there is null,
    # one that is [is_string | is_number << 1 | is_bool << 2 | is_true << 3, valuedouble's bits in
    # hex, strtoll, valuestring or null].  Bytes are written as latin-1 text.
    def node(n):
        if not n.there:
            assert n == results_ref.Node(False, False, False, False, False, 0, 0, None)
            return None
        flags = n.is_string | n.is_number << 1 | n.is_bool << 2 | n.is_true << 3
        return [flags, "%x" % n.bits, n.strtoll, None if n.string is None else n.string.decode("latin-1")]

    out = [[t, b.decode("latin-1"), f.rc, node(f.result), node(f.code), node(f.message)] for (t, b), f in zip(rows, facts)]
    with open(os.path.join(HERE, "results_golden.json"), "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in out) + "\n]\n")
    print(len(out), "rows")


if __name__ == "__main__":
    main()
