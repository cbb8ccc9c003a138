"""The frame args' rules against replies the reference's dispatcher recorded
(tests/golden/args_golden.json, written by tests/golden/make_args_golden.py): for an OK row the
reply recomputed from the decoded slots equals the recorded reply byte for byte, an INVALID
row's recorded reply is the -32602 form, a DEFER row claims nothing (args_fuzz.hold).  The
reference prints a double with %1.15g when that reads back within one epsilon, so its replies
pin a decoded double to about 1 ulp only; the bit-exact pin is float() in the rules
(tests/test_args_pow10.py)."""
import json
import os

import pytest

import args_cases as ac
import args_fuzz as af

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    doc = json.load(open(os.path.join(HERE, "golden", "args_golden.json")))
    rows = [af.Row(cls != "c", m, None if span is None else span.encode("latin-1"), rid)
            for cls, m, span, rid, _ in doc["entries"]]
    return doc, rows, [e[4].encode("latin-1") for e in doc["entries"]]


def test_rules_hold_against_the_recorded_replies(golden):
    doc, rows, replies = golden
    buf, entries = af.entries_of(rows)
    layer = ac.args_entries(buf, entries)
    n = af.hold(rows, replies, layer)
    assert len(rows) >= 400 and n[ac.OK] >= 200 and n[ac.INVALID] >= 40 and n[ac.DEFER] >= 40, n
    canon = [r[0] for row, r, e in zip(rows, layer, doc["entries"]) if e[0] == "c"]
    assert len(canon) >= 150 and set(canon) == {ac.OK}
    probes = {(e[1], e[2]): r[0] for r, e in zip(layer, doc["entries"]) if e[0] == "p"}
    assert probes[(ac.A, '{"a":2147483648,"b":1}')] == ac.DEFER and probes[(ac.A, "[1,2]")] == ac.INVALID
    assert probes[(ac.E, '{"x":"12a"}')] == ac.DEFER and probes[(ac.A, '{"A":1,"a":3,"b":2}')] == ac.OK


def test_fixture_is_the_makers_rows(golden):
    """The fixture's requests are the maker's own (its replies are the reference's)."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_args_golden as mk
    finally:
        sys.path.pop(0)
    doc = golden[0]
    assert [(c, m, None if s is None else s.encode("latin-1"), rid) for c, m, s, rid, _ in doc["entries"]] == mk.rows()
    assert doc["how"] == mk.HOW


def test_todays_reference_gives_the_recorded_replies(golden):
    from oracle import oracle
    _, rows, replies = golden
    got = oracle.ref_dispatch(af.bodies_of(rows))
    if got is None:
        pytest.skip("oracle/_ref/ref_dispatch is not built (needs the reference tree)")
    assert got == replies
