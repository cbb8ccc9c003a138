"""The frame route against the reference's own dispatcher: tests/golden/route_golden.json holds
bodies and the replies rpc_server_dispatch gave for them (its "how" field says how it was
recorded).  Wherever the route does not defer, its kind must be the one the recorded reply
implies and its id the reply's; a body the reference called a parse error must defer.  Two
conditions keep the comparison from being empty: no canonical body defers, and at least half
of the hostile class is routed.  Run on the CPU emulator, and on the GPU.  The recording can be
made again: tests/golden/make_route_golden.py writes the fixture from its own bodies with the
kept driver (oracle/ref_dispatch.c), and a test here asks today's reference for every recorded
reply."""
import json
import os
import subprocess
import sys

import pytest

import route_cases as rc
from test_route_emu import S_K, S_SMALL, route_emu, run_emu  # noqa: F401  (route_emu: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def replies():
    doc = json.load(open(os.path.join(HERE, "golden", "route_golden.json")))
    assert [m.encode() for m in doc["methods"]] == rc.METHODS and "rpc_server_dispatch" in doc["how"]
    assert len(doc["entries"]) <= 2000  # (a few hundred: the classes below, not the count, are what is needed)
    return [(cls, h.encode("latin-1"), json.loads(reply)) for cls, h, reply in doc["entries"]]


def implied(reply):
    """(kind, id) a recorded reply implies; kind None for a parse error."""
    if "error" in reply:
        code = reply["error"]["code"]
        kind = {-32601: rc.NOT_FOUND, -32600: rc.INVALID, -32602: rc.CALL, -32603: rc.CALL, -32700: None}[code]
    else:
        assert "result" in reply
        kind = rc.CALL
    return kind, reply["id"]


def hold_against_replies(replies, rows):
    canon_deferred, hostile, hostile_routed, parse_errors = [], 0, 0, 0
    for (cls, body, reply), row in zip(replies, rows):
        kind, rid = implied(reply)
        hostile += cls == "h"
        if kind is None:
            parse_errors += 1
            assert row[0] == rc.DEFER, (body, reply, row)
        if row[0] == rc.DEFER:
            if cls == "c":
                canon_deferred.append(body)
            continue
        hostile_routed += cls == "h"
        assert row[0] == kind and row[2] == rid, (body, reply, row)
    assert not canon_deferred, canon_deferred[:3]
    assert parse_errors >= 20 and hostile >= 90
    assert 2 * hostile_routed >= hostile, (hostile_routed, hostile)


def test_fixture_classes(replies):
    """The canonical class holds every method, unknown methods, missing and wrong-type methods
    and the ids 0, 4294967295 and 4294967296; the replies hold every error code."""
    canon = [(b, r) for c, b, r in replies if c == "c"]
    assert len(canon) >= 40
    for m in rc.METHODS:
        assert any(b'"method":"%s"' % m in b for b, _ in canon)
    for rid in (0, 4294967295, 4294967296):
        assert any(b.endswith(b'"id":%d}' % rid) for b, _ in canon)
    assert any(b'"method":5' in b for b, _ in canon) and any(b'"method"' not in b for b, _ in canon)
    codes = {r["error"]["code"] for _, _, r in replies if "error" in r}
    assert codes >= {-32700, -32600, -32601, -32602}


def test_todays_reference_gives_every_recorded_reply():
    """The fixture is what oracle/_ref/ref_dispatch answers today, reply for reply and byte for
    byte, and the generator beside it would write the file as it stands."""
    from route_fuzz import reference
    doc = json.load(open(os.path.join(HERE, "golden", "route_golden.json")))
    assert len(doc["entries"]) == 153 and "oracle/ref_dispatch.c" in doc["how"]
    today = reference([body.encode("latin-1") for _, body, _ in doc["entries"]])
    for (_, body, reply), now in zip(doc["entries"], today):
        assert now == reply.encode("latin-1"), (body, reply, now)
    made = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_route_golden.py"), "--check"])
    assert made.returncode == 0


def test_rules_agree_with_the_reference(replies):
    hold_against_replies(replies, [rc.route_body(b) for _, b, _ in replies])


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 9)])
def test_emulator_agrees_with_the_reference(route_emu, replies, stage, mis):  # noqa: F811
    buf, entries = rc.back_to_back([b for _, b, _ in replies])
    rows, _, _ = run_emu(route_emu, stage, mis, buf, entries, None, rc.IDL)
    hold_against_replies(replies, rows)


@pytest.mark.gpu
def test_gpu_agrees_with_the_reference(replies):
    from test_frames_route import gpu_route
    buf, entries = rc.back_to_back([b for _, b, _ in replies])
    rows, _, _ = gpu_route(buf, entries, None, rc.IDL)
    hold_against_replies(replies, rows)
