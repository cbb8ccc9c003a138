"""The frame results on recorded replies (tests/golden/results_golden.json, written by
tests/golden/make_results_golden.py from the reference's live dispatcher, decoder and cJSON):
the plain rules, the CPU emulator and, in a gpu-marked test, the device, each held to what the
reference's generated client would return.  Needs no reference tree."""
import json
import os

import pytest

import resolve_cases as rv
import results_cases as rs
import results_ref
from test_results_emu import results_emu, run_emu  # noqa: F401  (results_emu: a fixture)
from test_results_fuzz import hold
from test_route_emu import S_SMALL

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    rows = json.load(open(os.path.join(HERE, "golden", "results_golden.json")))

    def node(d):  # (the row format: make_results_golden.py)
        if d is None:
            return results_ref.Node(False, False, False, False, False, 0, 0, None)
        flags, bits, ll, s = d
        return results_ref.Node(True, bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8), int(bits, 16), ll,
                                None if s is None else s.encode("latin-1"))

    return [(t, body.encode("latin-1"), results_ref.Facts(rc, node(a), node(b), node(c))) for t, body, rc, a, b, c in rows]


def as_call(rows):
    """The bodies back to back, each decoded by the resolve's rules and, where it decodes, MATCHED
    to a slot of its own with the row's result type: (buf, entries, pending_method, slot_entry,
    types)."""
    buf, entries, pm, se = bytearray(b"##"), [], [], []
    for t, body, _ in rows:
        row = rv.decode_body(body)
        kind = rv.MATCHED if row[0] == rv.UNKNOWN else row[0]
        if kind == rv.MATCHED:
            se.append(len(entries))
            pm.append(t)
        entries.append((len(buf), len(body), kind, len(pm) - 1 if kind == rv.MATCHED else rv.NO_SLOT, *row[2:]))
        buf += body + b"\0"
    return bytes(buf), entries, pm, se, list(range(5))


def hold_all(rows, answers):
    """Each decoded row's answers against the recorded facts; returns how many were decided."""
    decided = 0
    for (t, body, f), e, r in zip(rows, as_call(rows)[1], answers):
        if e[2] != rv.MATCHED:
            assert r.status == rs.NONE
            continue
        hold(body, t, r, f)
        decided += rs.DEFER not in (r.status, r.error_status)
    return decided


def test_fixture_shape():
    rows = golden()
    assert 380 <= len(rows) <= 460 and {t for t, _, _ in rows} == set(range(5))
    assert os.path.getsize(os.path.join(HERE, "golden", "results_golden.json")) < 1 << 20


def test_rules_on_the_recorded_replies():
    rows = golden()
    buf, entries, pm, se, types = as_call(rows)
    decided = hold_all(rows, rs.results_entries(buf, entries, pm, types))
    print("decided %d of %d" % (decided, len(rows)))
    assert decided >= 250


def test_emulator_on_the_recorded_replies(results_emu):  # noqa: F811
    rows = golden()
    buf, entries, pm, se, types = as_call(rows)
    got, slots, nd = run_emu(results_emu, S_SMALL, 11, buf, entries, pm, se, types)
    want = rs.results_entries(buf, entries, pm, types)
    assert got == want and slots == rs.results_slots(entries, want, se) and nd == rs.ndefer(want)
    hold_all(rows, got)


@pytest.mark.gpu
def test_gpu_on_the_recorded_replies():
    from test_frames_results import check
    rows = golden()
    buf, entries, pm, se, types = as_call(rows)
    hold_all(rows, check(buf, entries, pm, se, types, mis=5, what="golden"))
