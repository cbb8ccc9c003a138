"""The frame values against replies the reference's dispatcher recorded
(tests/golden/values_golden.json, written by tests/golden/make_values_golden.py): each row's
typed result, formatted and wrapped by the reply's rule, is the recorded reply byte for byte --
on the plain rules, on the CPU emulator and on the GPU, so that the reference's bytes reach the
device test too."""
import json
import os

import pytest

import args_cases as ac
import values_cases as vc
import values_fuzz as vf
from test_values_emu import run_emu, values_emu  # noqa: F401  (values_emu: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    doc = json.load(open(os.path.join(HERE, "golden", "values_golden.json")))
    rows = [vf.Row(m, None if span is None else span.encode("latin-1"), rid, int(slot)) for m, span, rid, slot, _ in doc["entries"]]
    return doc, rows, doc["strings"].encode("latin-1"), [e[4].encode("latin-1") for e in doc["entries"]]


def test_rules_hold_against_the_recorded_replies(golden):
    _, rows, strings, replies = golden
    types, entries = vf.entries_of(rows)
    layer = [vc.values_entry(e, vc.FORM_RESULT, ac.IDL, types, 1, strings, b"") for e in entries]
    n = vf.hold(rows, replies, layer, strings)
    assert len(rows) >= 400 and n[vc.OK] >= 380 and n[vc.DEFER] >= 2, n
    assert {r.method for r in rows} == set(range(7))


def test_emulator_holds_against_the_recorded_replies(golden, values_emu):  # noqa: F811
    _, rows, strings, replies = golden
    types, entries = vf.entries_of(rows)
    got, out, _, _ = run_emu(values_emu, entries, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, texts=b"", tile=256,
                             mis=(5, 0, 11))
    vf.hold(rows, replies, [(r[0], out[r[2]:r[2] + r[3]]) for r in got], strings)


@pytest.mark.gpu
def test_gpu_holds_against_the_recorded_replies(golden):
    """values -> reply on the device gives the recorded replies themselves."""
    import numpy as np
    import rpc_amd
    from test_frames_unpack import dev_bytes, to_dev
    from test_frames_values import dev_form, dev_inputs
    _, rows, strings, replies = golden
    types, entries = vf.entries_of(rows)
    method, slots, _, _, _, _, _ = dev_inputs(entries, 1)
    v = rpc_amd.frames_values(method, slots, dev_form(vc.FORM_RESULT, ac.IDL, types), strings=dev_bytes(strings, 3))
    st = v.status.cpu().numpy().tolist()
    off, ln = v.value_offsets.cpu().numpy().tolist(), v.value_lens.cpu().numpy().tolist()
    out = v.values.cpu().numpy().tobytes()
    vf.hold(rows, replies, [(s, out[o:o + k]) for s, o, k in zip(st, off, ln)], strings)
    r = rpc_amd.frames_reply(None, to_dev(np.array([r.rid for r in rows], dtype=np.uint32).view(np.int32)), v.values,
                             v.value_offsets, v.value_lens, status=v.reply_status)
    bodies = r.bodies.cpu().numpy().tobytes()
    bo, bl = r.body_offsets.cpu().numpy().tolist(), r.body_lens.cpu().numpy().tolist()
    for row, s, o, k, reply in zip(rows, st, bo, bl, replies):
        if s == vc.OK:
            assert bodies[o:o + k] == reply, row
        else:
            assert b'"code":-32603' in bodies[o:o + k], row


def test_fixture_is_the_makers_rows(golden):
    """The fixture's requests are the maker's own (its replies are the reference's)."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_values_golden as mk
    finally:
        sys.path.pop(0)
    doc, rows, strings, _ = golden
    want_rows, want_strings = mk.rows()
    assert rows == want_rows and strings == want_strings and doc["how"] == mk.HOW


def test_todays_reference_gives_the_recorded_replies(golden):
    from oracle import oracle
    _, rows, _, replies = golden
    got = oracle.ref_dispatch(vf.bodies_of(rows))
    if got is None:
        pytest.skip("oracle/_ref/ref_dispatch is not built (needs the reference tree)")
    assert got == replies
