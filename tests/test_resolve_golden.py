"""The frame resolve against the reference client's own decoder, as recorded in
tests/golden/resolve_golden.json (rpc_codec_decode_response behind tests/dropin/ref_decode.c;
tests/golden/make_resolve_golden.py writes it).  Class c is what a client receives: the 153 reply
strings of route_golden.json; none may defer, and a result or error span equals the reference's
own unformatted print of that member byte for byte.  Class h is the hostile case table.  Wherever
the rules do not defer, kind, id and the presence of each member are the reference's, and a
recorded -1 never reads MATCHED, UNKNOWN or DUPLICATE.  The rules, the emulator and the GPU are
each held against the recording."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import resolve_cases as rc
import resolve_ref
from test_resolve_emu import S_K, S_SMALL, resolve_emu, run_emu  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = json.load(open(os.path.join(HERE, "golden", "resolve_golden.json")))["entries"]
BODIES = [e[1].encode("latin-1") for e in ENTRIES]
DECODED = (rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE)


def golden_call():
    """Every recorded body in one call; the pending table holds every third recorded id."""
    buf, offs, lens = rc.pack_bodies(BODIES, nul=1)
    ids = sorted({e[3] for e in ENTRIES if e[2] == 0})
    return rc.Call(buf, offs, lens, None, ids[::3] + [0xFFFFFFFE])


def hold(got, what):
    """got: a Resolved over golden_call()."""
    decoded_h = accepted_h = 0
    for i, (cls, _, code, rid, res, err) in enumerate(ENTRIES):
        b, kind = BODIES[i], got.kind[i]
        where = (what, i, b[:80], rc.KIND_NAMES[kind])
        if cls == "c":
            assert kind != rc.DEFER, where
        if cls == "h" and code == 0:
            accepted_h += 1
            decoded_h += kind in DECODED
        if code == -1:
            assert kind not in DECODED, where
        if kind == rc.DEFER:
            continue
        if kind == rc.INVALID:
            assert code == -1, where
            continue
        assert kind in DECODED and code == 0 and got.id[i] == rid, where
        assert (got.result_len[i] > 0) == (res is not None) and (got.error_len[i] > 0) == (err is not None), where
        if cls == "c":  # cJSON printed these bodies: the spans are its print of the member
            if res is not None:
                assert b[got.result_off[i]:got.result_off[i] + got.result_len[i]] == res.encode("latin-1"), where
            if err is not None:
                assert b[got.error_off[i]:got.error_off[i] + got.error_len[i]] == err.encode("latin-1"), where
    assert 2 * decoded_h >= accepted_h > 0, (what, decoded_h, accepted_h)  # deferring cannot hide a failure


def test_fixture_shape():
    assert sum(1 for e in ENTRIES if e[0] == "c") == 153 and 0 < sum(1 for e in ENTRIES if e[0] == "h") <= 400
    route = json.load(open(os.path.join(HERE, "golden", "route_golden.json")))["entries"]
    assert [e[1] for e in ENTRIES if e[0] == "c"] == [r[2] for r in route]
    assert [e[1].encode("latin-1") for e in ENTRIES if e[0] == "h"] == [rc.CASES[k] for k in sorted(rc.CASES)]
    assert {e[2] for e in ENTRIES} == {0, -1}


def test_class_c_is_strict_with_digit_ids_and_no_backslash_keys():
    """Why none of the 153 may defer: checked on today's fixture."""
    for e, b in zip(ENTRIES, BODIES):
        if e[0] != "c":
            continue
        members = rc.Strict(b).members
        assert not any(kesc for _, kesc, *_ in members)
        ids = [m for m in members if m[0].lower() == b"id"]
        assert ids and ids[0][2] == "number" and b[ids[0][3]:ids[0][4]].isdigit() and int(b[ids[0][3]:ids[0][4]]) < 2**32


def test_rules_against_the_recording():
    hold(golden_call().expect(), "rules")


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 9)])
def test_emulator_against_the_recording(resolve_emu, stage, mis):  # noqa: F811
    for descending in (False, True):
        hold(run_emu(resolve_emu, stage, mis, golden_call(), descending), "emulator")


@pytest.mark.gpu
def test_gpu_against_the_recording():
    torch = pytest.importorskip("torch")
    import rpc_amd
    call = golden_call()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    r = rpc_amd.frames_resolve(dev(np.frombuffer(call.buf, dtype=np.uint8).copy()),
                               dev(np.array(call.offs, dtype=np.uint64).view(np.int64)),
                               dev(np.array(call.lens, dtype=np.uint32).view(np.int32)),
                               dev(np.array(call.pending, dtype=np.uint32).view(np.int32)))
    torch.cuda.synchronize()
    u32 = lambda x: x.cpu().numpy().view(np.uint32).tolist()  # noqa: E731
    got = rc.Resolved(r.kind.cpu().numpy().tolist(), u32(r.id), u32(r.result_off), u32(r.result_len), u32(r.error_off),
                      u32(r.error_len), u32(r.slot), u32(r.slot_entry), u32(r.open)[:int(r.nopen.cpu()[0])])
    hold(got, "gpu")
    want = call.expect()
    assert got == want


def test_recording_is_todays_reference(tmp_path):
    """Where the reference tree is present: the generator would write the same file."""
    if resolve_ref.build(tmp_path) is None:
        pytest.skip("the reference tree is absent")
    p = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_resolve_golden.py"), "--check"])
    assert p.returncode == 0
