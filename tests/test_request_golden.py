"""The frame request against the reference client's own encoder: tests/golden/request_golden.json
holds (name, params text, id) triples and what rpc_codec_encode_request made of each (the params
through cJSON_Parse first).  Every entry whose recorded params print equals the given text, and
whose name needs no escape, must be rebuilt byte for byte from (method index, params span, id);
the names that need an escape read REQUEST_BAD_METHOD; an entry whose params the reference
reprints differently is not rebuilt from the text (the call copies, it does not reprint) and is
only laid out.  And the class c bodies of tests/golden/route_golden.json that the plain rules
route as CALL are rebuilt byte for byte from what the route gives: (method index, params span,
id).  Run on the plain rules, on the CPU emulator, and on the GPU."""
import json
import os

import numpy as np
import pytest

import request_cases as rq
import route_cases as rtc
from test_request_emu import T_K, request_emu, run_emu  # noqa: F401  (request_emu: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


def needs_escape(name):
    return any(c < 0x20 or c in b'"\\' for c in name)


@pytest.fixture(scope="module")
def recorded():
    doc = json.load(open(os.path.join(HERE, "golden", "request_golden.json")))
    assert "rpc_codec_encode_request" in doc["how"]
    lat = lambda s: None if s is None else s.encode("latin-1")  # noqa: E731
    return [(lat(n), lat(p), rid, lat(pr), lat(rq_)) for n, p, rid, pr, rq_ in doc["entries"]]


def case_of(recorded):
    names = []
    for name, *_ in recorded:
        if name not in names:
            names.append(name)
    table = rq.make_table(names)
    params, ents = bytearray(b"~"), []
    for name, text, rid, _, _ in recorded:
        ents.append((rq.DATA, names.index(name), rid, len(params), len(text or b"")))
        params += (text or b"") + b"~"
    return rq.Case("golden", bytes(params), table, ents, [0, len(ents)], typed=False)


def hold(recorded, offs, lens, status, out):
    rebuilt = escaped = 0
    for (name, text, rid, printed, request), at, ln, st in zip(recorded, offs, lens, status):
        if needs_escape(name):
            assert (st, ln) == (rq.Q_BAD_METHOD, 0), name
            escaped += 1
        elif printed == text:
            assert st == rq.Q_CALL and out[at:at + ln] == request, (name, text, rid)
            rebuilt += 1
        else:  # (the text goes out as given: the same request up to how the params are printed)
            assert st == rq.Q_CALL and json.loads(out[at:at + ln]) == json.loads(request), (name, text, rid)
    assert rebuilt >= 60 and escaped >= 4 and rebuilt + escaped < len(recorded)
    ids = {rid for (_, _, rid, _, _) in recorded}
    assert ids >= {0, 9, 10, 2147483648, 4294967295}
    assert any(text is None and not needs_escape(name) for name, text, *_ in recorded)
    assert any(name == b"" for name, *_ in recorded) and any(max(name, default=0) >= 0x80 for name, *_ in recorded)


def test_rules_rebuild_the_recorded_requests(recorded):
    want = rq.want_of(case_of(recorded), None)
    hold(recorded, want.body_offsets, want.body_lens, want.status, want.out)


@pytest.mark.parametrize("tile,src_mis,out_mis", [(T_K, 0, 0), (256, 7, 9)])
def test_emulator_rebuilds_the_recorded_requests(request_emu, recorded, tile, src_mis, out_mis):  # noqa: F811
    total, rows, conn, out = run_emu(request_emu, tile, src_mis, out_mis, case_of(recorded), None)
    hold(recorded, [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], out)
    assert conn == [0, total]


# ---- the route's recorded bodies, back from what the route gives ---------------------------------
@pytest.fixture(scope="module")
def routed_calls():
    doc = json.load(open(os.path.join(HERE, "golden", "route_golden.json")))
    assert [m.encode() for m in doc["methods"]] == rtc.METHODS
    bodies = [body.encode("latin-1") for cls, body, _ in doc["entries"] if cls == "c"]
    calls = [(b, rtc.route_body(b)) for b in bodies]
    calls = [(b, r) for b, r in calls if r[0] == rtc.CALL]
    assert len(calls) >= 25
    return calls


def route_case(routed_calls):
    """The bodies back to back are the params buffer: each entry's value is its own span."""
    buf, entries = rtc.back_to_back([b for b, _ in routed_calls])
    ents = [(rq.DATA, m, rid, off + po if pl else 0, pl) for (off, _), (_, (_, m, rid, po, pl)) in zip(entries, routed_calls)]
    return rq.Case("routed", buf, rq.make_table(rtc.METHODS), ents, [0, len(ents)], typed=False)


def hold_routed(routed_calls, offs, lens, status, out):
    for (body, _), at, ln, st in zip(routed_calls, offs, lens, status):
        assert st == rq.Q_CALL and out[at:at + ln] == body, body
    assert any(b'"params"' not in b for b, _ in routed_calls)


def test_rules_rebuild_the_routes_recorded_calls(routed_calls):
    want = rq.want_of(route_case(routed_calls), None)
    hold_routed(routed_calls, want.body_offsets, want.body_lens, want.status, want.out)


def test_emulator_rebuilds_the_routes_recorded_calls(request_emu, routed_calls):  # noqa: F811
    total, rows, conn, out = run_emu(request_emu, 256, 3, 5, route_case(routed_calls), None)
    hold_routed(routed_calls, [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], out)


@pytest.mark.gpu
def test_gpu_rebuilds_the_recorded_requests(recorded, routed_calls):
    import rpc_amd
    from test_frames_request import dev_table, entry_tensors
    from test_frames_unpack import dev_bytes, host
    for case, check, fixture in ((case_of(recorded), hold, recorded), (route_case(routed_calls), hold_routed, routed_calls)):
        _, method, rid, poff, plen = entry_tensors(case)
        r = rpc_amd.frames_request(method, rid, dev_bytes(case.params, 5), poff, plen, dev_table(case.table))
        check(fixture, host(r.body_offsets, np.uint64), host(r.body_lens, np.uint32), host(r.status, np.uint8),
              r.bodies.cpu().numpy().tobytes())
