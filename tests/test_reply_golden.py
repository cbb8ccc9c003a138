"""The frame reply against the reference's own dispatcher: tests/golden/route_golden.json holds
bodies and the replies rpc_server_dispatch gave for them.  For each recorded body the route's
kind and id (route_cases.route_body on the CPU layers, the device route on the GPU) and what a
handler would hand back -- the value cut from the recorded reply between `"result":` and the
final `}`, or the recorded error code as the status; for a deferred body the whole recorded
reply as a RAW value -- go through the reply, and the built body must be the recorded string
byte for byte, for every entry.  So that RAW cannot hide everything, at least 100 entries must
be built in the result or the error form.  (-32603 is not in the fixture: its text comes from
the reference's source and is held by the case table only.)  Run on the plain rules, on the
CPU emulator, and on the GPU."""
import json
import os

import numpy as np
import pytest

import reply_cases as rp
import route_cases as rc
from test_reply_emu import T_K, reply_emu, run_emu  # noqa: F401  (reply_emu: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
RESULT = b'"result":'


@pytest.fixture(scope="module")
def recorded():
    doc = json.load(open(os.path.join(HERE, "golden", "route_golden.json")))
    assert [m.encode() for m in doc["methods"]] == rc.METHODS and "rpc_server_dispatch" in doc["how"]
    return [(body.encode("latin-1"), reply.encode("latin-1")) for _, body, reply in doc["entries"]]


def case_of(recorded, routed):
    """The reply's inputs from (kind, id) rows of a route and the recorded replies."""
    values, ents = bytearray(b"~"), []
    for (body, reply), (kind, rid) in zip(recorded, routed):
        status, value = 0, b""
        if kind == rc.DEFER:
            value = reply
        elif kind == rc.CALL:
            doc = json.loads(reply)
            if "error" in doc:
                status = doc["error"]["code"]
            else:
                assert reply.endswith(b"}") and reply.count(RESULT) >= 1
                value = reply[reply.index(RESULT) + len(RESULT):-1]
        ents.append((rp.DATA, kind, rid, status, len(values), len(value)))
        values += value
    return rp.Case("golden", bytes(values), ents, [0, len(ents)], typed=False)


def hold(recorded, case, offs, lens, status, out):
    assert len(recorded) == len(case.entries) == 153
    for (body, reply), at, ln, e in zip(recorded, offs, lens, case.entries):
        assert out[at:at + ln] == reply, (body, e)
    formed = [s for s in status if s in (rp.R_RESULT, rp.R_ERROR)]
    assert len(formed) >= 100 and set(status) <= {rp.R_RESULT, rp.R_ERROR, rp.R_RAW}, len(formed)
    built = {rp.R_RESULT: 0, -32602: 0, -32600: 0, -32601: 0}
    for s, ln, at in zip(status, lens, offs):
        if s == rp.R_RESULT:
            built[rp.R_RESULT] += 1
        elif s == rp.R_ERROR:
            built[json.loads(out[at:at + ln])["error"]["code"]] += 1
    assert built == {rp.R_RESULT: 48, -32602: 13, -32600: 27, -32601: 17}


def test_rules_build_the_recorded_replies(recorded):
    case = case_of(recorded, [rc.route_body(b)[0:3:2] for b, _ in recorded])
    want = rp.want_of(case, None)
    hold(recorded, case, want.body_offsets, want.body_lens, want.status, want.out)


@pytest.mark.parametrize("tile,src_mis,out_mis", [(T_K, 0, 0), (256, 7, 9)])
def test_emulator_builds_the_recorded_replies(reply_emu, recorded, tile, src_mis, out_mis):  # noqa: F811
    case = case_of(recorded, [rc.route_body(b)[0:3:2] for b, _ in recorded])
    total, rows, conn, out = run_emu(reply_emu, tile, src_mis, out_mis, case, None)
    hold(recorded, case, [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], out)
    assert conn == [0, total]


@pytest.mark.gpu
def test_gpu_builds_the_recorded_replies(recorded):
    import torch
    import rpc_amd
    from test_frames_reply import entry_tensors
    from test_frames_unpack import dev_bytes, host, i64, to_dev
    buf, entries = rc.back_to_back([b for b, _ in recorded])
    off, ln = zip(*entries)
    rt = rpc_amd.frames_route(dev_bytes(buf), i64(off), to_dev(np.asarray(ln, dtype=np.int32)),
                              rpc_amd.route_table(rc.METHODS), group=False)
    torch.cuda.synchronize()
    routed = list(zip(host(rt.kind, np.uint8), host(rt.id, np.uint32)))
    case = case_of(recorded, routed)
    _, _, _, st, voff, vlen = entry_tensors(case)
    r = rpc_amd.frames_reply(rt.kind, rt.id, dev_bytes(case.values, 5), voff, vlen, status=st)  # the route's own outputs
    hold(recorded, case, host(r.body_offsets, np.uint64), host(r.body_lens, np.uint32), host(r.status, np.uint8),
         r.bodies.cpu().numpy().tobytes())
