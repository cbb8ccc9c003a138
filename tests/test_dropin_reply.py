"""The device server round with the reply in it -- scan + verify -> unpack -> route -> one D2H ->
handlers -> reply -> pack -- against the reference client itself: test_dropin_route.py's
server, but the host never writes an envelope.  A handler hands back only the JSON text of its
value; the ids stay on the device, NOT_FOUND and INVALID would be answered there without the
host seeing them, the reply bodies and their offsets are laid out there, and what goes up per
round is the value bytes alone.  A DEFER entry falls back to the old path (the host's whole
reply as a RAW value) and is counted: the reference client's requests are canonical, so the
run must count none."""
import json
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import route_cases as rc  # noqa: E402
from test_dropin_route import HANDLERS  # noqa: E402
from test_dropin_server import _client  # noqa: E402
from test_dropin_unpack import answer, batched_server, dev  # noqa: E402
import test_dropin_unpack  # noqa: E402

COUNTS = {"call": 0, "raw": 0, "value_bytes": 0, "uploaded": 0, "envelopes_on_host": 0, "built": 0}


def replied_round(carry):
    """test_dropin_route.routed_round with the reply between the handlers and the pack."""
    lens = [len(b) for b in carry]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev(np.frombuffer(b"".join(bytes(b) for b in carry), dtype=np.uint8), np.uint8)
    r = rpc_amd.frames_scan(raw, dev(offs, np.int64), dev(lens, np.int64), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, r.frame_offsets, r.verdict, role="server", nul=True, conn_first=r.conn_first)
    table = rpc_amd.route_table(rc.METHODS)
    rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, table, reply_types=u.reply_types)
    bodies = u.bodies.cpu().numpy().tobytes()  # the one copy of request bytes to the host
    at = u.body_offsets.cpu().tolist()
    poff, plen = rt.params_off.cpu().tolist(), rt.params_len.cpu().tolist()
    first = rt.group_first.cpu().tolist()
    order = rt.order.cpu().tolist()[:first[-1]]
    n = len(at)
    nm = table.nmethods
    values, voff, vlen = bytearray(), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    for m in range(nm):  # each handler once, over the array of its requests; it hands back value text
        idx = order[first[m]:first[m + 1]]
        if not idx:
            continue
        params = [json.loads(bodies[at[i] + poff[i]:at[i] + poff[i] + plen[i]]) if plen[i] else {} for i in idx]
        for i, result in zip(idx, HANDLERS[m](params)):
            text = json.dumps(result).encode()
            voff[i], vlen[i] = len(values), len(text)
            values += text
        COUNTS["call"] += len(idx)
    for i in order[first[nm + 2]:first[nm + 3]]:  # outside the strict subset: the old path, as a RAW value
        text = answer(json.loads(bodies[at[i]:bodies.index(0, at[i])]))
        voff[i], vlen[i] = len(values), len(text)
        values += text
        COUNTS["raw"] += 1
        COUNTS["envelopes_on_host"] += 1
    COUNTS["value_bytes"] += int(vlen.sum())
    COUNTS["uploaded"] += len(values)
    up = dev(np.frombuffer(bytes(values) or b"\0", dtype=np.uint8), np.uint8)[:len(values)]
    rp = rpc_amd.frames_reply(rt.kind, rt.id, up, dev(voff, np.int64), dev(vlen, np.int32), reply_types=u.reply_types,
                              conn_first=r.conn_first)
    COUNTS["built"] += int((rp.status != rpc_amd.REPLY_NONE).sum())
    p = rpc_amd.frames_pack(rp.bodies, rp.body_offsets, rp.body_lens, types=rp.types, versions=u.versions,
                            conn_first=r.conn_first)
    cbf = p.conn_bytes_first.cpu().tolist()
    wire = p.stream.cpu().numpy().tobytes()
    send = [wire[cbf[c]:cbf[c + 1]] for c in range(len(carry))]
    return send, r.consumed.cpu().tolist(), [s == rpc_amd.CONN_CLOSED for s in r.state.cpu().tolist()], r.nframes, first[-1]


def test_reference_client_against_the_replying_device_server(monkeypatch):
    """`client_rpccrc stress <port> 10 5` passes 50/50 against the server whose handlers return
    value text only; the run counts zero RAW entries, builds every reply on the device, and
    uploads exactly the sum of the value lengths."""
    monkeypatch.setattr(test_dropin_unpack, "device_round", replied_round)
    for k in COUNTS:
        COUNTS[k] = 0
    port, stop, stats, errors = [], threading.Event(), [], []
    t = threading.Thread(target=batched_server, args=(port, stop, stats, errors), daemon=True)
    t.start()
    while not port and t.is_alive():
        time.sleep(0.05)
    try:
        code, res, err = _client("stress", port[0], 10, 5)
    finally:
        stop.set()
        t.join(timeout=10)
    assert not errors, errors[0]
    assert code == 0 and res == {"success": 50, "failure": 0}, err[-2000:]
    assert COUNTS["raw"] == 0 and COUNTS["envelopes_on_host"] == 0, COUNTS
    assert COUNTS["call"] >= 150 and COUNTS["built"] == COUNTS["call"], COUNTS
    assert sum(s[2] for s in stats) == COUNTS["call"]  # every request was a CALL: none unknown, none invalid
    assert COUNTS["uploaded"] == COUNTS["value_bytes"] > 0, COUNTS
