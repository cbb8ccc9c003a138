"""The device server round with the route in it -- scan + verify -> unpack -> route -> one D2H ->
handlers -> pack -- against the reference client itself: test_dropin_unpack.py's server, but
the host never parses an envelope.  The handlers run once per group over d_order; json.loads
sees only the `params` span of CALL entries; NOT_FOUND and INVALID are answered from d_id; a
DEFER entry falls back to the old path (json.loads on the C string) and is counted: the
reference client's requests are canonical, so the run must count none."""
import json
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import route_cases as rc  # noqa: E402
from test_dropin_server import _client  # noqa: E402
from test_dropin_unpack import answer, batched_server, dev  # noqa: E402
import test_dropin_unpack  # noqa: E402

#: one handler per method of the table, each over the list of its requests' params
HANDLERS = [
    lambda ps: ["pong" for _ in ps],                                              # ping
    lambda ps: [str(int(p["x"])) for p in ps],                                   # echo_i64
    lambda ps: [int(p["a"]) + int(p["b"]) for p in ps],                          # add_i32
    lambda ps: [float(p["a"]) * float(p["b"]) for p in ps],                      # mul_double
    lambda ps: [int(p["n"]) % 2 == 0 for p in ps],                               # is_even
    lambda ps: [len(p["s"].encode()) for p in ps],                               # strlen_s
    lambda ps: ["%d:%g:%s" % (p["a"], p["b"], "true" if p["ok"] else "false") for p in ps],  # mix3
]
COUNTS = {"call": 0, "deferred": 0, "params_bytes": 0, "groups_run": 0}


def reply(rid, **kw):
    return json.dumps({"jsonrpc": "2.0", "id": rid, **kw}, separators=(",", ":")).encode()


def routed_round(carry):
    """test_dropin_unpack.device_round with the route between the unpack and the handlers."""
    lens = [len(b) for b in carry]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev(np.frombuffer(b"".join(bytes(b) for b in carry), dtype=np.uint8), np.uint8)
    r = rpc_amd.frames_scan(raw, dev(offs, np.int64), dev(lens, np.int64), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, r.frame_offsets, r.verdict, role="server", nul=True, conn_first=r.conn_first)
    table = rpc_amd.route_table(rc.METHODS)
    rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, table, reply_types=u.reply_types)
    bodies = u.bodies.cpu().numpy().tobytes()  # the one copy of request bytes to the host
    at = u.body_offsets.cpu().tolist()
    rid = rt.id.cpu().numpy().view(np.uint32).tolist()
    poff, plen = rt.params_off.cpu().tolist(), rt.params_len.cpu().tolist()
    first = rt.group_first.cpu().tolist()
    order = rt.order.cpu().tolist()[:first[-1]]
    n = len(at)
    replies = [b""] * n
    nm = table.nmethods
    for m in range(nm):  # each handler once, over the array of its requests
        idx = order[first[m]:first[m + 1]]
        if not idx:
            continue
        params = [json.loads(bodies[at[i] + poff[i]:at[i] + poff[i] + plen[i]]) if plen[i] else {} for i in idx]
        COUNTS["params_bytes"] += sum(plen[i] for i in idx)
        COUNTS["groups_run"] += 1
        for i, result in zip(idx, HANDLERS[m](params)):
            replies[i] = reply(rid[i], result=result)
        COUNTS["call"] += len(idx)
    for i in order[first[nm]:first[nm + 1]]:
        replies[i] = reply(rid[i], error={"code": -32601, "message": "Method not found"})
    for i in order[first[nm + 1]:first[nm + 2]]:
        replies[i] = reply(rid[i], error={"code": -32600, "message": "Invalid Request"})
    for i in order[first[nm + 2]:first[nm + 3]]:  # outside the strict subset: the old path
        replies[i] = answer(json.loads(bodies[at[i]:bodies.index(0, at[i])]))
        COUNTS["deferred"] += 1
    answered = first[-1]
    rlens = [len(b) for b in replies]
    roffs = np.concatenate([[0], np.cumsum(rlens[:-1])]).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    p = rpc_amd.frames_pack(dev(np.frombuffer(b"".join(replies) or b"\0", dtype=np.uint8), np.uint8), dev(roffs, np.int64),
                            dev(rlens, np.int32), types=u.reply_types, versions=u.versions, conn_first=r.conn_first)
    cbf = p.conn_bytes_first.cpu().tolist()
    wire = p.stream.cpu().numpy().tobytes()
    send = [wire[cbf[c]:cbf[c + 1]] for c in range(len(carry))]
    return send, r.consumed.cpu().tolist(), [s == rpc_amd.CONN_CLOSED for s in r.state.cpu().tolist()], r.nframes, answered


def test_reference_client_against_the_routed_device_server(monkeypatch):
    """`client_rpccrc stress <port> 10 5` passes 50/50 against the server whose handlers run per
    group; the run counts zero deferred entries and at least 150 CALLs."""
    monkeypatch.setattr(test_dropin_unpack, "device_round", routed_round)
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
    assert COUNTS["deferred"] == 0, COUNTS
    assert COUNTS["call"] >= 150, COUNTS
    assert sum(s[2] for s in stats) == COUNTS["call"]  # every request was a CALL: none unknown, none invalid
    assert COUNTS["params_bytes"] > 0 and COUNTS["groups_run"] <= 3 * len(stats)
