"""The device server round with the args in it -- scan + verify -> unpack -> route -> args -> one
D2H of columns -> handlers -> pack -- against the reference client itself:
test_dropin_route.py's server, but the host parses no `params` either.  The handlers run once per
group over the columns of `slots`; INVALID entries are answered -32602 without the host looking
at them; json.loads runs on DEFER entries only, and those are counted: the reference client's
requests are canonical, so the run must count none."""
import json
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import args_cases as ac  # noqa: E402
import route_cases as rc  # noqa: E402
from test_dropin_route import HANDLERS as PARSED_HANDLERS, reply  # noqa: E402
from test_dropin_server import _client  # noqa: E402
from test_dropin_unpack import answer, batched_server, dev  # noqa: E402
import test_dropin_unpack  # noqa: E402

METHODS = [(name.decode(), [(p.decode(), t) for p, t in params]) for name, params in ac.IDL_METHODS]
#: one handler per method, each over the columns of its requests (numpy arrays; `f` reads a
#: column as doubles)
HANDLERS = [
    lambda c, f, n: ["pong"] * n,                                                        # ping
    lambda c, f, n: [str(x) for x in c[0].tolist()],                                   # echo_i64
    lambda c, f, n: (c[0] + c[1]).tolist(),                                            # add_i32
    lambda c, f, n: (f(c[0]) * f(c[1])).tolist(),                                      # mul_double
    lambda c, f, n: (c[0] % 2 == 0).tolist(),                                          # is_even
    lambda c, f, n: (c[0] >> 32).tolist(),                                             # strlen_s: the STR slot's length
    lambda c, f, n: ["%d:%g:%s" % (a, b, "true" if ok else "false")
                     for a, b, ok in zip(c[0].tolist(), f(c[1]).tolist(), c[2].tolist())],  # mix3
]
COUNTS = {"call": 0, "decoded": 0, "deferred": 0, "invalid": 0, "groups_run": 0}


def args_round(carry):
    """test_dropin_route.routed_round with the args between the route and the handlers."""
    lens = [len(b) for b in carry]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev(np.frombuffer(b"".join(bytes(b) for b in carry), dtype=np.uint8), np.uint8)
    r = rpc_amd.frames_scan(raw, dev(offs, np.int64), dev(lens, np.int64), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, r.frame_offsets, r.verdict, role="server", nul=True, conn_first=r.conn_first)
    table = rpc_amd.route_table([m for m, _ in METHODS])
    schema = rpc_amd.args_schema(METHODS)
    rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, table, reply_types=u.reply_types)
    ar = rpc_amd.frames_args(u.bodies, u.body_offsets, u.body_lens, rt, schema)
    slots = ar.slots.cpu().numpy()  # the one copy of parameters to the host: [width, n] int64
    status = ar.status.cpu().numpy()
    rid = rt.id.cpu().numpy().view(np.uint32).tolist()
    first = rt.group_first.cpu().tolist()
    order = rt.order.cpu().numpy()[:first[-1]]
    n = len(rid)
    replies = [b""] * n
    nm = table.nmethods
    as_double = lambda col: col.view(np.float64)  # noqa: E731
    deferred = np.flatnonzero(status == rpc_amd.ARGS_DEFER)
    for m in range(nm):  # each handler once, over the columns of its requests
        idx = order[first[m]:first[m + 1]]
        idx = idx[status[idx] == rpc_amd.ARGS_OK]
        if not len(idx):
            continue
        cols = np.ascontiguousarray(slots[:, idx])
        COUNTS["groups_run"] += 1
        for i, result in zip(idx.tolist(), HANDLERS[m](cols, as_double, len(idx))):
            replies[i] = reply(rid[i], result=result)
        COUNTS["decoded"] += len(idx)
    COUNTS["call"] += first[nm]
    for i in np.flatnonzero(status == rpc_amd.ARGS_INVALID).tolist():  # decided on the device
        replies[i] = reply(rid[i], error={"code": -32602, "message": "Invalid params"})
        COUNTS["invalid"] += 1
    if len(deferred) or first[nm + 2] != first[nm + 3]:  # outside a strict subset: the old paths
        bodies = u.bodies.cpu().numpy().tobytes()
        at = u.body_offsets.cpu().tolist()
        method = rt.method.cpu().tolist()
        poff, plen = rt.params_off.cpu().tolist(), rt.params_len.cpu().tolist()
        for i in deferred.tolist():
            params = json.loads(bodies[at[i] + poff[i]:at[i] + poff[i] + plen[i]])
            replies[i] = reply(rid[i], result=PARSED_HANDLERS[method[i]]([params])[0])
            COUNTS["deferred"] += 1
        for i in order[first[nm + 2]:first[nm + 3]].tolist():
            replies[i] = answer(json.loads(bodies[at[i]:bodies.index(0, at[i])]))
            COUNTS["deferred"] += 1
    for i in order[first[nm]:first[nm + 1]].tolist():
        replies[i] = reply(rid[i], error={"code": -32601, "message": "Method not found"})
    for i in order[first[nm + 1]:first[nm + 2]].tolist():
        replies[i] = reply(rid[i], error={"code": -32600, "message": "Invalid Request"})
    answered = first[-1]
    rlens = [len(b) for b in replies]
    roffs = np.concatenate([[0], np.cumsum(rlens[:-1])]).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    p = rpc_amd.frames_pack(dev(np.frombuffer(b"".join(replies) or b"\0", dtype=np.uint8), np.uint8), dev(roffs, np.int64),
                            dev(rlens, np.int32), types=u.reply_types, versions=u.versions, conn_first=r.conn_first)
    cbf = p.conn_bytes_first.cpu().tolist()
    wire = p.stream.cpu().numpy().tobytes()
    send = [wire[cbf[c]:cbf[c + 1]] for c in range(len(carry))]
    return send, r.consumed.cpu().tolist(), [s == rpc_amd.CONN_CLOSED for s in r.state.cpu().tolist()], r.nframes, answered


def test_reference_client_against_the_args_device_server(monkeypatch):
    """`client_rpccrc stress <port> 10 5` passes 50/50 against the server whose handlers read
    columns; the run counts zero deferred and zero invalid entries, and every CALL decoded."""
    monkeypatch.setattr(test_dropin_unpack, "device_round", args_round)
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
    assert COUNTS["deferred"] == 0 and COUNTS["invalid"] == 0, COUNTS
    assert COUNTS["call"] >= 150 and COUNTS["decoded"] == COUNTS["call"], COUNTS
    assert sum(s[2] for s in stats) == COUNTS["call"]  # every request was a CALL: none unknown, none invalid
    assert COUNTS["groups_run"] <= 3 * len(stats)


def test_invalid_params_are_answered_without_the_host():
    """One round on wire bytes built here: the -32602 group is answered from the status alone,
    a DEFER entry goes through json.loads, the others through the columns."""
    import scan_cases as sc
    reqs = [b'{"jsonrpc":"2.0","method":"add_i32","params":{"a":2,"b":40},"id":1}',
            b'{"jsonrpc":"2.0","method":"add_i32","params":{"a":2},"id":2}',
            b'{"jsonrpc":"2.0","method":"strlen_s","params":{"s":"a\\nb"},"id":3}',
            b'{"jsonrpc":"2.0","method":"echo_i64","params":{"x":"-9223372036854775808"},"id":4}',
            b'{"jsonrpc":"2.0","method":"mul_double","params":[1,2],"id":5}',
            b'{"jsonrpc":"2.0","method":"nope","id":6}']
    for k in COUNTS:
        COUNTS[k] = 0
    send, consumed, closed, nframes, answered = args_round([b"".join(sc.frame(b) for b in reqs)])
    want = [reply(1, result=42), reply(2, error={"code": -32602, "message": "Invalid params"}), reply(3, result=3),
            reply(4, result="-9223372036854775808"), reply(5, error={"code": -32602, "message": "Invalid params"}),
            reply(6, error={"code": -32601, "message": "Method not found"})]
    assert send == [b"".join(sc.frame(b) for b in want)]
    assert (nframes, answered, closed) == (6, 6, [False])
    assert COUNTS == {"call": 5, "decoded": 2, "deferred": 1, "invalid": 2, "groups_run": 2}
