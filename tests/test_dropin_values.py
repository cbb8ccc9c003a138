"""The device server round with the values in it -- scan + verify -> unpack -> route -> args -> one
D2H of columns -> handlers -> one H2D of columns -> values -> reply -> pack -- against the
reference client itself: tests/test_dropin_args.py's server, but the host formats no result and
writes no envelope either.  A handler reads numpy columns and returns one numpy column of typed
64-bit slots (mix3 and ping, whose results are strings, return the string's bytes and a STR
slot); the values' DEFER entries are counted, and the reference client's run must count none."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import args_cases as ac  # noqa: E402
from test_dropin_route import reply  # noqa: E402
from test_dropin_server import _client  # noqa: E402
from test_dropin_unpack import batched_server, dev  # noqa: E402
import test_dropin_unpack  # noqa: E402

METHODS = [(name.decode(), [(p.decode(), t) for p, t in params]) for name, params in ac.IDL_METHODS]
RESULTS = ["string", "i64", "i32", "double", "bool", "i32", "string"]
COUNTS = {"call": 0, "formatted_on_device": 0, "values_deferred": 0, "args_deferred": 0, "invalid": 0}


def handlers(m, c, strings):
    """Method m over the columns c of its requests: one column of result slots (uint64).  A string
    result appends its bytes to `strings` and returns offset | length << 32."""
    f = lambda col: col.view(np.float64)  # noqa: E731
    u = lambda col: np.asarray(col, dtype=np.int64).view(np.uint64)  # noqa: E731
    n = c.shape[1]
    if m == 0:
        at = len(strings)
        strings += b"pong"
        return np.full(n, at | 4 << 32, dtype=np.uint64)
    if m == 1:
        return u(c[0])
    if m == 2:
        return u(c[0] + c[1])
    if m == 3:
        return (f(c[0]) * f(c[1])).view(np.uint64)
    if m == 4:
        return u(c[0] % 2 == 0)
    if m == 5:
        return u(c[0] >> 32)
    out = np.empty(n, dtype=np.uint64)
    for j, (a, b, ok) in enumerate(zip(c[0].tolist(), f(c[1]).tolist(), c[2].tolist())):
        t = ("a=%d,b=%.2f,ok=%s" % (a, b, "true" if ok else "false")).encode()
        out[j] = len(strings) | len(t) << 32
        strings += t
    return out


def values_round(carry):
    lens = [len(b) for b in carry]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev(np.frombuffer(b"".join(bytes(b) for b in carry), dtype=np.uint8), np.uint8)
    r = rpc_amd.frames_scan(raw, dev(offs, np.int64), dev(lens, np.int64), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, r.frame_offsets, r.verdict, role="server", nul=True, conn_first=r.conn_first)
    names = [m for m, _ in METHODS]
    table = rpc_amd.route_table(names)
    rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, table, reply_types=u.reply_types)
    ar = rpc_amd.frames_args(u.bodies, u.body_offsets, u.body_lens, rt, rpc_amd.args_schema(METHODS))
    slots = ar.slots.cpu().numpy()  # the one copy of parameters to the host
    status = ar.status.cpu().numpy()
    first = rt.group_first.cpu().tolist()
    order = rt.order.cpu().numpy()[:first[-1]]
    n = status.shape[0]
    nm = table.nmethods
    result = np.zeros(n, dtype=np.uint64)
    strings = bytearray()
    for m in range(nm):  # each handler once, over the columns of its requests
        idx = order[first[m]:first[m + 1]]
        idx = idx[status[idx] == rpc_amd.ARGS_OK]
        if len(idx):
            result[idx] = handlers(m, np.ascontiguousarray(slots[:, idx]), strings)
    COUNTS["call"] += first[nm]
    COUNTS["args_deferred"] += int((status == rpc_amd.ARGS_DEFER).sum()) + first[nm + 3] - first[nm + 2]
    COUNTS["invalid"] += int((status == rpc_amd.ARGS_INVALID).sum())
    # the one copy of results to the device: a column of slots and the strings' bytes
    v = rpc_amd.frames_values(rt.method, dev(result.view(np.int64).reshape(1, n), np.int64),
                              rpc_amd.result_types(names, RESULTS), status=ar.reply_status,
                              strings=dev(np.frombuffer(bytes(strings) or b"\0", dtype=np.uint8), np.uint8))
    vs = v.status.cpu().numpy()
    COUNTS["values_deferred"] += int((vs == rpc_amd.VALUES_DEFER).sum())
    COUNTS["formatted_on_device"] += int((vs == rpc_amd.VALUES_OK).sum())
    rp = rpc_amd.frames_reply(rt.kind, rt.id, v.values, v.value_offsets, v.value_lens, status=v.reply_status,
                              reply_types=u.reply_types, conn_first=r.conn_first)
    p = rpc_amd.frames_pack(rp.bodies, rp.body_offsets, rp.body_lens, types=rp.types, versions=u.versions,
                            conn_first=r.conn_first)
    cbf = p.conn_bytes_first.cpu().tolist()
    wire = p.stream.cpu().numpy().tobytes()
    send = [wire[cbf[c]:cbf[c + 1]] for c in range(len(carry))]
    return send, r.consumed.cpu().tolist(), [s == rpc_amd.CONN_CLOSED for s in r.state.cpu().tolist()], r.nframes, first[-1]


def test_reference_client_against_the_values_device_server(monkeypatch):
    """`client_rpccrc stress <port> 10 5` passes 50/50 against the server whose handlers return
    columns; every CALL's result is formatted on the device and no entry defers."""
    monkeypatch.setattr(test_dropin_unpack, "device_round", values_round)
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
    print("drop-in values:", COUNTS)
    assert COUNTS["values_deferred"] == 0 and COUNTS["args_deferred"] == 0 and COUNTS["invalid"] == 0, COUNTS
    assert COUNTS["call"] >= 150 and COUNTS["formatted_on_device"] == COUNTS["call"], COUNTS


def test_one_round_of_wire_bytes():
    """One round on wire bytes built here: results of every type from columns, a -32602 decided
    by the args, an unknown method, and a subnormal product that the values defer (it answers
    -32603 unless the host formats it)."""
    import scan_cases as sc
    reqs = [b'{"jsonrpc":"2.0","method":"add_i32","params":{"a":2,"b":40},"id":1}',
            b'{"jsonrpc":"2.0","method":"add_i32","params":{"a":2},"id":2}',
            b'{"jsonrpc":"2.0","method":"mul_double","params":{"a":0.1,"b":3},"id":3}',
            b'{"jsonrpc":"2.0","method":"echo_i64","params":{"x":"-9223372036854775808"},"id":4}',
            b'{"jsonrpc":"2.0","method":"mix3","params":{"a":7,"b":2.5,"ok":true},"id":5}',
            b'{"jsonrpc":"2.0","method":"nope","id":6}',
            b'{"jsonrpc":"2.0","method":"is_even","params":{"n":7},"id":7}',
            b'{"jsonrpc":"2.0","method":"ping","id":8}',
            b'{"jsonrpc":"2.0","method":"mul_double","params":{"a":1e-300,"b":1e-10},"id":9}',
            b'{"jsonrpc":"2.0","method":"strlen_s","params":{"s":"four"},"id":10}']
    for k in COUNTS:
        COUNTS[k] = 0
    send, consumed, closed, nframes, answered = values_round([b"".join(sc.frame(b) for b in reqs)])
    want = [reply(1, result=42), reply(2, error={"code": -32602, "message": "Invalid params"}),
            b'{"jsonrpc":"2.0","id":3,"result":0.3}', reply(4, result="-9223372036854775808"),
            reply(5, result="a=7,b=2.50,ok=true"), reply(6, error={"code": -32601, "message": "Method not found"}),
            reply(7, result=False), reply(8, result="pong"), reply(9, error={"code": -32603, "message": "Internal error"}),
            reply(10, result=4)]
    assert send == [b"".join(sc.frame(b) for b in want)]
    assert (nframes, answered, closed) == (10, 10, [False])
    assert COUNTS == {"call": 9, "formatted_on_device": 7, "values_deferred": 1, "args_deferred": 0, "invalid": 1}
