"""tests/test_dropin_request.py's device client with the params built on the device too -- typed
columns -> values (PARAMS form) -> request -> pack -> send ... recv -> carry -> scan + verify ->
unpack -> resolve -- against the reference server itself: the same 8 connections with 5 calls
pipelined on each.  The host uploads columns of numbers (and the bytes of the strings) and
nothing else; it builds no `params` text and no envelope.

Like test_dropin_request.py this module sorts before tests/test_dropin_server.py, whose ``server``
fixture it imports, and closes every socket of its own first."""
import json
import select
import socket
import struct
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from test_dropin_request import METHODS, NCONN, NREQ, RECV, call, dev  # noqa: E402
from test_dropin_server import PORT, server  # noqa: E402,F401  (server: the fixture)

#: the IDL's parameters per method of test_dropin_request.METHODS (the unknown method has none)
SCHEMA = [("ping", []), ("echo_i64", [("x", "i64")]), ("add_i32", [("a", "i32"), ("b", "i32")]),
          ("mul_double", [("a", "double"), ("b", "double")]), ("is_even", [("n", "i32")]), ("strlen_s", [("s", "string")]),
          ("mix3", [("a", "i32"), ("b", "double"), ("ok", "bool")]), ("no_such_method", [])]
assert [m for m, _ in SCHEMA] == METHODS


def columns(calls):
    """The calls' parameters as typed slots [3, n] and the strings' bytes."""
    slots = np.zeros((3, len(calls)), dtype=np.uint64)
    strings = bytearray()
    for i, c in enumerate(calls):
        params = json.loads(c[1])
        for k, (name, t) in enumerate(SCHEMA[c[0]][1]):
            v = params[name]
            if t == "string":
                slots[k, i] = len(strings) | len(v) << 32
                strings += v.encode()
            elif t == "double":
                slots[k, i] = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
            else:
                slots[k, i] = int(v) & (2**64 - 1)
    return slots, bytes(strings)


def test_device_client_builds_params_from_columns_against_reference_server(server):  # noqa: F811
    calls = [call(k) for k in range(NCONN * NREQ)]
    n = len(calls)
    # the sending half: columns go up, the params objects are built on the device
    slots, strings = columns(calls)
    method = dev([c[0] for c in calls], np.uint16).view(torch.int16)
    v = rpc_amd.frames_values(method, dev(slots.view(np.int64), np.int64), rpc_amd.args_schema(SCHEMA),
                              form=rpc_amd.VALUES_FORM_PARAMS, strings=dev(np.frombuffer(strings, dtype=np.uint8), np.uint8))
    assert v.status.cpu().tolist() == [rpc_amd.VALUES_OK] * n and int(v.ndefer.cpu()[0]) == 0
    assert v.values.cpu().numpy().tobytes() == b"".join(c[1] for c in calls)  # (what json.dumps would have built)
    ids = dev([c[2] for c in calls], np.uint32).view(torch.int32)
    conn = dev([c * NREQ for c in range(NCONN + 1)], np.int64)
    rq = rpc_amd.frames_request(method, ids, v.values, v.value_offsets, v.value_lens, rpc_amd.route_table(METHODS),
                                conn_first=conn)
    assert rq.status.cpu().tolist() == [rpc_amd.REQUEST_CALL] * n
    p = rpc_amd.frames_pack(rq.bodies, rq.body_offsets, rq.body_lens, types=rq.types, conn_first=conn)
    assert p.verdict.cpu().tolist() == [rpc_amd.FRAME_OK] * n
    wire = p.stream.cpu().numpy().tobytes()
    cbf = p.conn_bytes_first.cpu().tolist()
    assert cbf[-1] == len(wire) == rq.total + rpc_amd.RPC_HEADER_LEN * n
    # the receiving half: slot s holds call s, the pending ids are the request's ids
    slot_of = np.arange(n)
    pending = ids
    socks = []
    for c in range(NCONN):
        s = socket.create_connection(("127.0.0.1", PORT), timeout=30)
        s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        s.sendall(wire[cbf[c]:cbf[c + 1]])  # the pack's output, as it is
        socks.append(s)
    buf = torch.empty(0, dtype=torch.uint8, device="cuda")
    off = ln = used = torch.zeros(NCONN, dtype=torch.int64, device="cuda")
    done, kinds, rounds, deadline = {}, [], 0, time.time() + 30
    try:
        while len(done) < n:
            assert time.time() < deadline, (len(done), rounds)
            ready, _, _ = select.select(socks, [], [], 1.0)
            new = [b""] * NCONN
            for s in ready:
                new[socks.index(s)] = s.recv(RECV)
            if not any(new):
                continue
            rounds += 1
            nl = [len(b) for b in new]
            at, total = rpc_amd.carry_slots(nl)
            stage = np.zeros(total, dtype=np.uint8)
            for c, b in enumerate(new):
                stage[at[c]:at[c] + nl[c]] = np.frombuffer(b, dtype=np.uint8)
            nxt = torch.from_numpy(stage).cuda()
            k = rpc_amd.frames_carry(buf, off, ln, used, None, nxt, dev(at, np.int64), new_lengths=dev(nl, np.int64))
            sc = rpc_amd.frames_scan(nxt, k.next_offsets, k.next_lengths, role="client", verify=True)
            u = rpc_amd.frames_unpack(nxt, sc.frame_offsets, sc.verdict, role="client", nul=True, conn_first=sc.conn_first)
            buf, off, ln, used = nxt, k.next_offsets, k.next_lengths, sc.consumed
            assert sc.state.cpu().tolist() == [rpc_amd.CONN_OPEN] * NCONN
            r = rpc_amd.frames_resolve(u.bodies, u.body_offsets, u.body_lens, pending, reply_types=u.reply_types)
            kind = r.kind.cpu().numpy()
            kinds += kind.tolist()
            hit = np.flatnonzero(kind == rpc_amd.RESOLVE_MATCHED)
            if len(hit):
                bodies = u.bodies.cpu().numpy().tobytes()
                base = u.body_offsets.cpu().numpy()
                slot, ro, rl, eo, el = (x.cpu().numpy().view(np.uint32) for x in (r.slot, r.result_off, r.result_len,
                                                                                  r.error_off, r.error_len))
                for i in hit:
                    span = lambda o, m: bodies[int(base[i]) + int(o):int(base[i]) + int(o) + int(m)]  # noqa: E731
                    s = int(slot_of[slot[i]])
                    assert s not in done
                    done[s] = (json.loads(span(ro[i], rl[i])) if rl[i] else None,
                               json.loads(span(eo[i], el[i])) if el[i] else None)
            nopen = int(r.nopen.cpu()[0])
            still = r.open[:nopen].to(torch.int64)
            assert nopen == n - len(done)
            pending, slot_of = pending[still].contiguous(), slot_of[still.cpu().numpy()]
    finally:
        for s in socks:  # the client closes first
            s.close()
    assert sorted(done) == list(range(n)) and rounds > 1
    assert set(kinds) <= {rpc_amd.RESOLVE_NONE, rpc_amd.RESOLVE_MATCHED}  # no DEFER, INVALID, DUPLICATE or UNKNOWN
    assert kinds.count(rpc_amd.RESOLVE_MATCHED) == n
    for s, (result, error) in done.items():
        want = calls[s][3]
        if want is None:
            assert result is None and error["code"] == -32601, (s, error)
        else:
            # (cJSON prints 3.0 as 3: numbers compare by value, a bool stays a bool)
            assert error is None and result == want and isinstance(result, bool) == isinstance(want, bool), (s, result, want)
