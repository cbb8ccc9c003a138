"""The batched device client -- carry -> scan + verify -> unpack -> resolve, round after round --
against the reference server itself: 8 connections, 5 requests pipelined on each (the IDL's seven
methods and one unknown method, 40 distinct ids), replies read with recv(97) so that frames
really are cut and several rounds are needed.  The pending table lives on the device and shrinks
to the round's open slots; json.loads runs on result and error spans only.

The reference server binds its hard-coded port without SO_REUSEADDR (rpc_server_main.c:38), so
this module (a) sorts before tests/test_dropin_server.py, whose helpers and ``server`` fixture it
imports, and (b) closes every socket of its own first: the TIME_WAIT stays on the client's
ephemeral ports."""
import json
import select
import socket
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from test_dropin_server import PORT, frame, server  # noqa: E402,F401  (server: the fixture)

NCONN, NREQ = 8, 5
RECV = 97  # bytes per recv(): frames are cut


def dev(a, dt):
    return torch.from_numpy(np.array(a, dtype=dt)).cuda()


def call(k):
    """Request k of the 40: (body, what json.loads of the result span gives, or None for the
    unknown method)."""
    m = k % 8
    method, params, want = [
        ("ping", {}, "pong"),
        ("echo_i64", {"x": str(10**12 + k)}, str(10**12 + k)),
        ("add_i32", {"a": k, "b": 2}, k + 2),
        ("mul_double", {"a": 1.5, "b": k}, 1.5 * k),
        ("is_even", {"n": k}, k % 2 == 0),
        ("strlen_s", {"s": "x" * k}, k),
        ("mix3", {"a": k, "b": 2.5, "ok": True}, "a=%d,b=2.50,ok=true" % k),
        ("no_such_method", {}, None),
    ][m]
    rid = 1000003 * (k + 1) % 2**32
    body = json.dumps({"jsonrpc": "2.0", "method": method, "params": params, "id": rid}, separators=(",", ":")).encode()
    return body, rid, want


def test_batched_client_against_reference_server(server):  # noqa: F811
    calls = [call(k) for k in range(NCONN * NREQ)]
    order = np.random.default_rng(5).permutation(len(calls))  # slot s holds call order[s]
    slot_of = np.arange(len(calls))                            # the open slots, as the caller numbers them
    pending = dev([calls[k][1] for k in order], np.uint32).view(torch.int32)
    socks = []
    for c in range(NCONN):
        s = socket.create_connection(("127.0.0.1", PORT), timeout=30)
        s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        s.sendall(b"".join(frame(calls[c * NREQ + j][0]) for j in range(NREQ)))
        socks.append(s)
    buf = torch.empty(0, dtype=torch.uint8, device="cuda")
    off = ln = used = torch.zeros(NCONN, dtype=torch.int64, device="cuda")
    done, kinds, rounds, deadline = {}, [], 0, time.time() + 30
    try:
        while len(done) < len(calls):
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
                    span = lambda o, n: bodies[int(base[i]) + int(o):int(base[i]) + int(o) + int(n)]  # noqa: E731
                    s = int(slot_of[slot[i]])
                    assert s not in done
                    done[s] = (json.loads(span(ro[i], rl[i])) if rl[i] else None,
                               json.loads(span(eo[i], el[i])) if el[i] else None)
            nopen = int(r.nopen.cpu()[0])
            still = r.open[:nopen].to(torch.int64)
            assert nopen == len(calls) - len(done)
            pending, slot_of = pending[still].contiguous(), slot_of[still.cpu().numpy()]
    finally:
        for s in socks:  # the client closes first
            s.close()
    assert sorted(done) == list(range(len(calls))) and rounds > 1
    assert set(kinds) <= {rpc_amd.RESOLVE_NONE, rpc_amd.RESOLVE_MATCHED}  # no DEFER, INVALID, DUPLICATE or UNKNOWN
    assert kinds.count(rpc_amd.RESOLVE_MATCHED) == len(calls)
    for s, (result, error) in done.items():
        want = calls[order[s]][2]
        if want is None:
            assert result is None and error["code"] == -32601, (s, error)
        else:
            # (cJSON prints 3.0 as 3: numbers compare by value, a bool stays a bool)
            assert error is None and result == want and isinstance(result, bool) == isinstance(want, bool), (s, result, want)
