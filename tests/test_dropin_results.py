"""The batched device client of tests/test_dropin_resolve.py with the results behind the resolve
-- carry -> scan + verify -> unpack -> resolve -> results, round after round -- against the
reference server itself: the same 40 pipelined calls on 8 connections, replies read with
recv(97).  Every completion is read from the per-slot columns; json.loads runs on no result
span, and no round reports a deferred entry.

This module sorts before tests/test_dropin_server.py, whose ``server`` fixture it takes through
test_dropin_resolve, and closes every socket of its own first (see there)."""
import select
import socket
import struct
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from test_dropin_resolve import NCONN, NREQ, RECV, call, dev  # noqa: E402
from test_dropin_server import PORT, frame, server  # noqa: E402,F401  (server: the fixture)

#: the IDL's result types in the order of test_dropin_resolve.call's methods; the unknown method's
#: slot is given method 0 (its reply has no `result`)
RESULTS = ["string", "i64", "i32", "double", "bool", "i32", "string"]


def typed(want):
    """What the value column holds for json.loads' ``want`` (a string: its bytes)."""
    if isinstance(want, bool):
        return int(want)
    if isinstance(want, float):
        return struct.unpack("<Q", struct.pack("<d", want))[0]
    return want.encode() if isinstance(want, str) else want


def test_completions_come_from_the_slot_columns(server, monkeypatch):  # noqa: F811
    import json
    calls = [call(k) for k in range(NCONN * NREQ)]
    monkeypatch.setattr(json, "loads", lambda *a, **k: pytest.fail("json.loads ran"))  # (the calls are built)
    order = np.random.default_rng(5).permutation(len(calls))  # slot s holds call order[s]
    slot_of = np.arange(len(calls))                            # the open slots, as the caller numbers them
    pending = dev([calls[k][1] for k in order], np.uint32).view(torch.int32)
    pending_method = dev([k % 8 % 7 for k in order], np.int16)
    rtypes = rpc_amd.result_types(["m%d" % m for m in range(7)], RESULTS, device="cuda")
    socks = []
    for c in range(NCONN):
        s = socket.create_connection(("127.0.0.1", PORT), timeout=30)
        s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        s.sendall(b"".join(frame(calls[c * NREQ + j][0]) for j in range(NREQ)))
        socks.append(s)
    buf = torch.empty(0, dtype=torch.uint8, device="cuda")
    off = ln = used = torch.zeros(NCONN, dtype=torch.int64, device="cuda")
    done, rounds, ndefer, deadline = {}, 0, 0, time.time() + 30
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
            r = rpc_amd.frames_resolve(u.bodies, u.body_offsets, u.body_lens, pending, reply_types=u.reply_types)
            x = rpc_amd.frames_results(u.bodies, u.body_offsets, u.body_lens, r, pending_method, rtypes)
            # the D2H of columns: one row per pending slot, and the bodies for the strings
            status, value, estatus, ecode, base = (t.cpu().numpy() for t in (x.slot_status, x.slot_value.view(torch.int64),
                                                                              x.slot_error_status, x.slot_error_code,
                                                                              x.slot_str_base))
            ndefer += int(x.ndefer.cpu()[0])
            bodies = u.bodies.cpu().numpy().tobytes()
            methods = pending_method.cpu().numpy()
            for slot in np.flatnonzero(status != rpc_amd.RESULTS_NONE):
                s = int(slot_of[slot])
                assert s not in done
                v = int(value[slot]) & (2**64 - 1)
                if status[slot] == rpc_amd.RESULTS_OK and RESULTS[methods[slot]] == "string":
                    v = bodies[int(base[slot]) + (v & 0xFFFFFFFF):][:v >> 32]
                done[s] = (int(status[slot]), v, int(estatus[slot]), int(ecode[slot]))
            nopen = int(r.nopen.cpu()[0])
            still = r.open[:nopen].to(torch.int64)
            assert nopen == len(calls) - len(done)
            pending, pending_method = pending[still].contiguous(), pending_method[still].contiguous()
            slot_of = slot_of[still.cpu().numpy()]
    finally:
        for s in socks:  # the client closes first
            s.close()
    assert sorted(done) == list(range(len(calls))) and rounds > 1
    assert ndefer == 0
    for s, got in done.items():
        want = calls[order[s]][2]
        if want is None:
            assert got == (rpc_amd.RESULTS_ABSENT, 0, rpc_amd.RESULTS_OK, -32601), (s, got)
        else:
            if order[s] % 8 == 3:  # mul_double's result is a double whatever the product
                want = float(want)
            if order[s] % 8 == 1:  # echo_i64's quoted string is the integer
                want = int(want)
            assert got == (rpc_amd.RESULTS_OK, typed(want), rpc_amd.RESULTS_ABSENT, 0), (s, got, want)
