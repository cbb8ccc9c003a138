"""The device server round -- scan + verify -> unpack -> one D2H of the bodies -> handlers ->
pack -- against the reference client itself: `client_rpccrc stress` (the reference client
library on librpccrc, 10 user threads) talks to a Python server whose only per-frame work is
json.loads on the C string the unpack left and building the reply body.  Framing, CRC
verification, body extraction, the PING -> PONG plan, reply headers and reply CRCs all run on
the GPU, batched over every connection that had bytes in the round.

The server listens on an ephemeral port with SO_REUSEADDR (the pattern of
test_dropin_server._bad_crc_server) and stays away from the reference server's port."""
import json
import select
import socket
import threading
import time
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from test_dropin_server import _client  # noqa: E402


def answer(req):
    """The three methods `client_rpccrc stress` calls, in the reply form of
    test_dropin_server._bad_crc_reply."""
    p, m = req["params"], req["method"]
    if m == "add_i32":
        result = int(p["a"]) + int(p["b"])
    elif m == "echo_i64":
        result = str(int(p["x"]))  # (the client's stub takes a string or a number: rpc_client_gen.c echo_i64)
    elif m == "strlen_s":
        result = len(p["s"].encode())
    else:
        raise ValueError(m)
    return json.dumps({"jsonrpc": "2.0", "id": req["id"], "result": result}, separators=(",", ":")).encode()


def dev(a, dt):
    return torch.from_numpy(np.array(a, dtype=dt)).cuda()  # (a copy: np.frombuffer's arrays are read-only)


def device_round(carry):
    """One round over the connections' carried bytes (a list of bytearrays, none empty):
    returns (bytes to send per connection, bytes consumed per connection, closed per
    connection, frames found, requests answered)."""
    lens = [len(b) for b in carry]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev(np.frombuffer(b"".join(bytes(b) for b in carry), dtype=np.uint8), np.uint8)
    r = rpc_amd.frames_scan(raw, dev(offs, np.int64), dev(lens, np.int64), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, r.frame_offsets, r.verdict, role="server", nul=True, conn_first=r.conn_first)
    bodies = u.bodies.cpu().numpy().tobytes()  # the one copy of request bytes to the host: what is to be dispatched
    at = u.body_offsets.cpu().tolist()
    types = u.reply_types.cpu().numpy().view(np.uint16).tolist()
    replies, roffs, rlens, answered = [], [], [], 0
    cur = 0
    for i, t in enumerate(types):
        body = b""
        if t == rpc_amd.RPC_TYPE_DATA:
            body = answer(json.loads(bodies[at[i]:bodies.index(0, at[i])]))  # the C string up to its NUL
            answered += 1
        roffs.append(cur)
        rlens.append(len(body))
        replies.append(body)
        cur += len(body)
    p = rpc_amd.frames_pack(dev(np.frombuffer(b"".join(replies) or b"\0", dtype=np.uint8), np.uint8), dev(roffs, np.int64),
                            dev(rlens, np.int32), types=u.reply_types, versions=u.versions, conn_first=r.conn_first)
    cbf = p.conn_bytes_first.cpu().tolist()
    wire = p.stream.cpu().numpy().tobytes()
    send = [wire[cbf[c]:cbf[c + 1]] for c in range(len(carry))]
    return send, r.consumed.cpu().tolist(), [s == rpc_amd.CONN_CLOSED for s in r.state.cpu().tolist()], r.nframes, answered


def batched_server(port_holder, stop, stats, errors):
    ls = socket.socket()
    ls.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    ls.bind(("127.0.0.1", 0))
    ls.listen(64)
    port_holder.append(ls.getsockname()[1])
    conns = {}  # socket -> carried bytes
    try:
        while not stop.is_set():
            ready, _, _ = select.select([ls] + list(conns), [], [], 0.2)
            for s in ready:
                if s is ls:
                    c, _ = ls.accept()
                    c.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
                    c.settimeout(5)
                    conns[c] = bytearray()
                    continue
                try:
                    got = s.recv(65536)
                except OSError:
                    got = b""
                if not got:
                    s.close()
                    del conns[s]
                else:
                    conns[s] += got
            socks = [s for s, b in conns.items() if b]
            if not socks:
                continue
            send, consumed, closed, nframes, answered = device_round([conns[s] for s in socks])
            stats.append((len([x for x in send if x]), nframes, answered))
            for s, out, used, shut in zip(socks, send, consumed, closed):
                try:
                    if out:
                        s.sendall(out)
                except OSError:
                    shut = True
                del conns[s][:used]
                if shut:
                    s.close()
                    del conns[s]
    except Exception:  # (reported by the test: a daemon thread's traceback is otherwise lost)
        errors.append(traceback.format_exc())
    finally:
        for s in conns:
            s.close()
        ls.close()


def test_reference_client_against_the_batched_device_server():
    """`client_rpccrc stress <port> 10 5`: 50 rounds of add_i32 / echo_i64 / strlen_s from 10
    threads of the reference client, every one answered right; and the run was carried by
    batches: some round held frames of more than one connection, or several frames."""
    port, stop, stats, errors = [], threading.Event(), [], []
    t = threading.Thread(target=batched_server, args=(port, stop, stats, errors), daemon=True)
    t.start()
    while not port and t.is_alive():
        time.sleep(0.05)
    try:
        rc, res, err = _client("stress", port[0], 10, 5)
    finally:
        stop.set()
        t.join(timeout=10)
    assert not errors, errors[0]
    assert rc == 0 and res == {"success": 50, "failure": 0}, err[-2000:]
    assert sum(s[2] for s in stats) >= 150  # three calls per round
    assert any(s[0] > 1 or s[1] >= 2 for s in stats), stats[:50]
