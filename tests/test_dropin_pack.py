"""The frame pack (rpc_frames_pack_device) against the reference server itself: five
requests and a PING, packed on the GPU into one connection's bytes and sent with one
sendall.

The reference server binds its hard-coded port without SO_REUSEADDR
(rpc_server_main.c:38), so no connection may be closed by the server side: it would
linger in TIME_WAIT on that port and keep the next module's server from starting.  This
module therefore sorts before tests/test_dropin_pipelined.py and
tests/test_dropin_server.py, whose helpers and ``server`` fixture it imports, sends only
well-formed frames, reads every reply and then closes from the client."""
import socket
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from oracle import oracle  # noqa: E402
from test_dropin_server import PORT, recv_exact, server  # noqa: E402,F401  (server: the fixture)

NREQ = 5
PING_AFTER = 2


def test_packed_requests_against_reference_server(server):  # noqa: F811
    """Five add_i32 requests with a PING after the second: the reference server answers
    with five replies (right results, valid CRCs) and one PONG, in request order."""
    bodies = [('{"jsonrpc":"2.0","method":"add_i32","params":{"a":%d,"b":2},"id":%d}' % (k, k + 1)).encode()
              for k in range(NREQ)]
    types, offs, lens, at = [], [], [], 0
    for k, b in enumerate(bodies):
        if k == PING_AFTER:
            types.append(rpc_amd.RPC_TYPE_PING)
            offs.append(0)
            lens.append(0)
        types.append(rpc_amd.RPC_TYPE_DATA)
        offs.append(at)
        lens.append(len(b))
        at += len(b)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).cuda()  # noqa: E731
    p = rpc_amd.frames_pack(dev(np.frombuffer(b"".join(bodies), dtype=np.uint8).copy(), np.uint8), dev(offs, np.int64),
                            dev(lens, np.int32), types=dev(types, np.int16), conn_first=dev([0, len(types)], np.int64))
    assert p.verdict.cpu().tolist() == [rpc_amd.FRAME_CONTROL if t else rpc_amd.FRAME_OK for t in types]
    cbf = p.conn_bytes_first.cpu().tolist()
    raw = p.stream.cpu().numpy().tobytes()[cbf[0]:cbf[1]]
    assert len(raw) == p.total == 12 * len(types) + at
    s = socket.create_connection(("127.0.0.1", PORT), timeout=30)
    s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
    got = []
    try:
        s.sendall(raw)
        for _ in types:
            hdr = recv_exact(s, 12)
            assert len(hdr) == 12, got
            ver, typ, blen, crc = struct.unpack(">HHII", hdr)
            body = recv_exact(s, blen)
            assert len(body) == blen
            got.append((typ, crc, body))
    finally:
        s.close()  # every reply has been read: the client closes first
    assert [g[0] for g in got] == [rpc_amd.RPC_TYPE_PONG if t else rpc_amd.RPC_TYPE_DATA for t in types]
    replies = [g for g in got if g[0] == rpc_amd.RPC_TYPE_DATA]
    assert len(replies) == NREQ
    for k, (_, crc, body) in enumerate(replies):
        assert oracle.crc32(body) == crc
        assert b'"result":%d' % (k + 2) in body and b'"id":%d' % (k + 1) in body
    pong = got[PING_AFTER]
    assert pong[1] == 0 and pong[2] == b""
