"""The fused frame scan (rpc_frames_scan_verify_device) against the reference server
itself: several requests pipelined in one send on one connection, a bad CRC among them.

The reference server binds its hard-coded port without SO_REUSEADDR
(rpc_server_main.c:38), so a second instance cannot start while a connection the first
one closed lingers in TIME_WAIT on that port.  This module therefore (a) sorts before
tests/test_dropin_server.py, whose helpers and ``server`` fixture it imports, and (b)
sends only cases that leave request bytes unread behind the bad frame: the server then
closes with data pending, which resets the connection and leaves no TIME_WAIT behind."""
import socket
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from oracle import oracle  # noqa: E402
from test_dropin_server import PORT, frame, recv_exact, server  # noqa: E402,F401  (server: the fixture)

NREQ = 5


@pytest.mark.parametrize("j", [0, 2, 3])
def test_pipelined_frames_against_reference_server(server, j):  # noqa: F811
    """Five requests in one send, a bad CRC at position j < 4: the reference server
    answers exactly the first j, then closes (rpc_server_main.c:227-233); the fused call
    says j x OK, BAD_CRC, then NOT_REACHED, and the connection ends CLOSED."""
    bodies = [('{"jsonrpc":"2.0","method":"add_i32","params":{"a":%d,"b":2},"id":%d}' % (k, k + 1)).encode()
              for k in range(NREQ)]
    raw = b"".join(frame(b, crc=(oracle.crc32(b) ^ 0x100) if k == j else None) for k, b in enumerate(bodies))
    s = socket.create_connection(("127.0.0.1", PORT), timeout=30)
    s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
    replies = []
    try:
        s.sendall(raw)
        while True:
            hdr = recv_exact(s, 12)
            if len(hdr) < 12:
                break
            _, _, blen, crc = struct.unpack(">HHII", hdr)
            body = recv_exact(s, blen)
            assert len(body) == blen and oracle.crc32(body) == crc
            replies.append(body)
    except ConnectionResetError:  # closed with our bytes unread: an RST instead of a FIN
        pass
    s.close()
    assert len(replies) == j
    assert all(b'"result":%d' % (k + 2) in r for k, r in enumerate(replies))
    d = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    one = lambda v: torch.tensor([v], dtype=torch.int64).cuda()  # noqa: E731
    r = rpc_amd.frames_scan(d, one(0), one(len(raw)), verify=True)
    assert r.verdict.cpu().numpy().tolist() == ([rpc_amd.FRAME_OK] * j + [rpc_amd.FRAME_BAD_CRC]
                                                + [rpc_amd.FRAME_NOT_REACHED] * (NREQ - 1 - j))
    assert r.state.cpu().numpy().tolist() == [rpc_amd.CONN_CLOSED]
    assert r.consumed.cpu().numpy().tolist() == [len(raw)]
