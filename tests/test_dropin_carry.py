"""The multi-round device server -- carry -> scan + verify -> unpack -> one D2H of the bodies ->
handlers -> pack, round after round -- against the reference client itself: `client_rpccrc
stress` (the reference client library on librpccrc, 10 user threads) talks to a Python server
that reads with recv(61), so frames really are cut, and keeps every connection's unconsumed
bytes on the device: per round the host uploads only what recv() just returned, to the
carry_slots positions of the next buffer, and frames_carry moves the partial frames in front
of them.  No connection byte comes back to the host except inside a delivered body.

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
from test_dropin_unpack import answer  # noqa: E402

NSLOT = 32   # connections the server holds at once
RECV = 61    # bytes per recv(): less than a request frame


def dev(a, dt):
    return torch.from_numpy(np.array(a, dtype=dt)).cuda()


class DeviceStreams:
    """The connections' bytes, on the device: two buffers used in turn, and per slot the
    connection the last scan walked, what it consumed and whether the slot is to be dropped."""

    def __init__(self):
        self.buf = torch.empty(0, dtype=torch.uint8, device="cuda")
        self.off = self.len = self.used = torch.zeros(NSLOT, dtype=torch.int64, device="cuda")
        self.carried = torch.zeros(1, dtype=torch.int64, device="cuda")

    def round(self, new, drop):
        """new[slot]: the bytes recv() just returned (b"" for none); drop[slot]: 1 for a slot
        whose connection is gone (nothing is carried: the slot is empty afterwards).  Returns
        (bytes to send per slot, closed per slot, frames found, requests answered)."""
        nl = [len(b) for b in new]
        at, total = rpc_amd.carry_slots(nl)
        stage = np.zeros(total, dtype=np.uint8)
        for slot, b in enumerate(new):
            stage[at[slot]:at[slot] + nl[slot]] = np.frombuffer(b, dtype=np.uint8)
        nxt = torch.from_numpy(stage).cuda()  # the round's one upload: new bytes at their slots
        k = rpc_amd.frames_carry(self.buf, self.off, self.len, self.used, dev(drop, np.uint8), nxt, dev(at, np.int64),
                                 new_lengths=dev(nl, np.int64))
        self.carried += k.carried
        r = rpc_amd.frames_scan(nxt, k.next_offsets, k.next_lengths, role="server", verify=True)
        u = rpc_amd.frames_unpack(nxt, r.frame_offsets, r.verdict, role="server", nul=True, conn_first=r.conn_first)
        self.buf, self.off, self.len, self.used = nxt, k.next_offsets, k.next_lengths, r.consumed
        bodies = u.bodies.cpu().numpy().tobytes()  # the one copy of request bytes to the host: what is to be dispatched
        body_at = u.body_offsets.cpu().tolist()
        types = u.reply_types.cpu().numpy().view(np.uint16).tolist()
        replies, roffs, rlens, answered, cur = [], [], [], 0, 0
        for i, t in enumerate(types):
            body = b""
            if t == rpc_amd.RPC_TYPE_DATA:
                body = answer(json.loads(bodies[body_at[i]:bodies.index(0, body_at[i])]))  # the C string up to its NUL
                answered += 1
            roffs.append(cur)
            rlens.append(len(body))
            replies.append(body)
            cur += len(body)
        send = [b""] * NSLOT
        if types:
            p = rpc_amd.frames_pack(dev(np.frombuffer(b"".join(replies) or b"\0", dtype=np.uint8), np.uint8),
                                    dev(roffs, np.int64), dev(rlens, np.int32), types=u.reply_types, versions=u.versions,
                                    conn_first=r.conn_first)
            cbf = p.conn_bytes_first.cpu().tolist()
            wire = p.stream.cpu().numpy().tobytes()
            send = [wire[cbf[s]:cbf[s + 1]] for s in range(NSLOT)]
        return send, [s == rpc_amd.CONN_CLOSED for s in r.state.cpu().tolist()], r.nframes, answered


def carrying_server(port_holder, stop, stats, errors):
    ls = socket.socket()
    ls.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    ls.bind(("127.0.0.1", 0))
    ls.listen(64)
    port_holder.append(ls.getsockname()[1])
    socks = [None] * NSLOT  # slot -> socket
    drop = [0] * NSLOT      # slot -> its device bytes are to be dropped by the next round
    streams = DeviceStreams()

    def gone(slot):
        socks[slot].close()
        socks[slot] = None
        drop[slot] = 1

    try:
        while not stop.is_set():
            free = [s for s in range(NSLOT) if socks[s] is None and not drop[s]]
            ready, _, _ = select.select(([ls] if free else []) + [s for s in socks if s is not None], [], [], 0.2)
            new = [b""] * NSLOT
            for s in ready:
                if s is ls:
                    c, _ = ls.accept()
                    c.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
                    c.settimeout(5)
                    socks[free.pop(0)] = c
                    continue
                slot = socks.index(s)
                try:
                    got = s.recv(RECV)
                except OSError:
                    got = b""
                if not got:
                    gone(slot)
                new[slot] = got
            if not any(new) and not any(drop):
                continue
            send, closed, nframes, answered = streams.round(new, drop)
            stats.append((sum(map(len, new)), nframes, answered, len([x for x in send if x])))
            drop[:] = [0] * NSLOT  # (dropped slots are empty now)
            for slot in range(NSLOT):
                if socks[slot] is None:
                    continue
                shut = closed[slot]
                try:
                    if send[slot]:
                        socks[slot].sendall(send[slot])
                except OSError:
                    shut = True
                if shut:
                    gone(slot)
        stats.append(("carried", int(streams.carried.cpu()[0])))
    except Exception:  # (reported by the test: a daemon thread's traceback is otherwise lost)
        errors.append(traceback.format_exc())
    finally:
        for s in socks:
            if s is not None:
                s.close()
        ls.close()


def test_reference_client_against_the_carrying_device_server():
    """`client_rpccrc stress <port> 10 5`: 50 rounds of add_i32 / echo_i64 / strlen_s from 10
    threads of the reference client, every one answered right, by a server that never sees a
    whole frame in one recv(): partial frames were carried on the device (carried > 0)."""
    port, stop, stats, errors = [], threading.Event(), [], []
    t = threading.Thread(target=carrying_server, args=(port, stop, stats, errors), daemon=True)
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
    assert stats and stats[-1][0] == "carried"
    rounds, carried = stats[:-1], stats[-1][1]
    assert sum(s[2] for s in rounds) >= 150  # three calls per round
    assert carried > 0
    assert max(s[0] for s in rounds) <= NSLOT * RECV  # a round uploads what recv() returned, nothing carried
    assert any(s[1] >= 2 or s[3] > 1 for s in rounds), rounds[:50]
