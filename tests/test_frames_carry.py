"""Frame carry on the GPU (rpc_frames_carry_device): partial frames join the
next read.  Against the plain Python rules of tests/carry_cases.py byte for byte and word for
word, and -- carry -> scan + verify -> unpack, round after round on the device -- against one
scan + verify + unpack over the whole streams."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import carry_cases as cc  # noqa: E402
import scan_cases as sc  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARRY_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_carry.h")
GUARD = 64


def kernel_constant(name):
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(CARRY_H).read())
    assert m, f"{name} not found in {CARRY_H}"
    return int(m.group(1))


SHORT_ROOM = kernel_constant("kCarryShortRoom")
LONG_ROOM = SHORT_ROOM + 16  # the smallest room (a multiple of 16) that takes the long route
ROOMS = [rpc_amd.CARRY_ROOM, LONG_ROOM]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bytes(blob, mis=0):
    """blob on the device, its first byte mis bytes past a 16-byte boundary."""
    a = np.zeros(mis + len(blob), dtype=np.uint8)
    a[mis:] = np.frombuffer(bytes(blob), dtype=np.uint8)
    return to_dev(a)[mis:]


def i64(a):
    return to_dev(np.array([int(x) for x in a], dtype=np.uint64).view(np.int64))


def u8(a):
    return to_dev(np.asarray(a, dtype=np.uint8))


def host(t, dtype):
    return t.cpu().numpy().view(dtype).tolist()


def case_tensors(case):
    off, ln, used, state = zip(*case.conns)
    return (i64(off), i64(ln), i64(used), u8(state) if case.use_state else None, i64(case.next_at),
            None if case.new_len is None else i64(case.new_len))


def same(want, big, lead, off, ln, status, carried, what):
    """The next buffer byte for byte (FILL outside every written tail, the guard bytes on both
    sides included) and every word."""
    got = big.cpu().numpy()
    nb = len(want.next)
    assert (got[:lead] == cc.FILL).all() and (got[lead + nb:] == cc.FILL).all(), what
    assert got[lead:lead + nb].tobytes() == want.next, what
    assert host(off, np.uint64) == want.next_off, what
    assert host(ln, np.uint64) == want.next_len, what
    assert host(status, np.uint8) == want.status, what
    assert host(carried, np.uint64) == [want.carried], what


def guarded_next(case, next_mis):
    big = torch.full((GUARD + next_mis + case.next_bytes + GUARD,), cc.FILL, dtype=torch.uint8, device=DEV)
    nxt = big[GUARD + next_mis:GUARD + next_mis + case.next_bytes]
    assert nxt.data_ptr() % 16 == next_mis
    return big, nxt


def carry_into_guarded(case, src_mis=0, next_mis=0):
    want = cc.want_of(case)
    big, nxt = guarded_next(case, next_mis)
    off, ln, used, state, at, nl = case_tensors(case)
    stream = dev_bytes(case.stream, src_mis)
    assert stream.data_ptr() % 16 == src_mis
    r = rpc_amd.frames_carry(stream, off, ln, used, state, nxt, at, room=case.room, new_lengths=nl)
    same(want, big, GUARD + next_mis, r.next_offsets, r.next_lengths, r.status, r.carried,
         (case.name, case.room, src_mis, next_mis))
    assert host(off, np.uint64) == [c[0] for c in case.conns]  # the inputs are left alone
    return want


# ---- 1. the table ---------------------------------------------------------------

@pytest.mark.parametrize("room", ROOMS)
@pytest.mark.parametrize("src_mis,next_mis", [(0, 0), (5, 9)])
def test_case_table(src_mis, next_mis, room):
    """The emulator's table (tests/test_carry_emu.py) on both routes: every (source mod 16,
    destination mod 16) pair at tails of 0 .. 1035 bytes, 3584 connections; every byte of the
    pre-filled next buffer outside the written tails is unchanged."""
    case = cc.table_case(room)
    want = carry_into_guarded(case, src_mis, next_mis)
    assert len(case.conns) == 16 * 16 * len(cc.TABLE_TAILS) == 3584 and set(want.status) == {cc.OK}
    pairs = {((off + used) % 16, no % 16, ln - used) for (off, ln, used, _), no in zip(case.conns, want.next_off)}
    assert pairs == {(s, d, t) for s in range(16) for d in range(16) for t in cc.TABLE_TAILS}


@pytest.mark.parametrize("room", ROOMS)
@pytest.mark.parametrize("use_state", [True, False])
def test_contract_corners_table(room, use_state):
    """The emulator's corners: the stream's and the next buffer's edges, tail == room and one
    more, 64-bit wrap, closed connections with garbage words, with and without a state array."""
    case, names = cc.corner_case(room)
    want = carry_into_guarded(case._replace(use_state=use_state), 3, 7)
    assert set(want.status) == {cc.OK, cc.INVALID, cc.NO_ROOM} | ({cc.CLOSED} if use_state else set())


def test_long_tails_in_chunks():
    """The long route's chunking at the kernel's chunk: tails of chunk - 1, chunk, chunk + 1 and
    3 chunks + 5 bytes at odd offsets, ending anywhere in a chunk."""
    chunk = kernel_constant("kCarryChunk")
    case = cc.long_case(chunk, cc.long_tails(chunk), 4 * chunk)
    want = carry_into_guarded(case, 9, 13)
    assert set(want.status) == {cc.OK} and want.carried == sum(cc.long_tails(chunk))


# ---- 2. rounds equal one shot -----------------------------------------------------

def entries_by_conn(u, conn_first):
    """Per connection, the delivered entries and heartbeats in order: (body, version, reply type)."""
    bodies = u.bodies.cpu().numpy().tobytes()
    at, ln = host(u.body_offsets, np.uint64), host(u.body_lens, np.uint32)
    ty, ver, v = host(u.reply_types, np.uint16), host(u.versions, np.uint16), host(u.verdict, np.uint8)
    first = host(conn_first, np.uint64)
    return [[(bodies[at[i]:at[i] + ln[i]], ver[i], ty[i]) for i in range(first[c], first[c + 1])
             if v[i] in (rpc_amd.FRAME_OK, rpc_amd.FRAME_CONTROL)] for c in range(len(first) - 1)]


def one_shot(conns, role, lift_cap=False, seed=5):
    blob, offs, lens = sc.layout(np.random.default_rng(seed), conns)
    buf = dev_bytes(blob)
    r = rpc_amd.frames_scan(buf, i64(offs), i64(lens), role=role, lift_cap=lift_cap, verify=True)
    u = rpc_amd.frames_unpack(buf, r.frame_offsets, r.verdict, role=role, lift_cap=lift_cap, nul=False,
                              conn_first=r.conn_first)
    return entries_by_conn(u, r.conn_first), host(r.state, np.uint8)


def run_rounds(deliveries, role, lift_cap=False, room=rpc_amd.CARRY_ROOM, stream=None, copy_stream=None):
    """The multi-round loop with the streams on the device, double-buffered: per round the new
    bytes alone go up, to their carry_slots positions; then carry, scan + verify, unpack.  A
    connection that was closed in any round stays closed (the host's sticky flag).  Every
    round's carry is checked against the plain rules on the device's own inputs.  Returns the
    entries per connection over all rounds, the final flags and each round's plain result.
    With ``stream`` and ``copy_stream`` (two side streams) each round's H2D goes to the next
    buffer on ``copy_stream`` from pinned memory, ``stream`` waits on an event recorded behind
    that copy, and carry, scan + verify and unpack run on ``stream``; the host waits for
    ``stream`` before it looks at a result."""
    assert (stream is None) == (copy_stream is None)

    def settle():
        if stream is not None:
            stream.synchronize()

    nconn = len(deliveries)
    cur = torch.empty(0, dtype=torch.uint8, device=DEV)
    off = ln = used = i64([0] * nconn)
    sticky = u8([sc.OPEN] * nconn)
    got, wants = [[] for _ in range(nconn)], []
    for rnd in range(len(deliveries[0])):
        nl = [len(d[rnd]) for d in deliveries]
        at, total = rpc_amd.carry_slots(nl, room=room)
        stage = np.full(total, cc.FILL, dtype=np.uint8)
        for c, d in enumerate(deliveries):
            stage[at[c]:at[c] + nl[c]] = np.frombuffer(d[rnd], dtype=np.uint8)
        case = cc.Case("round %d" % rnd, cur.cpu().numpy().tobytes(),
                       list(zip(host(off, np.uint64), host(ln, np.uint64), host(used, np.uint64), host(sticky, np.uint8))),
                       total, at.tolist(), nl, room)
        want = cc.want_of(case)
        if stream is None:
            nxt = to_dev(stage)  # the round's one H2D: new bytes (and headroom) only
        else:
            pinned = torch.from_numpy(stage).pin_memory()
            nxt = torch.empty(total, dtype=torch.uint8, device=DEV)
            with torch.cuda.stream(copy_stream):
                nxt.copy_(pinned, non_blocking=True)
            up = torch.cuda.Event()
            up.record(copy_stream)
            stream.wait_event(up)  # (the copy fills the headroom too: the carry writes behind it)
        k = rpc_amd.frames_carry(cur, off, ln, used, sticky, nxt, i64(at), room=room, new_lengths=i64(nl), stream=stream)
        settle()
        plain = np.frombuffer(want.next, dtype=np.uint8).copy()
        for c in range(nconn):
            plain[at[c]:at[c] + nl[c]] = stage[at[c]:at[c] + nl[c]]  # (the plain rules know nothing of the new bytes)
        assert nxt.cpu().numpy().tobytes() == plain.tobytes(), rnd
        assert host(k.next_offsets, np.uint64) == want.next_off and host(k.next_lengths, np.uint64) == want.next_len, rnd
        assert host(k.status, np.uint8) == want.status and host(k.carried, np.uint64) == [want.carried], rnd
        s = rpc_amd.frames_scan(nxt, k.next_offsets, k.next_lengths, role=role, lift_cap=lift_cap, verify=True,
                                stream=stream)
        u = rpc_amd.frames_unpack(nxt, s.frame_offsets, s.verdict, role=role, lift_cap=lift_cap, nul=False,
                                  conn_first=s.conn_first, stream=stream)
        settle()
        for c, e in enumerate(entries_by_conn(u, s.conn_first)):
            got[c] += e
        sticky = torch.maximum(sticky, s.state)
        cur, off, ln, used = nxt, k.next_offsets, k.next_lengths, s.consumed
        wants.append(want)
    return got, host(sticky, np.uint8), wants


def cut_six(conn, role, pattern, after=0):
    """Six deliveries of conn with the forced cuts: inside a header, inside a body, exactly on
    a frame boundary, a 1-byte delivery and an empty one (pattern 1: the empty one first)."""
    frames, consumed, _ = sc.walk(conn, 0, len(conn), role)
    control = sc.PING if role == "server" else sc.PONG
    data = []
    for p in frames:
        typ, bl = struct.unpack_from(">HI", conn, p + 2)
        if p >= after and typ != control and 2 <= bl <= sc.MAX_BODY and p + sc.HDR + bl <= consumed:
            data.append((p, bl))
    assert len(data) >= 3
    h, b, e = data[0][0] + 5, data[1][0] + sc.HDR + data[1][1] // 2, data[2][0]
    assert 0 < h < b < e < e + 1 <= len(conn)
    cuts = [h, b, e, e + 1, e + 1] if pattern == 0 else [0, h, b, e, e + 1]
    bounds = [0] + cuts + [len(conn)]
    return [conn[bounds[i]:bounds[i + 1]] for i in range(6)]


@pytest.mark.parametrize("role,side_streams", [pytest.param("server", False, id="server"),
                                               pytest.param("client", False, id="client"),
                                               pytest.param("server", True, id="server-side_streams"),
                                               pytest.param("client", True, id="client-side_streams")])
def test_rounds_equal_one_shot(role, side_streams):
    """48 connections of about 6 KiB with all four endings, each cut into 6 deliveries: the
    entries delivered over the rounds, in order, and the final open / closed state are those of
    one scan + verify + unpack over the whole streams; nothing is delivered after a close; and
    in some round at least half of the connections carry a non-empty tail.  With side streams
    the rounds run on a stream of their own and each round's upload on a second one."""
    rng = np.random.default_rng(0xCA221 + (role == "client"))
    conns = [sc.random_conn(rng, 6000, role, ending=sc.ENDINGS[i % 4]) for i in range(48)]
    after = [0] * 48
    if role == "server":  # a mid-stream frame with a wrong CRC, early: every later delivery carries bytes
        body = sc.rand_body(rng, 100)
        head = sc.filler(rng, 600, role) + sc.frame(body, crc=zlib.crc32(body) ^ 1)
        conns[5] = head + sc.filler(rng, 5400, role)
        after[5] = len(head)
    deliveries = [cut_six(c, role, i % 2, after[i]) for i, c in enumerate(conns)]
    for d, c in zip(deliveries, conns):
        assert b"".join(d) == c
    assert {len(x) for d in deliveries for x in d} >= {0, 1}
    want_entries, want_state = one_shot(conns, role)
    streams = {}
    if side_streams:
        streams = {"stream": torch.cuda.Stream(device=DEV), "copy_stream": torch.cuda.Stream(device=DEV)}
    got, state, wants = run_rounds(deliveries, role, **streams)
    assert state == want_state and {sc.OPEN, sc.CLOSED} == set(state)
    for c in range(48):
        assert got[c] == want_entries[c], c
    assert sum(map(len, got)) > 48 * 5
    if role == "server":
        assert state[5] == sc.CLOSED and [w.status[5] for w in wants[2:]] == [cc.CLOSED] * 4
        assert all(len(x) > 0 for x in deliveries[5][1:]) and len(got[5]) < 4  # closed early, fed to the end
    # the carry did carry: judged on the plain rules' own output
    tails = [sum(1 for c in range(48) if w.status[c] == cc.OK and w.next_len[c] > len(deliveries[c][r]))
             for r, w in enumerate(wants)]
    assert max(tails) >= 24, tails


# ---- 3. lifted cap -----------------------------------------------------------------

def lifted_deliveries(rng):
    big, small = sc.rand_body(rng, 40005), [sc.rand_body(rng, n) for n in (300, 50, 700, 9)]
    conns = [sc.frame(big) + sc.frame(b"behind"), sc.frame(small[0]) + sc.frame(small[1]),
             sc.frame(small[2]) + sc.frame(small[3])]
    cuts = [[10012, 20012, 30012], [5, 200, 330], [0, 100, 100]]
    deliveries = [[c[a:b] for a, b in zip([0] + k, k + [len(c)])] for c, k in zip(conns, cuts)]
    bodies = [[big, b"behind"], small[:2], small[2:]]
    return deliveries, bodies


def test_lifted_cap_long_tail():
    """RPC_FRAMES_LIFT_CAP: one body of 40,005 bytes arrives in 4 deliveries beside two small
    connections; with room = 64 KiB (the long route) it is delivered byte-exact."""
    deliveries, bodies = lifted_deliveries(np.random.default_rng(0x11F7))
    got, state, wants = run_rounds(deliveries, "server", lift_cap=True, room=65536)
    assert [[e[0] for e in g] for g in got] == bodies and state == [sc.OPEN] * 3
    assert [w.next_len[0] - len(deliveries[0][r]) for r, w in enumerate(wants)] == [0, 10012, 20012, 30012]


def test_lifted_cap_needs_room():
    """The same deliveries with the default room: the long tail reads NO_ROOM, nothing of the
    next buffer is touched for it (run_rounds compares every byte), the others are unaffected."""
    deliveries, bodies = lifted_deliveries(np.random.default_rng(0x11F7))
    got, state, wants = run_rounds(deliveries, "server", lift_cap=True, room=rpc_amd.CARRY_ROOM)
    assert wants[1].status == [cc.NO_ROOM, cc.OK, cc.OK] and wants[1].next_len[0] == 0
    assert [[e[0] for e in g] for g in got[1:]] == bodies[1:]
    assert bodies[0][0] not in [e[0] for e in got[0]]


# ---- 4. contract corners -------------------------------------------------------------

@pytest.mark.parametrize("room", ROOMS)
def test_outputs_may_alias_inputs(room):
    """d_next_off is d_conn_off and d_next_len is d_conn_len, on both routes."""
    case, _ = cc.corner_case(room)
    want = cc.want_of(case)
    big, nxt = guarded_next(case, 0)
    off, ln, used, state, at, nl = case_tensors(case)
    stream = dev_bytes(case.stream)
    status = torch.empty(len(case.conns), dtype=torch.uint8, device=DEV)
    carried = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    rc = _lib.rpc_frames_carry_device(stream.data_ptr(), stream.numel(), off.data_ptr(), ln.data_ptr(), used.data_ptr(),
                                      state.data_ptr(), len(case.conns), nxt.data_ptr(), nxt.numel(), at.data_ptr(),
                                      room, nl.data_ptr(), off.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                      carried.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    same(want, big, GUARD, off, ln, status, carried, ("alias", room))


def test_no_connections_zeroes_carried():
    carried = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    rc = _lib.rpc_frames_carry_device(None, 0, None, None, None, None, 0, None, 0, None, rpc_amd.CARRY_ROOM, None, None,
                                      None, None, carried.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and host(carried, np.uint64) == [0]
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    r = rpc_amd.frames_carry(torch.empty(0, dtype=torch.uint8, device=DEV), e, e, e, None,
                             torch.empty(16, dtype=torch.uint8, device=DEV), e)
    assert r.next_offsets.numel() == 0 and host(r.carried, np.uint64) == [0]


def test_python_argument_checks():
    e = i64([0, 0])
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        rpc_amd.frames_carry(buf, e, i64([0]), e, None, buf.clone(), e)
    with pytest.raises(ValueError):
        rpc_amd.frames_carry(buf, e, e, e, e, buf.clone(), e)  # state is uint8
    with pytest.raises(ValueError):
        rpc_amd.frames_carry(buf, e, e, e, None, buf.clone(), e, new_lengths=u8([0, 0]))


def test_device_error_word_is_honoured():
    """While the device error word is set the call returns RPCCRC_EIO, as every asynchronous
    call; after a clear it works.  Forced in a child process on the fault-injection build
    (RPCCRC_TEST_STEAL_GIVEUP=1: the next tail-stealing launch gives up its waits)."""
    code = r"""
import numpy as np, torch, rpc_amd
torch.cuda.set_device(0)
n, L = 65536, 4096
base = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
rpc_amd.fill_random(base, 0x6E7)
rpc_amd.device_uniform(base, n, L)
torch.cuda.synchronize()
print("status", rpc_amd.device_status())
z = torch.zeros(2, dtype=torch.int64, device="cuda:0")
nxt = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
at = torch.full((2,), 2048, dtype=torch.int64, device="cuda:0")
def go():
    try:
        r = rpc_amd.frames_carry(base, z, z, z, None, nxt, at)
        return r.status.cpu().tolist()
    except rpc_amd.RpcCrcError as e:
        return e.code
print("carry", go())
print("clear", rpc_amd.device_clear_status(), rpc_amd.device_status())
print("after", go())
"""
    env = dict(os.environ, RPCCRC_TEST_STEAL_GIVEUP="1", PYTHONPATH=REPO,
               RPCCRC_LIB=os.path.join(REPO, "rpc_amd", "lib", "librpccrc_test.so"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    for want in ("status -5", "carry -5", "clear -5 0", "after [0, 0]"):
        assert want in p.stdout, (want, p.stdout)
