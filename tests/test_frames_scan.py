"""Frame scan on the GPU (rpc_frames_scan_device / rpc_frames_scan_verify_device,
DESIGN.md 4.11): the frames of raw connection bytes, found on the device, against
the plain Python walk of tests/scan_cases.py; the fused call against
``oracle.frame_verdict`` per frame (and against the reference server itself in
tests/test_dropin_pipelined.py)."""
import functools
import os
import re
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import scan_cases as sc  # noqa: E402
from oracle import oracle  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_scan.h")
CLOSING = (rpc_amd.FRAME_BAD_CRC, rpc_amd.FRAME_TOO_LARGE, rpc_amd.FRAME_RECV_ERR)


def kernel_constant(name):
    """The kernels' own value of a constant (frames_scan.h)."""
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(SCAN_H).read())
    assert m, f"{name} not found in {SCAN_H}"
    return int(m.group(1))


T = kernel_constant("kScanTile")
G = kernel_constant("kScanGroup")
LEVELS = kernel_constant("kScanMaxLevels")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_stream(blob):
    return to_dev(np.frombuffer(blob, dtype=np.uint8).copy())


def i64(a):
    return to_dev(np.asarray(a, dtype=np.uint64).view(np.int64))


@pytest.fixture(params=["serial", "tiled"])
def scan_path(request):
    """"tiled" cuts every cap-in-force connection of more than one tile into tiles;
    "serial" walks every connection with one lane."""
    rpc_amd.set_scan_path(request.param)
    yield request.param
    rpc_amd.set_scan_path("auto")


def scan(blob, offs, lens, role="server", lift_cap=False, **kw):
    r = rpc_amd.frames_scan(dev_stream(blob), i64(offs), i64(lens), role=role, lift_cap=lift_cap, **kw)
    return r, (r.frame_offsets.cpu().numpy().tolist(), r.frame_conn.cpu().numpy().tolist(),
               r.conn_first.cpu().numpy().tolist(), r.consumed.cpu().numpy().tolist(), r.state.cpu().numpy().tolist())


@functools.lru_cache(maxsize=None)
def mixed_stream(role, lift_cap):
    """About 300 connections of 0-8 KiB at unaligned, non-adjacent offsets: mixed frame
    kinds, decoys, every ending; an empty one, one of 11 bytes, one outside the stream;
    and a few of several tiles, so that the tiled route has work.  With its plain walk."""
    rng = np.random.default_rng(1000 + 2 * (role == "client") + lift_cap)
    conns = [sc.random_conn(rng, int(rng.integers(0, 8192)), role, lift_cap) for _ in range(300)]
    conns[17] = b""
    conns[18] = sc.frame(b"0123456789")[:11]
    for k, n in ((40, T + 5), (41, 2 * T), (42, 3 * T + 1000), (43, T + 12)):
        conns[k] = sc.random_conn(rng, n, role, lift_cap)
    conns[44] = sc.filler(rng, 2 * T, role)  # ends exactly at a tile end: its last tile is empty
    blob, offs, lens = sc.layout(rng, conns)
    offs = np.concatenate([offs, np.array([len(blob) - 50, 2**63 + 5], dtype=np.uint64)])
    lens = np.concatenate([lens, np.array([100, 12], dtype=np.uint64)])
    return blob, offs, lens, sc.expected(blob, offs, lens, role, lift_cap, tile=T)


@pytest.mark.parametrize("role", ["server", "client"])
@pytest.mark.parametrize("lift_cap", [False, True])
def test_scan_matches_plain_walk(role, lift_cap, scan_path):
    blob, offs, lens, want = mixed_stream(role, lift_cap)
    r, got = scan(blob, offs, lens, role, lift_cap)
    assert got[2] == want[2]
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[3] == want[3]
    assert got[4] == want[4]
    assert r.nframes == len(want[0])
    assert got[4][-2:] == [rpc_amd.CONN_CLOSED] * 2 and got[3][-2:] == [0, 0]  # outside the stream
    cats = want[5]
    kinds = ["data", "control", "decoys", "end_clean", "end_in_header", "end_in_body"]
    kinds += [] if lift_cap else ["close_too_large"]
    kinds += ["close_empty"] if role == "client" else []
    for k in kinds:
        assert cats.get(k), (k, cats)
    # every emitted frame is one the verify call does not call MALFORMED
    v, _ = rpc_amd.frames_verify(dev_stream(blob), r.frame_offsets, role=role, lift_cap=lift_cap)
    assert rpc_amd.FRAME_MALFORMED not in v.cpu().numpy().tolist()


def two_tile_conns(role):
    """Connections of exactly two tiles whose chain leaves the first tile at every exit
    0 .. 1035 (0: a frame ending exactly at the tile's end; 1035: a 1024-byte body whose
    frame starts at the tile's last byte)."""
    rng = np.random.default_rng(77 + (role == "client"))
    head = sc.filler(rng, T - 3000, role)
    conns = []
    for x in range(sc.E):
        bl = int(rng.integers(max(1, x - 11), sc.MAX_BODY + 1))
        start = T + x - (sc.HDR + bl)
        body = sc.decoy_body(rng, bl) if x % 3 == 0 else sc.rand_body(rng, bl)
        tail = sc.random_conn(rng, int(rng.integers(sc.HDR, 1500)), role)
        conns.append(head + sc.filler(rng, start - len(head), role) + sc.frame(body) + tail)
    blob, offs, lens = sc.layout(rng, conns)
    assert all(T < n < 2 * T for n in lens.tolist())
    want = sc.expected(blob, offs, lens, role, False, tile=T, want_decoys=False)
    assert all(want[5].get("exit_%d" % x) for x in range(sc.E))
    return blob, offs, lens, want


@pytest.mark.parametrize("role", ["server", "client"])
def test_two_tiles_every_straddle_position(role):
    """Tiled route: one connection of exactly two tiles, swept over every straddle
    position (two_tile_conns)."""
    blob, offs, lens, want = two_tile_conns(role)
    rpc_amd.set_scan_path("tiled")
    try:
        r, got = scan(blob, offs, lens, role)
    finally:
        rpc_amd.set_scan_path("auto")
    assert got == tuple(want[:5])


def top_level_stream():
    """One connection of G^kScanMaxLevels tiles and a bit, just long enough for the top
    up-sweep level to hold two maps (the constants come from frames_scan.h), built
    vectorised: (stream, connection offset, length, frame starts by construction)."""
    total = T * G**LEVELS + 777
    assert total // T + 1 > G**LEVELS and total <= 160 << 20
    rng = np.random.default_rng(4242)
    stream = rng.integers(0, 256, total + 9, dtype=np.uint8)
    lens = rng.integers(0, sc.MAX_BODY + 1, total // 500, dtype=np.int64)
    starts = 3 + np.concatenate([[0], np.cumsum(sc.HDR + lens)[:-1]])
    keep = starts + sc.HDR + lens <= 3 + total
    starts, lens = starts[keep], lens[keep]
    hdr = np.zeros((len(starts), 8), dtype=np.uint8)
    hdr[:, 1] = 1                                   # version 1, type DATA
    hdr[:, 3] = np.where(np.arange(len(starts)) % 50 == 7, rpc_amd.RPC_TYPE_PONG, 0)  # (a data frame at a server)
    hdr[:, 4:8] = lens.astype(">u4").view(np.uint8).reshape(-1, 4)
    stream[starts[:, None] + np.arange(8)[None, :]] = hdr
    return stream, 3, total, starts


def test_every_up_sweep_level():
    """Tiled route, every up-sweep level the kernels have (top_level_stream); under
    AUTO, which tiles a connection of this length."""
    stream, off, total, starts = top_level_stream()
    blob = stream.tobytes()
    offs, clen = np.array([off], dtype=np.uint64), np.array([total], dtype=np.uint64)
    want = sc.expected(blob, offs, clen, "server", False, tile=T, want_decoys=False)
    assert len(want[0]) >= len(starts) and want[0][:len(starts)] == starts.tolist()
    r = rpc_amd.frames_scan(to_dev(stream), i64(offs), i64(clen))
    assert r.nframes == len(want[0])
    assert np.array_equal(r.frame_offsets.cpu().numpy(), np.array(want[0], dtype=np.int64))
    assert r.conn_first.cpu().numpy().tolist() == want[2]
    assert r.consumed.cpu().numpy().tolist() == want[3] and r.state.cpu().numpy().tolist() == want[4]
    assert not r.frame_conn.cpu().numpy().any()


def raw_scan(blob, offs, lens, cap, guard=64, flags=rpc_amd.FRAMES_SERVER):
    """The C call itself, with a guard region behind both frame arrays."""
    d = dev_stream(blob)
    n = len(offs)
    fo = torch.full((cap + guard,), -7, dtype=torch.int64, device=DEV)
    fc = torch.full((cap + guard,), -7, dtype=torch.int32, device=DEV)
    first = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    consumed = torch.empty(n, dtype=torch.int64, device=DEV)
    state = torch.empty(n, dtype=torch.uint8, device=DEV)
    nf = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    do, dl = i64(offs), i64(lens)
    rc = rpc_amd._lib.rpc_frames_scan_device(d.data_ptr(), len(blob), do.data_ptr() if n else None,
                                             dl.data_ptr() if n else None, n, flags, fo.data_ptr() if cap else None,
                                             fc.data_ptr() if cap else None, cap, first.data_ptr(),
                                             consumed.data_ptr() if n else None, state.data_ptr() if n else None,
                                             nf.data_ptr(), rpc_amd._stream_handle(None))
    assert rc == 0, rc
    return (fo.cpu().numpy(), fc.cpu().numpy(), first.cpu().numpy().tolist(), consumed.cpu().numpy().tolist(),
            state.cpu().numpy().tolist(), int(nf.cpu()[0]))


def test_count_only_frame_cap_and_padding(scan_path):
    blob, offs, lens, want = mixed_stream("server", False)
    n = len(want[0])
    # count only: everything but the frame arrays
    fo, fc, first, consumed, state, nf = raw_scan(blob, offs, lens, 0)
    assert (nf, first, consumed, state) == (n, want[2], want[3], want[4])
    assert (fo == -7).all() and (fc == -7).all()
    # frame_cap below the count: the true count, the first frame_cap entries, nothing behind them
    cap = n - 321
    fo, fc, first, consumed, state, nf = raw_scan(blob, offs, lens, cap)
    assert (nf, first, consumed, state) == (n, want[2], want[3], want[4])
    assert fo[:cap].tolist() == want[0][:cap] and fc[:cap].tolist() == want[1][:cap]
    assert (fo[cap:] == -7).all() and (fc[cap:] == -7).all()
    # frame_cap above the count: the tail holds stream_bytes (connection -1)
    cap = n + 300
    fo, fc, first, consumed, state, nf = raw_scan(blob, offs, lens, cap)
    assert nf == n and fo[:n].tolist() == want[0] and fc[:n].tolist() == want[1]
    assert (fo[n:cap] == len(blob)).all() and (fc[n:cap] == -1).all()
    assert (fo[cap:] == -7).all() and (fc[cap:] == -7).all()
    # max_frames of the Python call: too small raises
    with pytest.raises(ValueError):
        rpc_amd.frames_scan(dev_stream(blob), i64(offs), i64(lens), max_frames=n - 1)
    assert rpc_amd.frames_scan(dev_stream(blob), i64(offs), i64(lens), max_frames=n).nframes == n


def test_no_connections_and_bad_arguments():
    fo, fc, first, consumed, state, nf = raw_scan(b"abcdefgh", np.zeros(0, np.uint64), np.zeros(0, np.uint64), 5)
    assert nf == 0 and first[0] == 0 and fo[:5].tolist() == [8] * 5 and (fo[5:] == -7).all()
    d, one, nfr = dev_stream(bytes(64)), i64([0]), torch.zeros(1, dtype=torch.int64, device=DEV)
    for flags in (0, 3, 8):
        rc = rpc_amd._lib.rpc_frames_scan_device(d.data_ptr(), 64, one.data_ptr(), one.data_ptr(), 1, flags, None, None,
                                                 0, one.data_ptr(), one.data_ptr(), one.data_ptr(), nfr.data_ptr(),
                                                 rpc_amd._stream_handle(None))
        assert rc == -22, flags
    assert rpc_amd._lib.rpc_frames_set_scan_path(3) == -22


def fused_expect(blob, want, role, lift_cap):
    """Per frame oracle.frame_verdict; behind a connection's first closing verdict
    NOT_REACHED with crc 0; a connection with a (reached) BAD_CRC is CLOSED."""
    fo, fc, first, consumed, state = want[:5]
    verdict, crc, state = [], [], list(state)
    for c in range(len(first) - 1):
        closed = False
        for i in range(first[c], first[c + 1]):
            v, k = (rpc_amd.FRAME_NOT_REACHED, 0) if closed else oracle.frame_verdict(blob, fo[i], role, lift_cap)
            verdict.append(v)
            crc.append(k)
            if v == rpc_amd.FRAME_BAD_CRC:
                state[c] = rpc_amd.CONN_CLOSED
            closed = closed or v in CLOSING
    return verdict, crc, state


def bad_crc_stream(role, seed):
    """Connections of a few pipelined frames; in some a bad CRC at position j, frames
    behind it; one connection whose only flaw is a bad CRC; closing headers; partial tails."""
    rng = np.random.default_rng(seed)
    conns, only_bad = [], None
    for c in range(300):
        k = int(rng.integers(0, 9))
        frames = [sc.frame(sc.decoy_body(rng, int(rng.integers(1, 700)))) for _ in range(k)]
        if k and c % 3 == 0:
            j = int(rng.integers(0, k))
            frames[j] = frames[j][:8] + struct.pack(">I", struct.unpack(">I", frames[j][8:12])[0] ^ 0x40) + frames[j][12:]
        if c % 7 == 1:
            frames.insert(int(rng.integers(0, k + 1)), sc.closing(rng, role))
        if c % 5 == 2:
            frames.append(sc.frame(b"x" * 100)[:int(rng.integers(1, 111))])
        conns.append(b"".join(frames))
    good = sc.frame(b'{"a":1}')
    conns[9] = good + good[:8] + struct.pack(">I", 1) + good[12:] + good  # only flaw: a bad CRC
    only_bad = 9
    return conns, only_bad


@pytest.mark.parametrize("role", ["server", "client"])
def test_fused_scan_verify(role, scan_path):
    conns, only_bad = bad_crc_stream(role, 31 + (role == "client"))
    rng = np.random.default_rng(1)
    blob, offs, lens = sc.layout(rng, conns)
    want = sc.expected(blob, offs, lens, role, False, want_decoys=False)
    verdict, crc, state = fused_expect(blob, want, role, False)
    n = len(want[0])
    r = rpc_amd.frames_scan(dev_stream(blob), i64(offs), i64(lens), role=role, max_frames=n + 9, verify=True)
    assert r.nframes == n
    assert r.frame_offsets.cpu().numpy().tolist() == want[0] + [len(blob)] * 9
    assert r.verdict.cpu().numpy().tolist() == verdict + [rpc_amd.FRAME_MALFORMED] * 9  # padding: MALFORMED, crc 0
    assert r.crc.cpu().numpy().view(np.uint32).tolist() == crc + [0] * 9
    assert r.state.cpu().numpy().tolist() == state
    assert r.consumed.cpu().numpy().tolist() == want[3]  # the scan's value
    assert verdict.count(rpc_amd.FRAME_NOT_REACHED) > 50 and verdict.count(rpc_amd.FRAME_BAD_CRC) > 30
    lo, hi = want[2][only_bad], want[2][only_bad + 1]
    assert verdict[lo:hi] == [rpc_amd.FRAME_OK, rpc_amd.FRAME_BAD_CRC, rpc_amd.FRAME_NOT_REACHED]
    assert want[4][only_bad] == rpc_amd.CONN_OPEN and state[only_bad] == rpc_amd.CONN_CLOSED
    assert want[3][only_bad] == len(conns[only_bad])
    # exact allocation (count first), no padding
    r2 = rpc_amd.frames_scan(dev_stream(blob), i64(offs), i64(lens), role=role, verify=True)
    assert r2.verdict.cpu().numpy().tolist() == verdict and r2.nframes == n


def test_fused_lifted_cap_big_bodies():
    """Cap lifted, about 4K frames in 64 connections, bodies of 256 KiB and more among
    them: verify's big-body route runs behind the scan.  One big body is corrupted:
    BAD_CRC, and what follows on its connection is NOT_REACHED."""
    rng = np.random.default_rng(8)
    conns = []
    for c in range(64):
        frames = [sc.frame(sc.rand_body(rng, int(rng.integers(0, 600)))) for _ in range(63)]
        conns.append(frames)
    for c, n in ((3, 256 << 10), (20, (300 << 10) + 1), (41, 1 << 20), (50, (256 << 10) - 1)):
        conns[c][10] = sc.frame(sc.rand_body(rng, n))
    f = conns[20][10]
    conns[20][10] = f[:200000] + bytes([f[200000] ^ 1]) + f[200001:]
    conns[33][5] = sc.frame(b"abc", crc=5)
    blob, offs, lens = sc.layout(rng, [b"".join(fr) for fr in conns])
    want = sc.expected(blob, offs, lens, "server", True, want_decoys=False)
    assert len(want[0]) == 64 * 63
    verdict, crc, state = fused_expect(blob, want, "server", True)
    r = rpc_amd.frames_scan(dev_stream(blob), i64(offs), i64(lens), lift_cap=True, max_frames=4096, verify=True)
    pad = 4096 - r.nframes
    assert r.frame_offsets.cpu().numpy().tolist() == want[0] + [len(blob)] * pad
    assert r.verdict.cpu().numpy().tolist() == verdict + [rpc_amd.FRAME_MALFORMED] * pad
    assert r.crc.cpu().numpy().view(np.uint32).tolist() == crc + [0] * pad
    assert r.state.cpu().numpy().tolist() == state and state[20] == state[33] == rpc_amd.CONN_CLOSED
    i = want[2][20] + 10
    assert verdict[i] == rpc_amd.FRAME_BAD_CRC and verdict[i + 1:want[2][21]] == [rpc_amd.FRAME_NOT_REACHED] * 52
    assert verdict.count(rpc_amd.FRAME_OK) == 64 * 63 - 2 - 52 - 57
