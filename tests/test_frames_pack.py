"""Frame pack on the GPU (rpc_frames_pack_device): wire streams built
on the device from bodies, against the plain Python rules of tests/pack_cases.py, the
golden frames the reference itself put on the wire, and -- the strongest check of
both -- fed straight back into the fused frame scan in the opposite role."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import pack_cases as pc  # noqa: E402
import scan_cases as sc  # noqa: E402
from oracle import oracle  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_pack.h")
GUARD = 64


def kernel_constant(name):
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(PACK_H).read())
    assert m, f"{name} not found in {PACK_H}"
    return int(m.group(1))


T = kernel_constant("kPackTile")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bytes(blob, mis=0):
    """blob on the device, its first byte mis bytes past a 16-byte boundary."""
    a = np.zeros(mis + len(blob), dtype=np.uint8)
    a[mis:] = np.frombuffer(bytes(blob), dtype=np.uint8)
    return to_dev(a)[mis:]


def i64(a):
    return to_dev(np.asarray(a, dtype=np.uint64).view(np.int64))


def i32(a):
    return to_dev(np.asarray(a, dtype=np.uint32).view(np.int32))


def i16(a):
    return to_dev(np.asarray(a, dtype=np.uint16).view(np.int16))


def host(t, dtype):
    return t.cpu().numpy().view(dtype).tolist()


def entry_tensors(entries):
    typ, ver, off, ln = zip(*entries)
    return i16(typ), i16(ver), i64(off), i32(ln)


def pack_into_guarded(case, cap, src_mis=0, out_mis=0):
    """Packs `case` into a slice of a larger 0xA5-filled tensor and checks everything
    against pack_cases.expected: the output byte for byte (0xA5 in every frame that is not
    written), the guard bytes on both sides, offsets, verdicts, CRCs, the CSR and the total."""
    want = pc.expected(case.bodies, case.entries, case.conn_first, case.lift_cap, cap)
    nb = len(want.out)
    big = torch.full((GUARD + out_mis + nb + GUARD,), pc.FILL, dtype=torch.uint8, device=DEV)
    out = big[GUARD + out_mis:GUARD + out_mis + nb]
    assert nb == 0 or out.data_ptr() % 16 == out_mis
    typ, ver, off, ln = entry_tensors(case.entries)
    r = rpc_amd.frames_pack(dev_bytes(case.bodies, src_mis), off, ln, types=typ, versions=ver,
                            conn_first=None if case.conn_first is None else i64(case.conn_first),
                            lift_cap=case.lift_cap, out=out)
    what = (case.name, cap, src_mis, out_mis)
    got = big.cpu().numpy()
    lead = GUARD + out_mis
    assert (got[:lead] == pc.FILL).all(), what
    assert (got[lead + nb:] == pc.FILL).all(), what
    assert got[lead:lead + nb].tobytes() == want.out, what
    assert host(r.offsets, np.uint64) == want.offsets, what
    assert host(r.verdict, np.uint8) == want.verdict, what
    assert host(r.crc, np.uint32) == want.crc, what
    assert int(r.total.cpu()[0]) == want.total, what
    if case.conn_first is not None:
        assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what
    return want


@pytest.mark.parametrize("src_mis,out_mis", [(0, 0), (5, 9)])
def test_case_table(src_mis, out_mis):
    """The emulator's table (tests/test_pack_emu.py) at the kernels' tile: every alignment
    pair at six lengths, headers split across a tile edge, a piece over three frames, runs
    of heartbeats and of entries that emit nothing, both ends of the source, capacity at
    every kind of place, n = 1, a lifted-cap body over several tiles."""
    for case in pc.all_cases(T, out_mis):
        for cap in case.out_caps:
            want = pack_into_guarded(case, cap, src_mis, out_mis)
    assert want.total < (1 << 20)


def test_golden_frames(golden):
    """The four frames the reference put on the wire (request, response, PING, PONG):
    packing their bodies reproduces header_hex + body byte for byte."""
    frames = golden["frames"]
    bodies = b"".join(f["body"].encode() for f in frames)
    wire = b"".join(bytes.fromhex(f["header_hex"]) + f["body"].encode() for f in frames)
    entries, at = [], 0
    for f in frames:
        hdr = bytes.fromhex(f["header_hex"])
        entries.append((int.from_bytes(hdr[2:4], "big"), int.from_bytes(hdr[0:2], "big"), at, len(f["body"])))
        at += len(f["body"])
    assert [e[0] for e in entries] == [pc.DATA, pc.DATA, pc.PING, pc.PONG]
    typ, ver, off, ln = entry_tensors(entries)
    r = rpc_amd.frames_pack(dev_bytes(bodies), off, ln, types=typ, versions=ver)
    assert r.total == len(wire)
    assert r.stream.cpu().numpy().tobytes() == wire
    assert host(r.verdict, np.uint8) == [pc.OK, pc.OK, pc.CONTROL, pc.CONTROL]


def round_trip_batch(rng, heartbeat, empty_only_last):
    """~2000 entries in 64 connections (two of them empty): bodies of 0 .. 1024 bytes with
    0, 1, 1023 and 1024 present, a heartbeat every so often."""
    src = sc.rand_body(rng, 200000)
    entries, conn = [], [0]
    for c in range(64):
        k = 0 if c in (7, 63) else int(rng.integers(20, 45))
        for j in range(k):
            last = j == k - 1
            if not last and rng.integers(0, 6) == 0:
                entries.append((heartbeat, 1, 0, 0))
                continue
            ln = int(rng.choice([1, 1023, 1024, int(rng.integers(1, 1025))]))
            if (last and c % 4 == 0) or (not empty_only_last and rng.integers(0, 10) == 0):
                ln = 0
            entries.append((pc.DATA, 1, int(rng.integers(0, len(src) - ln + 1)), ln))
        conn.append(len(entries))
    lens = {e[3] for e in entries if e[0] == pc.DATA}
    assert {0, 1, 1023, 1024} <= lens and 1900 <= len(entries) <= 2900
    return src, entries, conn


@pytest.mark.parametrize("packer", ["server", "client"])
def test_round_trip_through_the_scan(packer):
    """What pack produces, scanned and verified in the opposite role: the same offsets,
    every frame OK or CONTROL, every connection OPEN with all its bytes consumed.  A client
    closes on an empty data frame (RECV_ERR, rpc_async.c:330-349), so the server-packs leg
    has empty bodies only as the last frame of a connection and expects exactly that there."""
    rng = np.random.default_rng(11 + (packer == "client"))
    heartbeat = pc.PONG if packer == "server" else pc.PING
    receiver = "client" if packer == "server" else "server"
    src, entries, conn = round_trip_batch(rng, heartbeat, empty_only_last=(packer == "server"))
    typ, ver, off, ln = entry_tensors(entries)
    p = rpc_amd.frames_pack(dev_bytes(src), off, ln, types=typ, conn_first=i64(conn))
    want = pc.expected(src, entries, conn)
    assert p.total == want.total and host(p.offsets, np.uint64) == want.offsets
    assert p.stream.cpu().numpy().tobytes() == want.out
    cbf = p.conn_bytes_first
    r = rpc_amd.frames_scan(p.stream, cbf[:-1].contiguous(), (cbf[1:] - cbf[:-1]).contiguous(), role=receiver,
                            verify=True, max_frames=len(entries))
    assert r.nframes == len(entries)
    assert host(r.frame_offsets, np.uint64) == want.offsets
    assert host(r.conn_first, np.uint64) == conn
    empty_last = [c for c in range(64) if conn[c + 1] > conn[c] and entries[conn[c + 1] - 1][3] == 0
                  and entries[conn[c + 1] - 1][0] == pc.DATA]
    closes = receiver == "client"
    exp_v = [pc.CONTROL if e[0] == heartbeat else pc.OK for e in entries]
    exp_state = [rpc_amd.CONN_OPEN] * 64
    if closes:
        assert empty_last
        for c in empty_last:
            exp_v[conn[c + 1] - 1] = pc.RECV_ERR
            exp_state[c] = rpc_amd.CONN_CLOSED
    assert host(r.verdict, np.uint8) == exp_v
    assert host(r.state, np.uint8) == exp_state
    assert host(r.consumed, np.uint64) == [want.conn_bytes_first[c + 1] - want.conn_bytes_first[c] for c in range(64)]
    # and the plain walk of the host-built stream says the same
    wfo, _, wfirst, wconsumed, wstate, _ = sc.expected(want.out, np.array(want.conn_bytes_first[:-1], dtype=np.uint64),
                                                       np.diff(np.array(want.conn_bytes_first, dtype=np.uint64)),
                                                       receiver, False, want_decoys=False)
    assert wfo == want.offsets and wfirst == conn and wstate == exp_state


def test_lifted_cap_large_bodies():
    """RPC_FRAMES_LIFT_CAP: bodies of 5 MiB + 3, 300 KiB, 0 and 17 bytes at odd source
    offsets; the stream against the host-built one, the CRCs against the oracle."""
    lens = [5 * (1 << 20) + 3, 300 << 10, 0, 17]
    src = oracle.splitmix_bytes(sum(lens) + 64, 0x9ACC0001)
    offs, at = [], 1
    for n in lens:
        offs.append(at)
        at += n + (2 if (at + n) % 2 else 1)  # (every offset odd)
    assert all(o % 2 for o in offs) and at <= len(src)
    blob = src.tobytes()
    r = rpc_amd.frames_pack(to_dev(src), i64(offs), i32(lens), lift_cap=True)
    wire = b"".join(sc.frame(blob[o:o + n]) for o, n in zip(offs, lens))
    assert r.total == len(wire)
    assert r.stream.cpu().numpy().tobytes() == wire
    assert host(r.crc, np.uint32) == [oracle.crc32(blob[o:o + n]) for o, n in zip(offs, lens)]
    assert host(r.verdict, np.uint8) == [pc.OK] * 4
    capped = rpc_amd.frames_pack(to_dev(src), i64(offs), i32(lens))  # the cap in force: the two big ones stay home
    assert host(capped.verdict, np.uint8) == [pc.TOO_LARGE, pc.TOO_LARGE, pc.OK, pc.OK]
    assert capped.stream.cpu().numpy().tobytes() == sc.frame(b"") + sc.frame(blob[offs[3]:offs[3] + 17])


def test_layout_only_call_and_capacity():
    """out=None (layout-only call, then an exactly sized buffer) and a caller's exactly
    sized out give identical results; with one byte less only the last non-empty frame is
    MALFORMED and none of its bytes is touched."""
    case = next(c for c in pc.small_cases(T, 0) if c.name == "capacity")
    typ, ver, off, ln = entry_tensors(case.entries)
    bodies, conn = dev_bytes(case.bodies), i64(case.conn_first)
    a = rpc_amd.frames_pack(bodies, off, ln, types=typ, versions=ver, conn_first=conn)
    out = torch.full((a.total,), pc.FILL, dtype=torch.uint8, device=DEV)
    b = rpc_amd.frames_pack(bodies, off, ln, types=typ, versions=ver, conn_first=conn, out=out)
    assert int(b.total.cpu()[0]) == a.total == a.stream.numel()
    for x, y in ((a.stream, b.stream), (a.offsets, b.offsets), (a.verdict, b.verdict), (a.crc, b.crc),
                 (a.conn_bytes_first, b.conn_bytes_first)):
        assert torch.equal(x, y)
    short = torch.full((a.total,), pc.FILL, dtype=torch.uint8, device=DEV)
    c = rpc_amd.frames_pack(bodies, off, ln, types=typ, versions=ver, conn_first=conn, out=short[:a.total - 1])
    va, vc = host(a.verdict, np.uint8), host(c.verdict, np.uint8)
    sizes = np.diff(np.array(host(a.offsets, np.uint64) + [a.total]))
    last = int(np.flatnonzero(sizes)[-1])
    assert [i for i in range(len(va)) if va[i] != vc[i]] == [last] and vc[last] == pc.MALFORMED
    at = host(a.offsets, np.uint64)[last]
    assert torch.equal(short[:at], a.stream[:at]) and (short[at:] == pc.FILL).all()
    assert torch.equal(a.offsets, c.offsets) and int(c.total.cpu()[0]) == a.total  # the layout never depends on out_cap


def test_scalar_and_array_forms_agree():
    """`type` / `version` as scalars and as per-entry arrays of the same value."""
    rng = np.random.default_rng(3)
    src = sc.rand_body(rng, 5000)
    n = 300
    ln = rng.integers(0, 1025, n)
    off = [int(rng.integers(0, len(src) - k + 1)) for k in ln]
    bodies = dev_bytes(src)
    for typ, ver in ((pc.DATA, 1), (9, 0x0102), (pc.PING, 2), (pc.NONE, 1)):
        a = rpc_amd.frames_pack(bodies, i64(off), i32(ln), version=ver, type_=typ)
        b = rpc_amd.frames_pack(bodies, i64(off), i32(ln), types=i16([typ] * n), versions=i16([ver] * n))
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y), (typ, ver)
        assert a.total == b.total
        want = pc.expected(src, [(typ, ver, o, int(k)) for o, k in zip(off, ln)])
        assert a.stream.cpu().numpy().tobytes() == want.out and host(a.crc, np.uint32) == want.crc
    hb = rpc_amd.frames_pack(None, i64([0] * 5), None, type_=pc.PONG)  # a scalar heartbeat type needs no bodies at all
    assert hb.stream.cpu().numpy().tobytes() == sc.frame(b"", typ=pc.PONG, crc=0) * 5
