"""Frame unpack on the GPU (rpc_frames_unpack_device): verified bodies as C
strings and the reply plan, against the plain Python rules of tests/unpack_cases.py byte for
byte and word for word, and -- scan -> unpack -> pack -- as an echo server whose wire bytes
are built in Python from the plain walk and the oracle's CRC."""
import os
import re
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import scan_cases as sc  # noqa: E402
import unpack_cases as uc  # noqa: E402
from oracle import oracle  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_pack.h")
GUARD = 64
VARIANTS = [("server", 1), ("server", 0), ("client", 1), ("client", 0)]


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


def u8(a):
    return to_dev(np.asarray(a, dtype=np.uint8))


def host(t, dtype):
    return t.cpu().numpy().view(dtype).tolist()


def entry_tensors(case):
    off, v = zip(*case.entries)
    return i64(off), u8(v)


def same_words(r, want, what, conn=True):
    assert host(r.body_offsets, np.uint64) == want.body_offsets, what
    assert host(r.body_lens, np.uint32) == want.body_lens, what
    assert host(r.reply_types, np.uint16) == want.reply_types, what
    assert host(r.versions, np.uint16) == want.versions, what
    assert host(r.verdict, np.uint8) == want.verdict, what
    total = r.total if isinstance(r.total, int) else int(r.total.cpu()[0])
    assert total == want.total, what
    if conn:
        assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what


def unpack_into_guarded(case, cap, src_mis=0, out_mis=0):
    """Unpacks `case` into a slice of a larger 0xA5-filled tensor and checks everything against
    unpack_cases.expected: the output byte for byte (0xA5 outside every written entry), the
    guard bytes on both sides and beyond out_cap, and every per-entry word."""
    want = uc.want_of(case, cap)
    nb = len(want.out)
    big = torch.full((GUARD + out_mis + nb + GUARD,), uc.FILL, dtype=torch.uint8, device=DEV)
    out = big[GUARD + out_mis:GUARD + out_mis + nb]
    assert nb == 0 or out.data_ptr() % 16 == out_mis
    off, v = entry_tensors(case)
    stream = dev_bytes(case.stream, src_mis)
    assert stream.data_ptr() % 16 == src_mis
    r = rpc_amd.frames_unpack(stream, off, v, role=case.role, lift_cap=case.lift_cap, nul=bool(case.nul),
                              conn_first=None if case.conn_first is None else i64(case.conn_first), out=out)
    what = (case.name, case.role, case.nul, cap, src_mis, out_mis)
    got = big.cpu().numpy()
    lead = GUARD + out_mis
    assert (got[:lead] == uc.FILL).all(), what
    assert (got[lead + nb:] == uc.FILL).all(), what
    assert got[lead:lead + nb].tobytes() == want.out, what
    same_words(r, want, what, conn=case.conn_first is not None)
    assert host(v, np.uint8) == [e[1] for e in case.entries], what  # the input verdicts are left alone
    return want


@pytest.mark.parametrize("role,nul", VARIANTS)
@pytest.mark.parametrize("src_mis,out_mis", [(0, 0), (5, 9)])
def test_case_table(src_mis, out_mis, role, nul):
    """The emulator's table (tests/test_unpack_emu.py) at the kernels' tile: every alignment
    pair at six lengths, an entry ending on a tile edge and one starting on it, 40 heartbeats,
    2000 empty bodies (1-byte entries, more than the LDS staging holds), every verdict that
    delivers nothing, padding entries, empty connections at both ends of the CSR."""
    case = uc.table_case(T, out_mis, role, nul)
    want = unpack_into_guarded(case, None, src_mis, out_mis)
    assert want.total < (1 << 20) and len(case.stream) < (1 << 20)
    if role == "server" and nul:
        assert sum(1 for c in want.chunks if len(c) == 1) >= uc.EMPTY_RUN > 1536
    assert case.conn_first[:2] == [0, 0] and case.conn_first[-1] == case.conn_first[-2]


@pytest.mark.parametrize("role,nul", VARIANTS)
def test_lying_verdicts(role, nul):
    """A verdict the stream contradicts -- OK on a header or a body that ends past the
    stream, on body_len 1025 with the cap in force, on a heartbeat, on an empty body at a
    client; CONTROL on a data frame -- reads MALFORMED / NONE and writes nothing; the entries
    around it are delivered."""
    names = set()
    for case in uc.lying_cases(role, nul):
        want = unpack_into_guarded(case, None, 3, 7)
        assert want.verdict == [uc.OK, uc.MALFORMED, uc.OK] and want.reply_types[1] == uc.NONE, case.name
        assert want.body_lens[1] == 0 and want.versions[1] == 0 and not want.chunks[1]
        names.add(case.name)
    assert {"header_past_end", "body_past_end", "over_cap", "ok_on_control", "control_on_data"} <= names
    assert ("empty_at_client" in names) == (role == "client")


@pytest.mark.parametrize("role,nul", VARIANTS)
def test_capacity(role, nul):
    """out_cap at the total, one less, inside a body, on a NUL and 0, and the layout-only
    call: the layout is the same in all of them and only the entries that do not fit change."""
    case = next(c for c in uc.small_cases(T, 0, role, nul) if c.name == "capacity")
    full = uc.want_of(case, None)
    for cap in case.out_caps:
        want = unpack_into_guarded(case, cap, 0, 11)
        assert want.body_offsets == full.body_offsets and want.total == full.total
        assert want.body_lens == full.body_lens and want.versions == full.versions
        lim = full.total if cap is None else cap
        for i, c in enumerate(full.chunks):
            fits = not c or full.body_offsets[i] + len(c) <= lim
            assert (want.verdict[i], want.reply_types[i]) == ((full.verdict[i], full.reply_types[i]) if fits
                                                             else (uc.MALFORMED, uc.NONE))
    off, v = entry_tensors(case)
    conn = i64(case.conn_first)
    a = rpc_amd.frames_unpack(dev_bytes(case.stream), off, v, role=role, nul=bool(nul), conn_first=conn)  # layout-only first
    assert a.total == full.total == a.bodies.numel()
    assert a.bodies.cpu().numpy().tobytes() == full.out
    same_words(a, full, (role, nul))
    for c in uc.small_cases(T, 0, role, nul):
        if c.name.startswith("one_"):
            for cap in c.out_caps:
                unpack_into_guarded(c, cap, 1, 2)


@pytest.mark.parametrize("nul", [1, 0])
def test_lifted_cap(nul):
    """RPC_FRAMES_LIFT_CAP: one body of 3 tiles + 5 bytes at an odd stream offset between
    small frames; with the cap in force the same verdicts are contradicted."""
    cases = {c.name: c for c in uc.small_cases(T, 5, "server", nul)}
    for cap in cases["lifted"].out_caps:
        want = unpack_into_guarded(cases["lifted"], cap, 0, 5)
    assert max(uc.want_of(cases["lifted"], None).body_lens) == 3 * T + 5
    assert want.verdict == [uc.OK, uc.MALFORMED, uc.SKIPPED, uc.MALFORMED, uc.MALFORMED]  # (the short out_cap)
    want = unpack_into_guarded(cases["lifted_not"], None, 0, 5)
    assert want.verdict == [uc.OK, uc.MALFORMED, uc.SKIPPED, uc.MALFORMED, uc.OK]


def test_verdict_in_place():
    """d_verdict_out aliasing d_verdict (through the C-ABI) gives what separate arrays give."""
    case = next(c for c in uc.small_cases(T, 0, "server", 1) if c.name == "capacity")
    case = case._replace(entries=case.entries + [(uc.FAR, uc.OK)])  # (an OK far past the stream)
    cap = uc.want_of(case, None).total - 1  # the last body does not fit: its verdict changes too
    want = uc.want_of(case, cap)
    off, v = entry_tensors(case)
    stream = dev_bytes(case.stream, 1)
    out_a = torch.full((cap,), uc.FILL, dtype=torch.uint8, device=DEV)
    sep = rpc_amd.frames_unpack(stream, off, v, out=out_a)
    out = torch.full((cap,), uc.FILL, dtype=torch.uint8, device=DEV)
    n = len(case.entries)
    offs = torch.empty(n, dtype=torch.int64, device=DEV)
    rc = rpc_amd._lib.rpc_frames_unpack_device(stream.data_ptr(), stream.numel(), off.data_ptr(), v.data_ptr(), n, None, 0,
                                               rpc_amd.FRAMES_SERVER, 1, out.data_ptr(), out.numel(), offs.data_ptr(),
                                               None, None, None, v.data_ptr(), None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert host(v, np.uint8) == want.verdict == host(sep.verdict, np.uint8)
    changed = [i for i, e in enumerate(case.entries) if e[1] != want.verdict[i]]
    assert len(changed) == 2 and all(want.verdict[i] == uc.MALFORMED for i in changed)
    assert torch.equal(out, out_a) and out.cpu().numpy().tobytes() == want.out
    assert torch.equal(offs, sep.body_offsets)


def echo_batch(rng, role):
    """64 connections of about 8 KiB, all four endings, some CRC fields broken."""
    conns = [sc.random_conn(rng, int(rng.integers(7000, 9000)), role, ending=sc.ENDINGS[c % 4]) for c in range(64)]
    blob, offs, lens = sc.layout(rng, conns)
    blob = bytearray(blob)
    fo, fc, first, _, _, _ = sc.expected(bytes(blob), offs, lens, role, False, want_decoys=False)
    ctl = sc.PING if role == "server" else sc.PONG
    broken = 0
    for c in range(0, 64, 5):  # break the CRC field of a data frame somewhere in the middle
        mine = [o for o in fo[first[c]:first[c + 1]] if struct.unpack_from(">H", blob, o + 2)[0] != ctl]
        if len(mine) > 4:
            blob[mine[len(mine) // 2] + 11] ^= 0x40
            broken += 1
    assert broken >= 8
    return bytes(blob), offs, lens


def echo_expected(blob, offs, lens, role):
    """Per connection, what an echo server (or client) built on the plain walk puts on the
    wire: each frame the reference would dispatch re-stamped as DATA with its own version,
    body and CRC, each PING (server) as a PONG heartbeat, nothing for anything else."""
    fo, fc, first, _, _, _ = sc.expected(blob, offs, lens, role, False, want_decoys=False)
    ctl = sc.PING if role == "server" else sc.PONG
    wire, kinds = [], set()
    for c in range(len(offs)):
        out = b""
        for o in fo[first[c]:first[c + 1]]:
            ver, typ, bl, crc = struct.unpack_from(">HHII", blob, o)
            if typ == ctl:
                if role == "server":
                    out += sc.frame(b"", typ=sc.PONG, crc=0, version=ver)
                kinds.add("control")
                continue
            if bl > sc.MAX_BODY or (bl == 0 and role == "client"):
                kinds.add("close")
                break
            body = blob[o + sc.HDR:o + sc.HDR + bl]
            if oracle.crc32(body) != crc:
                kinds.add("bad_crc")
                break
            out += sc.frame(body, typ=0, version=ver, crc=oracle.crc32(body))
            kinds.add("data")
        wire.append(out)
    assert kinds == {"control", "close", "bad_crc", "data"}
    return wire, len(fo), first


@pytest.mark.parametrize("role", ["server", "client"])
def test_echo_round_trip(role):
    """scan + verify (padded) -> unpack (both nul values) -> pack with the unpack's reply
    types, versions and the scan's CSR: connection c's packed bytes are the echo of what the
    reference would have dispatched on it."""
    rng = np.random.default_rng(21 + (role == "client"))
    blob, offs, lens = echo_batch(rng, role)
    assert len(blob) < (1 << 20)
    wire, nframes, first = echo_expected(blob, offs, lens, role)
    stream = dev_bytes(blob, 3)
    padded = nframes + 37
    r = rpc_amd.frames_scan(stream, i64(offs), i64(lens), role=role, verify=True, max_frames=padded)
    assert r.nframes == nframes and host(r.conn_first, np.uint64) == first
    fo, vin = host(r.frame_offsets, np.uint64), host(r.verdict, np.uint8)
    assert {uc.OK, uc.CONTROL, uc.BAD_CRC, uc.NOT_REACHED, uc.TOO_LARGE, uc.MALFORMED} <= set(vin)
    for nul in (1, 0):
        u = rpc_amd.frames_unpack(stream, r.frame_offsets, r.verdict, role=role, nul=bool(nul), conn_first=r.conn_first)
        want = uc.expected(blob, fo, vin, first, role, False, nul)
        same_words(u, want, (role, nul))
        assert u.bodies.cpu().numpy().tobytes() == want.out
        types = set(host(u.reply_types, np.uint16))
        assert types == ({uc.DATA, uc.PONG, uc.NONE} if role == "server" else {uc.DATA, uc.NONE})
        p = rpc_amd.frames_pack(u.bodies, u.body_offsets, u.body_lens, types=u.reply_types, versions=u.versions,
                                conn_first=r.conn_first)
        cbf = host(p.conn_bytes_first, np.uint64)
        sent = p.stream.cpu().numpy().tobytes()
        for c in range(64):
            assert sent[cbf[c]:cbf[c + 1]] == wire[c], (role, nul, c)
        assert p.total == sum(map(len, wire))


def test_no_connections_and_no_entries():
    """nconn == 0, and n == 0 with d_total (and a CSR): everything reads 0."""
    case = next(c for c in uc.small_cases(T, 0) if c.name == "capacity")
    off, v = entry_tensors(case)
    want = uc.want_of(case._replace(conn_first=[0]), None)
    r = rpc_amd.frames_unpack(dev_bytes(case.stream), off, v, conn_first=i64([0]))  # nconn == 0
    same_words(r, want, "nconn 0")
    assert host(r.conn_bytes_first, np.uint64) == [want.total]
    none64, none8 = torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV)
    e = rpc_amd.frames_unpack(dev_bytes(case.stream), none64, none8, conn_first=i64([0, 0, 0]))
    assert e.total == 0 and e.bodies.numel() == 0 and host(e.conn_bytes_first, np.uint64) == [0, 0, 0]
    out = torch.full((32,), uc.FILL, dtype=torch.uint8, device=DEV)
    e = rpc_amd.frames_unpack(dev_bytes(case.stream), none64, none8, out=out)
    assert int(e.total.cpu()[0]) == 0 and (out == uc.FILL).all()
