"""Every frame stage on a stream of its own (one round on one hipStream_t, one
synchronisation at its end).  On the default stream a launch or memset sent to the wrong stream,
a workspace lease returned too early or wrapper work on torch's current stream all cost nothing;
here each of them is a wrong answer, deterministically:

* the late-inputs harness (``behind_blocker``): the stage's inputs start as decoys -- legal
  inputs, all zero bytes -- and the real ones are copied over them on the side stream behind a
  long kernel, with the stage enqueued behind the copies and no host synchronisation in between.
  Whatever part of the stage runs on another stream runs at once, on the decoys.
* the busy default stream (``form_c``): the call gets ``stream=s`` alone while torch's current
  stream is held by the long kernel; wrapper work put on the current stream lands late (and a
  read-back put there would not return while the kernel runs).

Every expectation is the plain Python rules of the ``*_cases`` modules (and the oracle's CRC),
bit for bit; none is a default-stream run of the code under test.

The long kernel ("blocker").  The issue behind this module asked for the kernel of
test_drop_in_beside_a_long_kernel: one body given to ``device_batch(..., max_len=65536)``, taken
to be walked by a single wave.  Measured on an MI355X, that call does not last: one body of
256 MiB takes 0.13 ms and one of 2 GiB 0.65 ms (about 3 TB/s, CRCs right), so the longest body
the call accepts (4 GiB) ends after 1.3 ms, before even one pipeline is enqueued.  The blocker
is therefore ``torch.cuda._sleep(BLOCKER_CYCLES)``: one thread that spins on the clock and ends
by itself -- no host callback, no wait on memory, nothing a bug can leave closed -- and leaves
the whole chip free for whatever is misplaced (measured: a batch on another stream ends while it
spins).  Measured: 1e9 cycles last 417 ms, so BLOCKER_CYCLES = 3.6e8 lasts 150 ms.  The host
time to enqueue, printed by the tests with ``-s``: the two rounds of section 4, the longest
pipelines, 0.40 ms (server) and 0.50 ms (client), copies included; one stage 0.06 - 0.2 ms (up
to 1 ms the first time a kernel is used); the 60 calls of test_two_streams_interleaved 5.4 ms.
150 ms is 300 times a round and 27 times the three interleaved passes.

A process has four hardware queues, and streams that share one run in turn: a side stream on
the default stream's queue hid the wrapper defect of form (c) in one run on the MI355X.  So
``side_streams`` picks, once for the module, two side streams that run beside the default
stream and beside each other.  Every test that relies on the blocker asserts that it was still
running when the last call returned; if it was not, the run proved nothing and the test fails."""
import functools
import struct
import time
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import args_cases as ac  # noqa: E402
import carry_cases as cc  # noqa: E402
import pack_cases as pc  # noqa: E402
import reply_cases as rp  # noqa: E402
import request_cases as rq  # noqa: E402
import resolve_cases as rs  # noqa: E402
import route_cases as rc  # noqa: E402
import scan_cases as sc  # noqa: E402
import unpack_cases as uc  # noqa: E402
from oracle import oracle  # noqa: E402
from test_frames_carry import LONG_ROOM  # noqa: E402
from test_frames_route import DEV, FILL, GUARD, dev_bytes, filled, to_dev  # noqa: E402
from test_frames_scan import bad_crc_stream, fused_expect, mixed_stream, two_tile_conns  # noqa: E402
from test_frames_unpack import T as PACK_T  # noqa: E402

BLOCKER_CYCLES = 360_000_000
BYTE_GUARD = 64  # bytes of FILL on both sides of every byte output
WORD_FILL = {1: FILL, 2: FILL * 0x0101, 4: FILL * 0x01010101, 8: FILL * 0x0101010101010101}
MALFORMED = rpc_amd.FRAME_MALFORMED


# ---- small helpers ----------------------------------------------------------------------------

def u64(a):
    return to_dev(np.asarray([int(x) for x in a], dtype=np.uint64).view(np.int64))


def u32(a):
    return to_dev(np.asarray([int(x) & 0xFFFFFFFF for x in a], dtype=np.uint32).view(np.int32))


def u16(a):
    return to_dev(np.asarray(a, dtype=np.uint16).view(np.int16))


def u8(a):
    return to_dev(np.asarray(a, dtype=np.uint8))


def host(t, dtype):
    return t.cpu().numpy().view(dtype).tolist()


def total_of(r):
    return r.total if isinstance(r.total, int) else int(r.total.cpu()[0])


def guarded(nb, mis=0):
    """nb bytes of FILL whose first byte lies mis bytes past a 16-byte boundary, inside a larger
    FILL-ed tensor: (the whole tensor, the slice the call gets)."""
    big = torch.full((BYTE_GUARD + mis + nb + BYTE_GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = big[BYTE_GUARD + mis:BYTE_GUARD + mis + nb]
    assert nb == 0 or out.data_ptr() % 16 == mis
    return big, out


def same_bytes(big, mis, want, what):
    """The output byte for byte and the guard bytes on both sides."""
    got = big.cpu().numpy()
    lead = BYTE_GUARD + mis
    assert (got[:lead] == FILL).all() and (got[lead + len(want):] == FILL).all(), what
    assert got[lead:lead + len(want)].tobytes() == want, what


def guarded_words(n, np_dtype, torch_dtype):
    """n elements of FILL bytes with GUARD elements on both sides: (the whole tensor, the slice)."""
    big = filled(n, np_dtype, torch_dtype)
    return big, big[GUARD:GUARD + n]


def same_words(big, np_dtype, want, what):
    a = big.cpu().numpy().view(np_dtype)
    f = WORD_FILL[np.dtype(np_dtype).itemsize]
    assert (a[:GUARD] == f).all() and (a[GUARD + len(want):] == f).all(), what
    assert a[GUARD:GUARD + len(want)].tolist() == want, what


class on:
    """The test's own glue (slices, differences) on the stream under test."""

    def __init__(self, s):
        self.ctx = torch.cuda.stream(s)

    def __enter__(self):
        return self.ctx.__enter__()

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


# ---- the blocker and the late inputs -------------------------------------------------------------

class Blocker:
    """``start(s)`` enqueues the spin kernel on s and returns an event recorded behind it."""

    def start(self, s):
        with on(s):
            torch.cuda._sleep(BLOCKER_CYCLES)
        ev = torch.cuda.Event()
        ev.record(s)
        return ev


def runs_beside(a, b):
    """True if work on stream b ends while a kernel on stream a still runs: the two do not share
    a hardware queue.  (A process has four of them; streams that share one run in turn, and then
    a blocker on a holds b's work back as well and nothing misplaced could show.)"""
    with on(a):
        torch.cuda._sleep(BLOCKER_CYCLES // 10)
    ev = torch.cuda.Event()
    ev.record(a)
    with on(b):
        torch.cuda._sleep(1000)
    b.synchronize()
    beside = not ev.query()
    a.synchronize()
    return beside


@functools.lru_cache(maxsize=None)
def side_streams():
    """Two non-blocking side streams for the whole module, chosen so that the default stream and
    the two run beside one another in every pairing (checked both ways round)."""
    torch.cuda.synchronize()
    default, found = torch.cuda.default_stream(), []
    for _ in range(16):
        s = torch.cuda.Stream(device=DEV)
        if all(runs_beside(x, s) and runs_beside(s, x) for x in [default] + found):
            found.append(s)
        if len(found) == 2:
            return tuple(found)
    raise AssertionError("no two side streams with hardware queues of their own among 16")


STILL = "the blocker had ended when the call returned: this run proved nothing"


class Late:
    """Tensors whose real contents arrive late: each is copied to a staging tensor and zeroed
    (the decoy: zero bytes, zero offsets, zero lengths -- legal inputs that give another answer);
    ``enqueue(s)`` copies the staging tensors back over them on s."""

    def __init__(self, tensors):
        self.pairs = [(x, x.clone()) for x in tensors if x is not None and x.numel()]
        for x, _ in self.pairs:
            x.zero_()

    def enqueue(self, s):
        with on(s):
            for x, staged in self.pairs:
                x.copy_(staged, non_blocking=True)


def behind_blocker(s, late, call, what="enqueue"):
    """blocker, event, the late inputs, then ``call()`` -- all on s, nothing synchronised until
    the call has returned.  Returns what the call returned, after ``s.synchronize()``."""
    late = Late(late)
    blocker = Blocker()
    torch.cuda.synchronize()
    ev = blocker.start(s)
    t0 = time.perf_counter()
    late.enqueue(s)
    r = call()
    dt = time.perf_counter() - t0
    running = not ev.query()
    s.synchronize()
    print(f"{what}: {dt * 1e3:.2f} ms of host time behind the blocker")
    assert running, STILL
    return r


def form_c(s, call):
    """``call()`` (with stream=s inside) while torch's current stream, the default one, is held by
    the blocker: the call returns while the blocker runs, whatever it reads back on s."""
    blocker = Blocker()
    torch.cuda.synchronize()
    ev = blocker.start(torch.cuda.current_stream())
    r = call()
    running = not ev.query()
    s.synchronize()
    assert running, STILL
    return r


# ---- the stages as jobs --------------------------------------------------------------------------

class Job:
    """One stage call: ``late`` are its input tensors (real contents, uploaded), ``call(stream)``
    makes the call and ``check(result)`` compares with the plain rules after a synchronisation.
    ``sized``: the variant that reads a count or a total back (out=None, max_frames=None)."""

    def __init__(self, name, late, call, check):
        self.name, self.late, self.call, self.check = name, late, call, check


@functools.lru_cache(maxsize=None)
def big_body_stream():
    """A small lifted-cap batch (16 connections of 24 frames) with bodies at and over the
    big-body threshold of small batches (16 KiB): verify's and stamp's nested ragged call takes
    its route passes.  One big body is corrupted, one small frame has a wrong CRC."""
    rng = np.random.default_rng(0xB16)
    conns = [[sc.frame(sc.rand_body(rng, int(rng.integers(0, 600)))) for _ in range(24)] for _ in range(16)]
    for c, n in ((2, 16384), (5, 16385), (9, 40005), (13, (300 << 10) + 1)):
        conns[c][7] = sc.frame(sc.rand_body(rng, n))
    f = conns[9][7]
    conns[9][7] = f[:20000] + bytes([f[20000] ^ 1]) + f[20001:]
    conns[11][3] = sc.frame(b"abc", crc=5)
    blob, offs, lens = sc.layout(rng, [b"".join(fr) for fr in conns])
    want = sc.expected(blob, offs, lens, "server", True, want_decoys=False)
    assert len(want[0]) == 16 * 24
    return blob, offs, lens, want


@functools.lru_cache(maxsize=None)
def two_tiles(role):
    return two_tile_conns(role)


@functools.lru_cache(maxsize=None)
def bad_crc(role):
    conns, _ = bad_crc_stream(role, 31 + (role == "client"))
    blob, offs, lens = sc.layout(np.random.default_rng(1), conns)
    return blob, offs, lens, sc.expected(blob, offs, lens, role, False, want_decoys=False)


def frames_of(kind, role):
    """(stream, frame offsets, lift_cap) of the two verify / stamp cases."""
    if kind == "mixed":
        blob, _, _, want = mixed_stream(role, False)
        return blob, want[0], False
    blob, _, _, want = big_body_stream()
    return blob, want[0], True


def verify_job(kind, role):
    blob, frames, lift = frames_of(kind, role)
    n = len(frames)
    want = [oracle.frame_verdict(blob, o, role, lift) for o in frames]
    d_blob, d_off = dev_bytes(blob), u64(frames)
    crc_big, crc = guarded_words(n, np.uint32, torch.int32)

    def call(stream):
        return rpc_amd.frames_verify(d_blob, d_off, role=role, lift_cap=lift, crc_out=crc, stream=stream)

    def check(r):
        assert host(r[0], np.uint8) == [w[0] for w in want], (kind, role)
        same_words(crc_big, np.uint32, [w[1] for w in want], (kind, role))
        assert len({w[0] for w in want}) >= (2 if lift else 4)

    return Job(f"verify {kind} {role}", [d_blob, d_off], call, check)


def stamp_job(kind, role):
    """The frames of the verify case re-stamped (version 3, type 9) with the lengths their
    headers claim: a body that leaves the stream reads MALFORMED, one over the cap in force
    TOO_LARGE, and neither is touched."""
    blob, frames, lift = frames_of(kind, role)
    control = sc.PING if role == "server" else sc.PONG
    lens = []
    for o in frames:  # (a heartbeat's length field claims the frames behind it: only where it will not be stamped)
        typ, n = struct.unpack_from(">HI", blob, o + 2)
        lens.append(n if typ != control or n > sc.MAX_BODY else 0)
    stamped, verdict = bytearray(blob), []
    for o, n in zip(frames, lens):
        if o + sc.HDR + n > len(blob):
            verdict.append(MALFORMED)
        elif n > sc.MAX_BODY and not lift:
            verdict.append(rpc_amd.FRAME_TOO_LARGE)
        else:
            verdict.append(rpc_amd.FRAME_OK)
            stamped[o:o + sc.HDR] = struct.pack(">HHII", 3, 9, n, zlib.crc32(blob[o + sc.HDR:o + sc.HDR + n]))
    big, d_blob = guarded(len(blob))
    d_blob.copy_(dev_bytes(blob))
    d_off, d_len = u64(frames), u32(lens)

    def call(stream):
        return rpc_amd.frames_stamp(d_blob, d_off, d_len, version=3, type_=9, lift_cap=lift, stream=stream)

    def check(r):
        assert host(r, np.uint8) == verdict, (kind, role)
        same_bytes(big, 0, bytes(stamped), (kind, role))
        assert rpc_amd.FRAME_OK in verdict and (lift or len(set(verdict)) == 3)

    return Job(f"stamp {kind} {role}", [d_blob, d_off, d_len], call, check)


def scan_job(kind, role, verify, sized=False, pad=9):
    if kind == "mixed":
        blob, offs, lens, want = mixed_stream(role, False)
    elif kind == "two_tiles":
        blob, offs, lens, want = two_tiles(role)
    else:
        blob, offs, lens, want = bad_crc(role)
    fo, fc, first, consumed, state = want[:5]
    n = len(fo)
    pad = 0 if sized else pad
    if verify:
        verdict, crc, state = fused_expect(blob, want, role, False)
    d_blob, d_off, d_len = dev_bytes(blob), u64(offs), u64(lens)

    def call(stream):
        if sized:
            return rpc_amd.frames_scan(d_blob, d_off, d_len, role=role, verify=verify, stream=stream)
        return rpc_amd.frames_scan(d_blob, d_off, d_len, role=role, max_frames=n + pad, verify=verify, stream=stream,
                                   read_count=False)

    def check(r):
        what = (kind, role, verify, sized)
        assert (r.nframes if sized else int(r.nframes.cpu()[0])) == n, what
        assert host(r.conn_first, np.uint64) == first, what
        assert host(r.frame_offsets, np.uint64) == fo + [len(blob)] * pad, what
        assert host(r.frame_conn, np.int32) == fc + [-1] * pad, what
        assert host(r.consumed, np.uint64) == consumed and host(r.state, np.uint8) == state, what
        if verify:
            assert host(r.verdict, np.uint8) == verdict + [MALFORMED] * pad, what
            assert host(r.crc, np.uint32) == crc + [0] * pad, what
            assert kind != "bad_crc" or verdict.count(rpc_amd.FRAME_NOT_REACHED) > 50

    return Job(f"scan {kind} {role}", [d_blob, d_off, d_len], call, check)


def pack_job(case, mis, sized=False):
    want = pc.expected(case.bodies, case.entries, case.conn_first, case.lift_cap, None)
    big, out = guarded(want.total, mis)
    typ, ver, off, ln = zip(*case.entries)
    d_typ, d_ver, d_off, d_len = u16(typ), u16(ver), u64(off), u32(ln)
    d_bodies = dev_bytes(case.bodies, 5 if mis else 0)
    d_conn = None if case.conn_first is None else u64(case.conn_first)

    def call(stream):
        return rpc_amd.frames_pack(d_bodies, d_off, d_len, types=d_typ, versions=d_ver, conn_first=d_conn,
                                   lift_cap=case.lift_cap, out=None if sized else out, stream=stream)

    def check(r):
        what = ("pack", case.name, mis, sized)
        assert total_of(r) == want.total, what
        if sized:
            assert r.stream.cpu().numpy().tobytes() == want.out, what
        else:
            same_bytes(big, mis, want.out, what)
        assert host(r.offsets, np.uint64) == want.offsets and host(r.verdict, np.uint8) == want.verdict, what
        assert host(r.crc, np.uint32) == want.crc, what
        if case.conn_first is not None:
            assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what

    return Job(f"pack {case.name} {mis}", [d_bodies, d_typ, d_ver, d_off, d_len, d_conn], call, check)


def heartbeat_job(n=700):
    """Nothing but heartbeats, the type a scalar: no body is looked at and the CRCs are cleared
    with a memset.  The versions arrive late."""
    vers = [1 + i % 5 for i in range(n)]
    conn = [0, 0, 300, n, n]
    want = pc.expected(b"", [(pc.PONG, v, 0, 0) for v in vers], conn)
    big, out = guarded(want.total, 3)
    d_ver, d_off, d_conn = u16(vers), u64([0] * n), u64(conn)

    def call(stream):
        return rpc_amd.frames_pack(None, d_off, None, type_=pc.PONG, versions=d_ver, conn_first=d_conn, out=out,
                                   stream=stream)

    def check(r):
        assert total_of(r) == want.total == 12 * n
        same_bytes(big, 3, want.out, "heartbeats")
        assert host(r.offsets, np.uint64) == want.offsets and host(r.verdict, np.uint8) == want.verdict
        assert host(r.crc, np.uint32) == [0] * n and host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first

    return Job("pack heartbeats", [d_ver, d_conn], call, check)


def unpack_job(case, mis, sized=False):
    want = uc.want_of(case, None)
    big, out = guarded(want.total, mis)
    off, v = zip(*case.entries)
    d_off, d_v = u64(off), u8(v)
    d_stream = dev_bytes(case.stream, 5 if mis else 0)
    d_conn = None if case.conn_first is None else u64(case.conn_first)

    def call(stream):
        return rpc_amd.frames_unpack(d_stream, d_off, d_v, role=case.role, lift_cap=case.lift_cap, nul=bool(case.nul),
                                     conn_first=d_conn, out=None if sized else out, stream=stream)

    def check(r):
        what = ("unpack", case.name, mis, sized)
        assert total_of(r) == want.total, what
        if sized:
            assert r.bodies.cpu().numpy().tobytes() == want.out, what
        else:
            same_bytes(big, mis, want.out, what)
        assert host(r.body_offsets, np.uint64) == want.body_offsets and host(r.body_lens, np.uint32) == want.body_lens, what
        assert host(r.reply_types, np.uint16) == want.reply_types and host(r.versions, np.uint16) == want.versions, what
        assert host(r.verdict, np.uint8) == want.verdict, what
        if case.conn_first is not None:
            assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what

    return Job(f"unpack {case.name} {mis}", [d_stream, d_off, d_v, d_conn], call, check)


def reply_job(case, mis, sized=False):
    want = rp.want_of(case, None)
    big, out = guarded(want.total, mis)
    cols = list(zip(*case.entries))
    d_ty = u16(cols[0]) if case.typed else None
    d_kind = u8(cols[1]) if case.kinded else None
    d_id, d_st = u32(cols[2]), (u32(cols[3]) if case.stated else None)
    d_voff, d_vlen = u64(cols[4]), u32(cols[5])
    d_values = dev_bytes(case.values, 5 if mis else 0)
    d_conn = None if case.conn_first is None else u64(case.conn_first)

    def call(stream):
        return rpc_amd.frames_reply(d_kind, d_id, d_values, d_voff, d_vlen, status=d_st, reply_types=d_ty,
                                    conn_first=d_conn, out=None if sized else out, stream=stream)

    def check(r):
        what = ("reply", case.name, mis, sized)
        assert total_of(r) == want.total, what
        if sized:
            assert r.bodies.cpu().numpy().tobytes() == want.out, what
        else:
            same_bytes(big, mis, want.out, what)
        assert host(r.body_offsets, np.uint64) == want.body_offsets and host(r.body_lens, np.uint32) == want.body_lens, what
        assert host(r.types, np.uint16) == want.types and host(r.status, np.uint8) == want.status, what
        if case.conn_first is not None:
            assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what

    return Job(f"reply {case.name} {mis}", [d_values, d_ty, d_kind, d_id, d_st, d_voff, d_vlen, d_conn], call, check)


def request_job(case, mis, sized=False):
    want = rq.want_of(case, None)
    big, out = guarded(want.total, mis)
    cols = list(zip(*case.entries))
    d_ty = u16(cols[0]) if case.typed else None
    d_m, d_id, d_poff, d_plen = u16(cols[1]), u32(cols[2]), u64(cols[3]), u32(cols[4])
    d_params = dev_bytes(case.params, 5 if mis else 0)
    d_conn = None if case.conn_first is None else u64(case.conn_first)
    table = rpc_amd.RouteTable(dev_bytes(case.table.names), u32(case.table.offsets), case.table.nmethods)

    def call(stream):
        return rpc_amd.frames_request(d_m, d_id, d_params, d_poff, d_plen, table, types=d_ty, conn_first=d_conn,
                                      out=None if sized else out, stream=stream)

    def check(r):
        what = ("request", case.name, mis, sized)
        assert total_of(r) == want.total, what
        if sized:
            assert r.bodies.cpu().numpy().tobytes() == want.out, what
        else:
            same_bytes(big, mis, want.out, what)
        assert host(r.body_offsets, np.uint64) == want.body_offsets and host(r.body_lens, np.uint32) == want.body_lens, what
        assert host(r.types, np.uint16) == want.types and host(r.status, np.uint8) == want.status, what
        if case.conn_first is not None:
            assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what

    return Job(f"request {case.name} {mis}", [d_params, d_ty, d_m, d_id, d_poff, d_plen, d_conn], call, check)


def carry_job(case, mis=0):
    want = cc.want_of(case)
    big, nxt = guarded(case.next_bytes, mis)
    off, ln, used, state = zip(*case.conns)
    d_off, d_len, d_used, d_state = u64(off), u64(ln), u64(used), (u8(state) if case.use_state else None)
    d_at = u64(case.next_at)
    d_nl = None if case.new_len is None else u64(case.new_len)
    d_stream = dev_bytes(case.stream, 5 if mis else 0)

    def call(stream):
        return rpc_amd.frames_carry(d_stream, d_off, d_len, d_used, d_state, nxt, d_at, room=case.room,
                                    new_lengths=d_nl, stream=stream)

    def check(r):
        what = ("carry", case.name, case.room, mis)
        same_bytes(big, mis, want.next, what)
        assert host(r.next_offsets, np.uint64) == want.next_off and host(r.next_lengths, np.uint64) == want.next_len, what
        assert host(r.status, np.uint8) == want.status and host(r.carried, np.uint64) == [want.carried], what

    return Job(f"carry {case.name}", [d_stream, d_off, d_len, d_used, d_state, d_at, d_nl], call, check)


@functools.lru_cache(maxsize=None)
def route_set(seed):
    """The route's case table plus 300 canonical and 300 mutated requests, with the plain rules'
    rows, groups and -- the route's own rows fed on -- args."""
    buf, entries, types = rc.case_entries(pad_front=3)
    more, ents = rc.back_to_back(rc.canonical_set(seed, 300) + rc.mutation_set(seed + 1, 300))
    entries = entries + [(o + len(buf), n) for o, n in ents]
    types = types + [rc.DATA] * len(ents)
    buf = buf + more
    routed = rc.route_entries(buf, entries, rc.IDL, types)
    order, first = rc.groups_of(routed, rc.IDL.nmethods)
    args = ac.args_entries(buf, [(o, n, r[0], r[1], r[3], r[4]) for (o, n), r in zip(entries, routed)], ac.IDL, 3)
    assert {r[0] for r in routed} == {rc.NONE, rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER, rc.RANGE}
    assert {a[0] for a in args} >= {ac.NONE, ac.OK, ac.INVALID}
    return buf, entries, types, routed, order, first, args


def args_rows(r, n):
    st, rs_ = host(r.status, np.uint8), host(r.reply_status, np.int32)
    sl = r.slots.cpu().numpy().view(np.uint64)
    return [(st[i], rs_[i], tuple(int(x) for x in sl[:, i])) for i in range(n)]


def route_args_job(seed, mis):
    """frames_route with its groups, and frames_args behind it on the route's own outputs."""
    buf, entries, types, routed, order, first, args = route_set(seed)
    n = len(entries)
    d_buf = dev_bytes(buf, mis)
    d_off, d_len, d_ty = u64([e[0] for e in entries]), u32([e[1] for e in entries]), u16(types)
    table = rpc_amd.route_table(rc.METHODS, device=DEV)
    methods = [(name.decode(), [(p.decode(), t) for p, t in params]) for name, params in ac.IDL_METHODS]
    assert [m for m, _ in methods] == [m.decode() for m in rc.METHODS]
    schema = rpc_amd.args_schema(methods, device=DEV)

    def call(stream):
        rt = rpc_amd.frames_route(d_buf, d_off, d_len, table, reply_types=d_ty, group=True, stream=stream)
        return rt, rpc_amd.frames_args(d_buf, d_off, d_len, rt, schema, stream=stream)

    def check(r):
        rt, a = r
        cols = [host(rt.kind, np.uint8), host(rt.method, np.uint16), host(rt.id, np.uint32),
                host(rt.params_off, np.uint32), host(rt.params_len, np.uint32)]
        assert list(zip(*cols)) == [tuple(w) for w in routed], ("route", seed, mis)
        gfirst = host(rt.group_first, np.uint32)
        assert gfirst == first and host(rt.order, np.uint32)[:first[-1]] == order, ("groups", seed, mis)
        assert args_rows(a, n) == args, ("args", seed, mis)

    return Job(f"route + args {seed}", [d_buf, d_off, d_len, d_ty], call, check)


@functools.lru_cache(maxsize=None)
def args_set():
    buf, entries = ac.case_entries(pad_front=3)
    more, ents = ac.back_to_back(ac.canonical_set(0x57, 300) + ac.mutation_set(0x58, 300))
    entries = entries + [(e[0] + len(buf),) + tuple(e[1:]) for e in ents]
    buf = buf + more
    return buf, entries, ac.args_entries(buf, entries, ac.IDL, ac.MAX_PARAMS)


def args_job(mis):
    """frames_args on its own case table (every status), the route's four columns late too."""
    buf, entries, want = args_set()
    n = len(entries)
    d_buf = dev_bytes(buf, mis)
    col = lambda j, f: f([e[j] for e in entries])  # noqa: E731
    d_off, d_len = col(0, u64), col(1, u32)
    route = rpc_amd.FrameRoute(col(2, u8), col(3, u16), None, col(4, u32), col(5, u32), None, None)
    w32 = lambda ws: u32(ws)  # noqa: E731
    schema = rpc_amd.ArgsSchema(w32(ac.IDL.first), u8(ac.IDL.types), w32(ac.IDL.noff),
                                to_dev(np.frombuffer(ac.IDL.names, dtype=np.uint8).copy()), ac.IDL.nmethods,
                                len(ac.IDL.types), 0)

    def call(stream):
        return rpc_amd.frames_args(d_buf, d_off, d_len, route, schema, width=ac.MAX_PARAMS, stream=stream)

    def check(r):
        assert args_rows(r, n) == want, ("args", mis)
        assert {w[0] for w in want} == {ac.NONE, ac.OK, ac.INVALID, ac.DEFER, ac.RANGE, ac.BAD_SCHEMA}

    return Job("args table", [d_buf, d_off, d_len, route.kind, route.method, route.params_off, route.params_len],
               call, check)


def resolve_job(name, call_, mis=0, pending=True):
    want = rs.resolve(call_.buf, call_.offs, call_.lens, call_.types, call_.pending if pending else [])
    d_buf = dev_bytes(call_.buf, mis)
    d_off, d_len = u64(call_.offs), u32(call_.lens)
    d_ty = None if call_.types is None else u16(call_.types)
    d_pend = u32(call_.pending) if pending else None

    def call(stream):
        return rpc_amd.frames_resolve(d_buf, d_off, d_len, d_pend, reply_types=d_ty, stream=stream)

    def check(r):
        nopen = int(r.nopen.cpu()[0])
        got = rs.Resolved(host(r.kind, np.uint8), host(r.id, np.uint32), host(r.result_off, np.uint32),
                          host(r.result_len, np.uint32), host(r.error_off, np.uint32), host(r.error_len, np.uint32),
                          host(r.slot, np.uint32), host(r.slot_entry, np.uint32), host(r.open, np.uint32)[:nopen])
        for field in rs.Resolved._fields:
            assert getattr(got, field) == getattr(want, field), ("resolve", name, field)

    return Job(f"resolve {name}", [d_buf, d_off, d_len, d_ty, d_pend], call, check)


def run_late(job):
    s = side_streams()[0]
    job.check(behind_blocker(s, job.late, lambda: job.call(s), job.name))


# ---- 2. every stage behind late inputs -------------------------------------------------------------

@pytest.mark.parametrize("role", ["server", "client"])
@pytest.mark.parametrize("kind", ["mixed", "big"])
def test_verify_behind_late_inputs(kind, role):
    run_late(verify_job(kind, role))


@pytest.mark.parametrize("role", ["server", "client"])
@pytest.mark.parametrize("kind", ["mixed", "big"])
def test_stamp_behind_late_inputs(kind, role):
    run_late(stamp_job(kind, role))


@pytest.mark.parametrize("kind,role,path,verify", [("mixed", "server", "serial", False), ("mixed", "client", "tiled", False),
                                                   ("bad_crc", "server", "serial", True), ("bad_crc", "client", "tiled", True),
                                                   ("two_tiles", "server", "tiled", False)])
def test_scan_behind_late_inputs(kind, role, path, verify):
    """Serial and tiled, the fused verify + reach pass, two-tile connections; ``max_frames`` from
    the plain walk's count (and 9 entries of padding), nothing read back."""
    rpc_amd.set_scan_path(path)
    try:
        run_late(scan_job(kind, role, verify))
    finally:
        rpc_amd.set_scan_path("auto")


@pytest.mark.parametrize("mis", [0, 5])
def test_pack_behind_late_inputs(mis):
    run_late(pack_job(pc.table_case(PACK_T, mis), mis))


def test_pack_heartbeats_behind_late_inputs():
    run_late(heartbeat_job())


@pytest.mark.parametrize("role", ["server", "client"])
@pytest.mark.parametrize("mis", [0, 5])
def test_unpack_behind_late_inputs(mis, role):
    run_late(unpack_job(uc.table_case(PACK_T, mis, role, 1), mis))


@pytest.mark.parametrize("mis", [0, 5])
def test_reply_behind_late_inputs(mis):
    run_late(reply_job(rp.table_case(PACK_T, mis), mis))


@pytest.mark.parametrize("mis", [0, 5])
def test_request_behind_late_inputs(mis):
    run_late(request_job(rq.table_case(PACK_T, mis), mis))


@pytest.mark.parametrize("room", [rpc_amd.CARRY_ROOM, LONG_ROOM])
@pytest.mark.parametrize("which", ["table", "corner"])
def test_carry_behind_late_inputs(which, room):
    """Both cases on the short route (room 1040) and on the long one, which leases workspace."""
    case = cc.table_case(room) if which == "table" else cc.corner_case(room)[0]
    run_late(carry_job(case, 9 if which == "corner" else 0))


@pytest.mark.parametrize("mis", [0, 5])
def test_route_and_args_behind_late_inputs(mis):
    run_late(route_args_job(0x60, mis))


def test_args_behind_late_inputs():
    run_late(args_job(3))


@pytest.mark.parametrize("name", ["collide_wrap", "three_replies", "npending_257", "types_and_ranges"])
def test_resolve_behind_late_inputs(name):
    """join_calls() with pending ids: the cells, slot_entry and nopen memsets run."""
    run_late(resolve_job(name, rs.join_calls()[name]))


def test_resolve_decode_only_behind_late_inputs():
    _, call = rs.case_call(nul=1)
    run_late(resolve_job("decode only", call, mis=5, pending=False))


# ---- 3. the wrapper's stream forms -------------------------------------------------------------------

FORM_JOBS = {
    "verify": lambda: verify_job("mixed", "server"),
    "stamp": lambda: stamp_job("mixed", "client"),
    "scan": lambda: scan_job("bad_crc", "server", True),
    "scan_sized": lambda: scan_job("bad_crc", "client", True, sized=True),
    "pack": lambda: pack_job(pc.table_case(PACK_T, 5), 5),
    "pack_sized": lambda: pack_job(pc.table_case(PACK_T, 0), 0, sized=True),
    "unpack": lambda: unpack_job(uc.table_case(PACK_T, 5, "server", 1), 5),
    "unpack_sized": lambda: unpack_job(uc.table_case(PACK_T, 0, "client", 0), 0, sized=True),
    "reply": lambda: reply_job(rp.table_case(PACK_T, 5), 5),
    "reply_sized": lambda: reply_job(rp.table_case(PACK_T, 0), 0, sized=True),
    "request": lambda: request_job(rq.table_case(PACK_T, 5), 5),
    "request_sized": lambda: request_job(rq.table_case(PACK_T, 0), 0, sized=True),
    "carry": lambda: carry_job(cc.table_case(LONG_ROOM)),
    "route_args": lambda: route_args_job(0x60, 5),
    "args": lambda: args_job(3),
    "resolve": lambda: resolve_job("collide_wrap", rs.join_calls()["collide_wrap"]),
}


@pytest.mark.parametrize("form", ["a", "b", "c"])
@pytest.mark.parametrize("name", sorted(FORM_JOBS))
def test_wrapper_stream_forms(name, form):
    """(a) inside ``with torch.cuda.stream(s)`` with ``stream=s``; (b) inside it with
    ``stream=None``; (c) ``stream=s`` alone while torch's current stream, the default one, is
    busy with the blocker.  The ``_sized`` jobs are the variants that read a total or a count
    back.  In (c) the call must return while the blocker still runs (nothing of the wrapper's
    waits for, or lands on, the current stream) and the total a kernel wrote on s must not be
    overwritten by a fill that the wrapper left on the current stream."""
    job = FORM_JOBS[name]()
    s = side_streams()[0]
    torch.cuda.synchronize()
    if form == "c":
        r = form_c(s, lambda: job.call(s))
    else:
        with torch.cuda.stream(s):
            r = job.call(s if form == "a" else None)
        s.synchronize()
    job.check(r)


def test_scan_counted_on_a_side_stream():
    """``max_frames`` with the count read back (the default): one synchronisation, of s alone."""
    blob, offs, lens, want = bad_crc("server")
    n = len(want[0])
    s = side_streams()[0]
    d_blob, d_off, d_len = dev_bytes(blob), u64(offs), u64(lens)
    r = form_c(s, lambda: rpc_amd.frames_scan(d_blob, d_off, d_len, max_frames=n + 1, stream=s))
    assert r.nframes == n and host(r.frame_offsets, np.uint64) == want[0] + [len(blob)]
    with pytest.raises(ValueError):
        rpc_amd.frames_scan(d_blob, d_off, d_len, max_frames=n - 1, stream=s)
    with pytest.raises(ValueError):
        rpc_amd.frames_scan(d_blob, d_off, d_len, stream=s, read_count=False)


def test_raw_stream_handle_serves_every_variant():
    """A holder of a raw hipStream_t (``cuda_stream`` and nothing else) serves the variants that
    read back too: the copy goes to that stream."""
    from test_gpu_parity import _RawStream, _hip_runtime
    s = _RawStream(_hip_runtime())
    try:
        for name in ("pack_sized", "scan_sized", "reply", "carry"):
            job = FORM_JOBS[name]()
            torch.cuda.synchronize()
            r = job.call(s)
            torch.cuda.synchronize()
            job.check(r)
    finally:
        torch.cuda.synchronize()
        s.destroy()


# ---- 4. a whole round on one stream, one synchronisation -------------------------------------------

class Round:
    pass


@functools.lru_cache(maxsize=None)
def server_round():
    """16 connections of about 6 KiB: requests of route_cases (with PINGs between them) in front
    of a random_conn with each of the four endings; and the plain rules chained: scan + verify ->
    unpack -> route -> args -> reply -> pack, and the carry."""
    w = Round()
    rng = np.random.default_rng(0x5E12)
    reqs = [b for b in rc.canonical_set(0x41, 300) + rc.mutation_set(0x42, 80) if len(b) <= sc.MAX_BODY]
    conns, k = [], 0
    for c in range(16):
        parts, size = [], 0
        while size < 3000:
            if k % 6 == 5:
                parts.append(sc.frame(typ=sc.PING, version=2))
            parts.append(sc.frame(reqs[k % len(reqs)], version=1 + k % 3))
            size += len(parts[-1])
            k += 1
        conns.append(b"".join(parts) + sc.random_conn(rng, 3000, "server", ending=sc.ENDINGS[c % 4]))
    w.blob, w.offs, w.lens = sc.layout(rng, conns)
    w.scan = sc.expected(w.blob, w.offs, w.lens, "server", False, want_decoys=False)
    fo, _, first, consumed, _ = w.scan[:5]
    w.verdict, w.crc, w.state = fused_expect(w.blob, w.scan, "server", False)
    w.pad = 5
    w.cap = len(fo) + w.pad
    w.first = first
    w.unpack = uc.expected(w.blob, fo + [len(w.blob)] * w.pad, w.verdict + [MALFORMED] * w.pad, first, "server", False, 1)
    entries = list(zip(w.unpack.body_offsets, w.unpack.body_lens))
    w.routed = rc.route_entries(w.unpack.out, entries, rc.IDL, w.unpack.reply_types)
    w.args = ac.args_entries(w.unpack.out, [(o, n, r[0], r[1], r[3], r[4]) for (o, n), r in zip(entries, w.routed)],
                             ac.IDL, 3)
    values, w.voff, w.vlen = bytearray(b"#"), [], []
    for i in range(w.cap):  # the handlers' fixed texts (a whole reply where the route defers)
        v = rp.error_body(0, -32700, rp.MESSAGES[-32700]) if w.routed[i][0] == rc.DEFER else b'{"r":[%d,"x"]}' % i
        w.voff.append(len(values))
        w.vlen.append(len(v))
        values += v + b"#"
    w.values = bytes(values)
    w.reply = rp.want_of(rp.Case("round", w.values, [(w.unpack.reply_types[i], w.routed[i][0], w.routed[i][2], w.args[i][1],
                                                      w.voff[i], w.vlen[i]) for i in range(w.cap)], first), None)
    w.pack = pc.expected(w.reply.out, [(w.reply.types[i], w.unpack.versions[i], w.reply.body_offsets[i],
                                        w.reply.body_lens[i]) for i in range(w.cap)], first)
    w.new_len = [64 + 16 * c for c in range(16)]
    at, w.next_bytes = rpc_amd.carry_slots(w.new_len)
    w.next_at = at.tolist()
    w.carry = cc.want_of(cc.Case("round", w.blob, list(zip(w.offs.tolist(), w.lens.tolist(), consumed, w.state)),
                                 w.next_bytes, w.next_at, w.new_len, rpc_amd.CARRY_ROOM))
    assert {r[0] for r in w.routed} >= {rc.NONE, rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER}
    assert {a[0] for a in w.args} >= {ac.NONE, ac.OK, ac.INVALID} and set(w.state) == {sc.OPEN, sc.CLOSED}
    assert set(w.reply.status) >= {rp.R_NONE, rp.R_RESULT, rp.R_ERROR, rp.R_RAW} and uc.PONG in w.reply.types
    assert sum(1 for t in w.carry.next_len if t) >= 8 and w.carry.carried > 0
    return w


def test_server_round_one_stream_one_synchronisation():
    """scan + verify -> unpack -> route -> args -> reply -> pack -> carry on one side stream behind
    late inputs, each stage fed the previous stage's device tensors, nothing read back before the
    one synchronisation: the packed bytes and the carried tails are those of the plain rules
    chained the same way.  (This is the pipeline whose enqueue time sizes the blocker.)"""
    w = server_round()
    s = side_streams()[0]
    d_blob, d_off, d_len = dev_bytes(w.blob, 3), u64(w.offs), u64(w.lens)
    table = rpc_amd.route_table(rc.METHODS, device=DEV)
    schema = rpc_amd.args_schema([(name.decode(), [(p.decode(), t) for p, t in params]) for name, params in ac.IDL_METHODS],
                                 device=DEV)
    d_values, d_voff, d_vlen = dev_bytes(w.values, 1), u64(w.voff), u32(w.vlen)
    d_at, d_nl = u64(w.next_at), u64(w.new_len)
    u_big, u_out = guarded(w.unpack.total, 5)
    r_big, r_out = guarded(w.reply.total, 9)
    p_big, p_out = guarded(w.pack.total, 7)
    n_big, nxt = guarded(w.next_bytes, 0)

    def round_():
        f = rpc_amd.frames_scan(d_blob, d_off, d_len, role="server", max_frames=w.cap, verify=True, stream=s,
                                read_count=False)
        u = rpc_amd.frames_unpack(d_blob, f.frame_offsets, f.verdict, role="server", nul=True, conn_first=f.conn_first,
                                  out=u_out, stream=s)
        rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, table, reply_types=u.reply_types, stream=s)
        a = rpc_amd.frames_args(u.bodies, u.body_offsets, u.body_lens, rt, schema, stream=s)
        rep = rpc_amd.frames_reply(rt.kind, rt.id, d_values, d_voff, d_vlen, status=a.reply_status,
                                   reply_types=u.reply_types, conn_first=f.conn_first, out=r_out, stream=s)
        p = rpc_amd.frames_pack(rep.bodies, rep.body_offsets, rep.body_lens, types=rep.types, versions=u.versions,
                                conn_first=f.conn_first, out=p_out, stream=s)
        k = rpc_amd.frames_carry(d_blob, d_off, d_len, f.consumed, f.state, nxt, d_at, new_lengths=d_nl, stream=s)
        return f, u, rt, a, rep, p, k

    f, u, rt, a, rep, p, k = behind_blocker(s, [d_blob, d_off, d_len], round_, "server round")
    # what the issue asks for: the packed bytes and the carried tails
    same_bytes(p_big, 7, w.pack.out, "packed bytes")
    same_bytes(n_big, 0, w.carry.next, "carried tails")
    assert host(p.conn_bytes_first, np.uint64) == w.pack.conn_bytes_first and total_of(p) == w.pack.total
    assert host(k.next_offsets, np.uint64) == w.carry.next_off and host(k.next_lengths, np.uint64) == w.carry.next_len
    assert host(k.status, np.uint8) == w.carry.status and host(k.carried, np.uint64) == [w.carry.carried]
    # and every stage on the way, so that a failure names its stage
    assert int(f.nframes.cpu()[0]) == w.cap - w.pad and host(f.verdict, np.uint8) == w.verdict + [MALFORMED] * w.pad
    assert host(f.state, np.uint8) == w.state
    same_bytes(u_big, 5, w.unpack.out, "unpacked bodies")
    assert host(u.reply_types, np.uint16) == w.unpack.reply_types and host(u.versions, np.uint16) == w.unpack.versions
    assert list(zip(host(rt.kind, np.uint8), host(rt.method, np.uint16), host(rt.id, np.uint32),
                    host(rt.params_off, np.uint32), host(rt.params_len, np.uint32))) == [tuple(r) for r in w.routed]
    assert args_rows(a, w.cap) == w.args
    same_bytes(r_big, 9, w.reply.out, "reply bodies")
    assert host(rep.types, np.uint16) == w.reply.types and host(rep.status, np.uint8) == w.reply.status
    assert host(p.verdict, np.uint8) == w.pack.verdict and host(p.crc, np.uint32) == w.pack.crc


@functools.lru_cache(maxsize=None)
def client_round():
    """240 entries on 8 connections (the seven methods with the params the client stubs build,
    some calls without params, a PONG as every tenth entry, the edge ids among distinct 32-bit
    ids) and the plain rules chained: request -> pack -> the wire as the peer's stream -> scan +
    verify as a client -> unpack -> resolve against the request's ids."""
    import json
    import random
    w = Round()
    rng = random.Random(0xC11E)
    n, nconn = 240, 8
    w.ids = rng.sample(range(1, 1 << 32), n)
    w.ids[:3] = [0, 4294967295, 2147483648]
    w.types, w.method, params, w.poff, w.plen = [], [], bytearray(b"#"), [], []
    for i in range(n):
        pong = i % 10 == 9
        text = b"" if pong or i % 9 == 8 else json.dumps(rc.canonical_params(rng, i % 7), separators=(",", ":"),
                                                          ensure_ascii=False).encode()
        w.types.append(rq.PONG if pong else rq.DATA)
        w.method.append(i % 7)
        w.poff.append(len(params))
        w.plen.append(len(text))
        params += text + b"#"
    w.params = bytes(params)
    w.conn = [c * (n // nconn) for c in range(nconn)] + [n]
    w.table = rq.make_table(rc.METHODS)
    w.request = rq.want_of(rq.Case("round", w.params, w.table, list(zip(w.types, w.method, w.ids, w.poff, w.plen)), w.conn),
                           None)
    w.pack = pc.expected(w.request.out, [(w.request.types[i], 1, w.request.body_offsets[i], w.request.body_lens[i])
                                         for i in range(n)], w.conn)
    cbf = w.pack.conn_bytes_first
    w.scan = sc.expected(w.pack.out, np.array(cbf[:-1], dtype=np.uint64), np.diff(np.array(cbf, dtype=np.uint64)),
                         "client", False, want_decoys=False)
    fo, _, first, _, _ = w.scan[:5]
    assert len(fo) == n and first == w.conn
    w.verdict, w.crc, w.state = fused_expect(w.pack.out, w.scan, "client", False)
    w.pad = 3
    w.cap = n + w.pad
    w.unpack = uc.expected(w.pack.out, fo + [len(w.pack.out)] * w.pad, w.verdict + [MALFORMED] * w.pad, first, "client",
                           False, 1)
    w.resolve = rs.resolve(w.unpack.out, w.unpack.body_offsets, w.unpack.body_lens, w.unpack.reply_types, w.ids)
    calls = [i for i in range(n) if w.types[i] == rq.DATA]
    assert [i for i, kd in enumerate(w.resolve.kind) if kd == rs.MATCHED] == calls
    assert w.resolve.open == [i for i in range(n) if w.types[i] != rq.DATA] and set(w.state) == {sc.OPEN}
    return w


def test_client_round_one_stream_one_synchronisation():
    """request -> pack -> (the packed bytes as the peer's stream) scan + verify -> unpack -> resolve
    against the request's ids, on one side stream behind late inputs, one synchronisation."""
    w = client_round()
    n = len(w.ids)
    s = side_streams()[0]
    d_ty, d_m, d_id = u16(w.types), u16(w.method), u32(w.ids)
    d_params, d_poff, d_plen, d_conn = dev_bytes(w.params, 7), u64(w.poff), u32(w.plen), u64(w.conn)
    table = rpc_amd.route_table(rc.METHODS, device=DEV)
    q_big, q_out = guarded(w.request.total, 3)
    p_big, p_out = guarded(w.pack.total, 11)
    u_big, u_out = guarded(w.unpack.total, 5)

    def round_():
        q = rpc_amd.frames_request(d_m, d_id, d_params, d_poff, d_plen, table, types=d_ty, conn_first=d_conn, out=q_out,
                                   stream=s)
        p = rpc_amd.frames_pack(q.bodies, q.body_offsets, q.body_lens, types=q.types, conn_first=d_conn, out=p_out,
                                stream=s)
        with on(s):
            cbf = p.conn_bytes_first
            at, ln = cbf[:-1].contiguous(), (cbf[1:] - cbf[:-1]).contiguous()
        f = rpc_amd.frames_scan(p.stream, at, ln, role="client", max_frames=w.cap, verify=True, stream=s, read_count=False)
        u = rpc_amd.frames_unpack(p.stream, f.frame_offsets, f.verdict, role="client", nul=True, conn_first=f.conn_first,
                                  out=u_out, stream=s)
        x = rpc_amd.frames_resolve(u.bodies, u.body_offsets, u.body_lens, d_id, reply_types=u.reply_types, stream=s)
        return q, p, f, u, x, (at, ln)

    with on(s):  # (the glue's two kernels, loaded before the blocker starts)
        (d_conn[1:] - d_conn[:-1]).contiguous()
    s.synchronize()
    q, p, f, u, x, _ = behind_blocker(s, [d_ty, d_m, d_id, d_params, d_poff, d_plen, d_conn], round_, "client round")
    nopen = int(x.nopen.cpu()[0])
    got = rs.Resolved(host(x.kind, np.uint8), host(x.id, np.uint32), host(x.result_off, np.uint32),
                      host(x.result_len, np.uint32), host(x.error_off, np.uint32), host(x.error_len, np.uint32),
                      host(x.slot, np.uint32), host(x.slot_entry, np.uint32), host(x.open, np.uint32)[:nopen])
    for field in rs.Resolved._fields:
        assert getattr(got, field) == getattr(w.resolve, field), field
    same_bytes(q_big, 3, w.request.out, "request bodies")
    same_bytes(p_big, 11, w.pack.out, "packed bytes")
    same_bytes(u_big, 5, w.unpack.out, "unpacked bodies")
    assert int(f.nframes.cpu()[0]) == n and host(f.verdict, np.uint8) == w.verdict + [MALFORMED] * w.pad
    assert host(f.conn_first, np.uint64) == w.conn and host(f.state, np.uint8) == w.state
    assert host(u.reply_types, np.uint16) == w.unpack.reply_types


# ---- 6. two streams, interleaved ---------------------------------------------------------------------

def interleaved_jobs():
    """Two lists with different cases of the same stages, so that equal-sized workspace blocks
    change hands between the streams."""
    join = rs.join_calls()
    a = [verify_job("mixed", "server"), stamp_job("mixed", "server"), scan_job("bad_crc", "server", True),
         pack_job(pc.table_case(PACK_T, 0), 0), unpack_job(uc.table_case(PACK_T, 0, "server", 1), 0),
         reply_job(rp.table_case(PACK_T, 0), 0), request_job(rq.table_case(PACK_T, 0), 0),
         carry_job(cc.table_case(LONG_ROOM)), route_args_job(0x60, 0), resolve_job("collide_wrap", join["collide_wrap"])]
    b = [verify_job("mixed", "client"), stamp_job("big", "server"), scan_job("bad_crc", "client", True),
         pack_job(pc.table_case(PACK_T, 5), 5), unpack_job(uc.table_case(PACK_T, 5, "client", 0), 5),
         reply_job(rp.table_case(PACK_T, 5), 5), request_job(rq.table_case(PACK_T, 5), 5),
         carry_job(cc.corner_case(LONG_ROOM)[0], 9), route_args_job(0x70, 5),
         resolve_job("three_replies", join["three_replies"])]
    return a, b


def test_two_streams_interleaved():
    """Two side streams, each behind a blocker of its own; the stage calls alternate between them
    for three passes (the lists swap streams each pass, so that a block one stream released is
    leased by the other), nothing synchronised until everything is enqueued on both."""
    s1, s2 = side_streams()
    passes = []
    for k in range(3):
        a, b = interleaved_jobs()
        sa, sb = (s1, s2) if k % 2 == 0 else (s2, s1)
        passes.append([(j, sa, Late(j.late)) for j in a] + [(j, sb, Late(j.late)) for j in b])
    b1, b2 = Blocker(), Blocker()
    torch.cuda.synchronize()
    ev1, ev2 = b1.start(s1), b2.start(s2)
    t0 = time.perf_counter()
    results = []
    for jobs in passes:
        for _, s, late in jobs:
            late.enqueue(s)
        half = len(jobs) // 2
        for x, y in zip(jobs[:half], jobs[half:]):  # one call on one stream, the next on the other
            results.append((x[0], x[0].call(x[1])))
            results.append((y[0], y[0].call(y[1])))
    dt = time.perf_counter() - t0
    running = not ev1.query() and not ev2.query()
    s1.synchronize()
    s2.synchronize()
    print(f"interleaved: {dt * 1e3:.2f} ms of host time behind the blockers, {len(results)} stage calls")
    assert running, STILL
    for job, r in results:
        job.check(r)
    assert rpc_amd.device_status() == 0
