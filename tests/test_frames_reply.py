"""Frame reply on the GPU (rpc_frames_reply_device): JSON-RPC reply bodies from
id + value, against the plain Python rules of tests/reply_cases.py byte for byte and word for
word, and -- route -> reply -> pack -> scan + verify -> unpack -- a round trip that brings the
reply bodies back unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import reply_cases as rp  # noqa: E402
import route_cases as rc  # noqa: E402
from test_frames_unpack import DEV, GUARD, T, dev_bytes, host, i64, to_dev  # noqa: E402


def entry_tensors(case):
    """(types, kind, id, status, value offsets, value lengths); None where the case gives none."""
    cols = list(zip(*case.entries))
    return (to_dev(np.asarray(cols[0], dtype=np.uint16).view(np.int16)) if case.typed else None,
            to_dev(np.asarray(cols[1], dtype=np.uint8)) if case.kinded else None,
            to_dev(np.asarray(cols[2], dtype=np.uint32).view(np.int32)),
            to_dev(np.asarray(cols[3], dtype=np.int32)) if case.stated else None,
            i64(cols[4]), to_dev(np.asarray(cols[5], dtype=np.uint32).view(np.int32)))


def same_words(r, want, what, conn=True):
    assert host(r.body_offsets, np.uint64) == want.body_offsets, what
    assert host(r.body_lens, np.uint32) == want.body_lens, what
    assert host(r.types, np.uint16) == want.types, what
    assert host(r.status, np.uint8) == want.status, what
    total = r.total if isinstance(r.total, int) else int(r.total.cpu()[0])
    assert total == want.total, what
    if conn:
        assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what


def reply_into_guarded(case, cap, src_mis=0, out_mis=0):
    """Builds `case` into a slice of a larger 0xA5-filled tensor and checks everything against
    reply_cases.want_of: the output byte for byte (0xA5 outside every written entry), the guard
    bytes on both sides and beyond out_cap, every per-entry word, and that the inputs are left
    alone."""
    want = rp.want_of(case, cap)
    nb = len(want.out)
    big = torch.full((GUARD + out_mis + nb + GUARD,), rp.FILL, dtype=torch.uint8, device=DEV)
    out = big[GUARD + out_mis:GUARD + out_mis + nb]
    assert nb == 0 or out.data_ptr() % 16 == out_mis
    ty, kind, rid, st, voff, vlen = entry_tensors(case)
    values = dev_bytes(case.values, src_mis)
    assert len(case.values) == 0 or values.data_ptr() % 16 == src_mis
    r = rpc_amd.frames_reply(kind, rid, values, voff, vlen, status=st, reply_types=ty,
                             conn_first=None if case.conn_first is None else i64(case.conn_first), out=out)
    what = (case.name, cap, src_mis, out_mis)
    got = big.cpu().numpy()
    lead = GUARD + out_mis
    assert (got[:lead] == rp.FILL).all(), what
    assert (got[lead + nb:] == rp.FILL).all(), what
    assert got[lead:lead + nb].tobytes() == want.out, what
    same_words(r, want, what, conn=case.conn_first is not None)
    if case.typed:
        assert host(ty, np.uint16) == [e[0] for e in case.entries], what
    return want


@pytest.mark.parametrize("src_mis,out_mis", [(0, 0), (5, 9)])
def test_case_table(src_mis, out_mis):
    """The emulator's table (tests/test_reply_emu.py) at the kernels' tile: every id beside every
    code, every kind beside every reply type, every alignment pair at seven lengths in the
    three copying forms, a value of three tiles, values outside the buffer, 20,000 one-byte RAW
    entries (more than the LDS staging holds), 5,000 zero-size entries between two results."""
    case = rp.table_case(T, out_mis)
    want = reply_into_guarded(case, None, src_mis, out_mis)
    assert want.total < (1 << 20) and max(want.body_lens) > 2 * T
    assert sum(1 for c in want.chunks if len(c) == 1) >= rp.RAW_RUN > 1536
    assert set(want.status) == {rp.R_NONE, rp.R_RESULT, rp.R_ERROR, rp.R_RAW, rp.R_RANGE}


def test_capacity_nulls_and_single_entries():
    """out_cap inside an entry's prefix, its value, its suffix, exactly at its end and 0;
    d_reply_types, d_kind and d_status each NULL; n = 1 of each form; an empty values buffer;
    and the call that sizes itself."""
    for case in rp.small_cases(T):
        for cap in case.out_caps:
            reply_into_guarded(case, cap, 3, 11)
    case = rp.small_cases(T)[0]
    full = rp.want_of(case, None)
    ty, kind, rid, st, voff, vlen = entry_tensors(case)
    a = rpc_amd.frames_reply(kind, rid, dev_bytes(case.values), voff, vlen, status=st, reply_types=ty,
                             conn_first=i64(case.conn_first))  # layout-only first
    assert a.total == full.total == a.bodies.numel()
    assert a.bodies.cpu().numpy().tobytes() == full.out
    same_words(a, full, "sized by itself")


def test_bodies_at_the_32_bit_edge():
    """Layout-only, on a values buffer that is only claimed (nothing of it is read): a body of
    exactly 0xFFFFFFFF bytes is laid out, one byte more reads RANGE, and the offsets are 64-bit
    sums."""
    for case in rp.wide_cases():
        want = rp.want_of(case, 0)
        ty, kind, rid, st, voff, vlen = entry_tensors(case)
        n = len(case.entries)
        dummy = torch.zeros(16, dtype=torch.uint8, device=DEV)
        offs, lens = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        types, state = torch.empty(n, dtype=torch.int16, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
        conn = i64(case.conn_first)
        cbf, total = torch.empty(conn.numel(), dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
        code = rpc_amd._lib.rpc_frames_reply_device(kind.data_ptr(), rid.data_ptr(), st.data_ptr(), ty.data_ptr(), n,
                                                    dummy.data_ptr(), case.values, voff.data_ptr(), vlen.data_ptr(),
                                                    conn.data_ptr(), conn.numel() - 1, None, 0, offs.data_ptr(),
                                                    lens.data_ptr(), types.data_ptr(), state.data_ptr(), cbf.data_ptr(),
                                                    total.data_ptr(), None)
        assert code == 0
        torch.cuda.synchronize()
        r = rpc_amd.FrameReply(None, offs, lens, types, state, cbf, total)
        same_words(r, want, case.name)
        assert want.total > (1 << 33) and want.status.count(rp.R_RANGE) == 4


def test_types_in_place():
    """d_types_out aliasing d_reply_types (through the C-ABI) gives what separate arrays give."""
    case = rp.small_cases(T)[0]
    cap = rp.want_of(case, None).total - 1  # the last body does not fit: its type changes
    want = rp.want_of(case, cap)
    ty, kind, rid, st, voff, vlen = entry_tensors(case)
    values = dev_bytes(case.values, 1)
    out_a = torch.full((cap,), rp.FILL, dtype=torch.uint8, device=DEV)
    sep = rpc_amd.frames_reply(kind, rid, values, voff, vlen, status=st, reply_types=ty, out=out_a)
    out = torch.full((cap,), rp.FILL, dtype=torch.uint8, device=DEV)
    n = len(case.entries)
    state = torch.empty(n, dtype=torch.uint8, device=DEV)
    code = rpc_amd._lib.rpc_frames_reply_device(kind.data_ptr(), rid.data_ptr(), st.data_ptr(), ty.data_ptr(), n,
                                                values.data_ptr(), values.numel(), voff.data_ptr(), vlen.data_ptr(), None, 0,
                                                out.data_ptr(), out.numel(), None, None, ty.data_ptr(), state.data_ptr(),
                                                None, None, None)
    assert code == 0
    torch.cuda.synchronize()
    assert host(ty, np.uint16) == want.types == host(sep.types, np.uint16)
    assert host(state, np.uint8) == want.status
    assert [i for i, e in enumerate(case.entries) if e[0] != want.types[i]] == [5]
    assert torch.equal(out, out_a) and out.cpu().numpy().tobytes() == want.out


def test_no_connections_and_no_entries():
    """nconn == 0, and n == 0 with d_total (and a CSR): everything reads 0."""
    case = rp.small_cases(T)[0]
    ty, kind, rid, st, voff, vlen = entry_tensors(case)
    want = rp.want_of(case._replace(conn_first=[0]), None)
    r = rpc_amd.frames_reply(kind, rid, dev_bytes(case.values), voff, vlen, status=st, reply_types=ty, conn_first=i64([0]))
    same_words(r, want, "nconn 0")
    assert host(r.conn_bytes_first, np.uint64) == [want.total]
    e64, e32 = torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV)
    e = rpc_amd.frames_reply(None, e32, dev_bytes(case.values), e64, e32, conn_first=i64([0, 0, 0]))
    assert e.total == 0 and e.bodies.numel() == 0 and host(e.conn_bytes_first, np.uint64) == [0, 0, 0]
    out = torch.full((32,), rp.FILL, dtype=torch.uint8, device=DEV)
    e = rpc_amd.frames_reply(None, e32, dev_bytes(case.values), e64, e32, out=out)
    assert int(e.total.cpu()[0]) == 0 and (out == rp.FILL).all()


def test_round_trip_through_route_pack_scan_and_unpack():
    """route -> reply -> pack -> scan + verify -> unpack: the reply bodies come back unchanged,
    every frame reads OK, and each body is the rules' for the route's kind and id."""
    bodies = rc.canonical_set(11, 180) + rc.mutation_set(12, 60)
    buf, entries = rc.back_to_back(bodies)
    routed = rc.route_entries(buf, entries)
    assert {r[0] for r in routed} == {rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER}
    off, ln = zip(*entries)
    table = rpc_amd.route_table(rc.METHODS)
    rt = rpc_amd.frames_route(dev_bytes(buf), i64(off), to_dev(np.asarray(ln, dtype=np.int32)), table, group=False)
    # the handlers' verdicts: a result, a fixed error, a custom error; the host's whole reply for a deferred entry
    values, voff, vlen, status, want = bytearray(), [], [], [], []
    for i, (kind, m, rid, _, _) in enumerate(routed):
        s, v = 0, b""
        if kind == rc.CALL:
            s = (0, 0, -32602, -7)[i % 4]
            v = (b'"v%d"' % i, b"%d" % i, b"", b"no %d" % i)[i % 4]
        elif kind == rc.DEFER:
            v = rp.error_body(0, -32700, rp.MESSAGES[-32700])
        voff.append(len(values))
        vlen.append(len(v))
        status.append(s)
        values += v + b"#"
        want.append(rp.rule(values, len(values), False, rp.DATA, kind, rid, s, voff[-1], len(v))[0])
    r = rpc_amd.frames_reply(rt.kind, rt.id, dev_bytes(values, 3), i64(voff), to_dev(np.asarray(vlen, dtype=np.int32)),
                             status=to_dev(np.asarray(status, dtype=np.int32)), conn_first=i64([0, 100, len(bodies)]))
    assert r.total == sum(map(len, want)) and all(want)
    built = r.bodies.cpu().numpy().tobytes()
    at = host(r.body_offsets, np.uint64)
    assert [built[a:a + len(w)] for a, w in zip(at, want)] == want
    assert set(host(r.status, np.uint8)) == {rp.R_RESULT, rp.R_ERROR, rp.R_RAW}
    p = rpc_amd.frames_pack(r.bodies, r.body_offsets, r.body_lens, types=r.types, conn_first=i64([0, 100, len(bodies)]))
    cbf = host(p.conn_bytes_first, np.uint64)
    s = rpc_amd.frames_scan(p.stream, i64(cbf[:2]), i64([cbf[1] - cbf[0], cbf[2] - cbf[1]]), role="client", verify=True)
    assert s.nframes == len(bodies)
    assert set(host(s.verdict, np.uint8)[:s.nframes]) == {rpc_amd.FRAME_OK}
    u = rpc_amd.frames_unpack(p.stream, s.frame_offsets, s.verdict, role="client", nul=False)
    assert u.total == r.total and torch.equal(u.bodies, r.bodies)
    assert host(u.body_lens, np.uint32)[:s.nframes] == host(r.body_lens, np.uint32)
