"""Frame request on the GPU (rpc_frames_request_device): JSON-RPC request bodies
from method index + params + id, against the plain Python rules of tests/request_cases.py byte
for byte and word for word; the inverse loop request -> pack -> scan + verify -> unpack -> route
that gives every input back; and the closed loop on through reply -> pack -> scan + verify ->
unpack -> resolve with the request's ids as the pending ids."""
import json
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import request_cases as rq  # noqa: E402
import route_cases as rtc  # noqa: E402
from test_frames_unpack import DEV, GUARD, T, dev_bytes, host, i64, to_dev  # noqa: E402


def i32(a):
    return to_dev(np.asarray(a, dtype=np.uint32).view(np.int32))


def i16(a):
    return to_dev(np.asarray(a, dtype=np.uint16).view(np.int16))


def dev_table(tb):
    """A RouteTable with the case's words as they are (route_table makes only sound ones)."""
    return rpc_amd.RouteTable(dev_bytes(tb.names), i32(tb.offsets), tb.nmethods)


def entry_tensors(case):
    """(types, method, id, params offsets, params lengths); types None where the case gives none."""
    cols = list(zip(*case.entries))
    return (i16(cols[0]) if case.typed else None, i16(cols[1]), i32(cols[2]), i64(cols[3]), i32(cols[4]))


def same_words(r, want, what, conn=True):
    assert host(r.body_offsets, np.uint64) == want.body_offsets, what
    assert host(r.body_lens, np.uint32) == want.body_lens, what
    assert host(r.types, np.uint16) == want.types, what
    assert host(r.status, np.uint8) == want.status, what
    total = r.total if isinstance(r.total, int) else int(r.total.cpu()[0])
    assert total == want.total, what
    if conn:
        assert host(r.conn_bytes_first, np.uint64) == want.conn_bytes_first, what


def request_into_guarded(case, cap, src_mis=0, out_mis=0):
    """Builds `case` into a slice of a larger 0xA5-filled tensor and checks everything against
    request_cases.want_of: the output byte for byte (0xA5 outside every written entry), the
    guard bytes on both sides and beyond out_cap, every per-entry word, and that the inputs are
    left alone."""
    want = rq.want_of(case, cap)
    nb = len(want.out)
    big = torch.full((GUARD + out_mis + nb + GUARD,), rq.FILL, dtype=torch.uint8, device=DEV)
    out = big[GUARD + out_mis:GUARD + out_mis + nb]
    assert nb == 0 or out.data_ptr() % 16 == out_mis
    ty, method, rid, poff, plen = entry_tensors(case)
    params = dev_bytes(case.params, src_mis)
    assert len(case.params) == 0 or params.data_ptr() % 16 == src_mis
    r = rpc_amd.frames_request(method, rid, params, poff, plen, dev_table(case.table), types=ty,
                               conn_first=None if case.conn_first is None else i64(case.conn_first), out=out)
    what = (case.name, cap, src_mis, out_mis)
    got = big.cpu().numpy()
    lead = GUARD + out_mis
    assert (got[:lead] == rq.FILL).all(), what
    assert (got[lead + nb:] == rq.FILL).all(), what
    assert got[lead:lead + nb].tobytes() == want.out, what
    same_words(r, want, what, conn=case.conn_first is not None)
    if case.typed:
        assert host(ty, np.uint16) == [e[0] for e in case.entries], what
    return want


@pytest.mark.parametrize("src_mis,out_mis", [(0, 0), (5, 9)])
def test_case_table(src_mis, out_mis):
    """The emulator's table (tests/test_request_emu.py) at the kernels' tile: every id beside
    every name, every method class beside every type, every alignment pair at lengths 0-33 as a
    call and raw, a value of three tiles, values outside the buffer, 20,000 one-byte RAW entries
    (more than the LDS staging holds), 5,000 zero-size entries between two requests."""
    case = rq.table_case(T, out_mis)
    want = request_into_guarded(case, None, src_mis, out_mis)
    assert want.total < (1 << 21) and max(want.body_lens) > 2 * T
    assert sum(1 for ln, s in zip(want.body_lens, want.status) if ln == 1 and s == rq.Q_RAW) >= rq.RAW_RUN > 1536
    assert set(want.status) == {rq.Q_NONE, rq.Q_CALL, rq.Q_RAW, rq.Q_BAD_METHOD, rq.Q_RANGE}


def test_capacity_nulls_and_single_entries():
    """out_cap inside an entry's front, its name, its value, its `,"id":` tail, exactly at its
    end and 0 (a caller's out with too little room); d_types NULL; n = 1 of each kind and n =
    257; an empty params buffer; an empty table; a 4096-byte name that is the whole table, across
    a tile edge; and the call that sizes itself (the layout-only call first)."""
    for case in rq.small_cases(T) + [rq.long_name_case(T, 11)]:
        for cap in case.out_caps:
            request_into_guarded(case, cap, 3, 11)
    case = rq.small_cases(T)[0]
    full = rq.want_of(case, None)
    ty, method, rid, poff, plen = entry_tensors(case)
    a = rpc_amd.frames_request(method, rid, dev_bytes(case.params), poff, plen, dev_table(case.table), types=ty,
                               conn_first=i64(case.conn_first))  # layout-only first
    assert a.total == full.total == a.bodies.numel()
    assert a.bodies.cpu().numpy().tobytes() == full.out
    same_words(a, full, "sized by itself")


def test_bodies_at_the_32_bit_edge():
    """Layout-only, on a params buffer that is only claimed (nothing of it is read): a body of
    exactly 0xFFFFFFFF bytes is laid out, one byte more reads RANGE, and the offsets are 64-bit
    sums."""
    for case in rq.wide_cases():
        want = rq.want_of(case, 0)
        ty, method, rid, poff, plen = entry_tensors(case)
        tb = dev_table(case.table)
        n = len(case.entries)
        dummy = torch.zeros(16, dtype=torch.uint8, device=DEV)
        offs, lens = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        types, state = torch.empty(n, dtype=torch.int16, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
        conn = i64(case.conn_first)
        cbf, total = torch.empty(conn.numel(), dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
        code = rpc_amd._lib.rpc_frames_request_device(method.data_ptr(), rid.data_ptr(), ty.data_ptr(), n,
                                                      tb.names.data_ptr(), tb.names.numel(), tb.offsets.data_ptr(),
                                                      tb.nmethods, dummy.data_ptr(), case.params, poff.data_ptr(),
                                                      plen.data_ptr(), conn.data_ptr(), conn.numel() - 1, None, 0,
                                                      offs.data_ptr(), lens.data_ptr(), types.data_ptr(), state.data_ptr(),
                                                      cbf.data_ptr(), total.data_ptr(), None)
        assert code == 0
        torch.cuda.synchronize()
        r = rpc_amd.FrameRequest(None, offs, lens, types, state, cbf, total)
        same_words(r, want, case.name)
        assert want.total > (1 << 33) and want.status == rq.WIDE_STATUS and want.body_lens == rq.WIDE_LENS


def test_types_in_place():
    """d_types_out aliasing d_types (through the C-ABI) gives what separate arrays give."""
    case = rq.small_cases(T)[0]
    cap = rq.want_of(case, None).total - 1  # the last body does not fit: its type changes
    want = rq.want_of(case, cap)
    ty, method, rid, poff, plen = entry_tensors(case)
    tb = dev_table(case.table)
    params = dev_bytes(case.params, 1)
    out_a = torch.full((cap,), rq.FILL, dtype=torch.uint8, device=DEV)
    sep = rpc_amd.frames_request(method, rid, params, poff, plen, tb, types=ty, out=out_a)
    out = torch.full((cap,), rq.FILL, dtype=torch.uint8, device=DEV)
    n = len(case.entries)
    state = torch.empty(n, dtype=torch.uint8, device=DEV)
    code = rpc_amd._lib.rpc_frames_request_device(method.data_ptr(), rid.data_ptr(), ty.data_ptr(), n, tb.names.data_ptr(),
                                                  tb.names.numel(), tb.offsets.data_ptr(), tb.nmethods, params.data_ptr(),
                                                  params.numel(), poff.data_ptr(), plen.data_ptr(), None, 0,
                                                  out.data_ptr(), out.numel(), None, None, ty.data_ptr(), state.data_ptr(),
                                                  None, None, None)
    assert code == 0
    torch.cuda.synchronize()
    assert host(ty, np.uint16) == want.types == host(sep.types, np.uint16)
    assert host(state, np.uint8) == want.status
    # (entry 4, DATA with a bad method, reads NONE with or without room; entry 5 is the one cut off)
    assert [i for i, e in enumerate(case.entries) if e[0] != want.types[i]] == [4, 5]
    assert rq.want_of(case, None).types[5] == rq.DATA
    assert torch.equal(out, out_a) and out.cpu().numpy().tobytes() == want.out


def test_no_connections_and_no_entries():
    """nconn == 0, and n == 0 with d_total (and a CSR): everything reads 0."""
    case = rq.small_cases(T)[0]
    ty, method, rid, poff, plen = entry_tensors(case)
    tb = dev_table(case.table)
    want = rq.want_of(case._replace(conn_first=[0]), None)
    r = rpc_amd.frames_request(method, rid, dev_bytes(case.params), poff, plen, tb, types=ty, conn_first=i64([0]))
    same_words(r, want, "nconn 0")
    assert host(r.conn_bytes_first, np.uint64) == [want.total]
    e64, e32 = torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV)
    e16 = torch.empty(0, dtype=torch.int16, device=DEV)
    e = rpc_amd.frames_request(e16, e32, dev_bytes(case.params), e64, e32, tb, conn_first=i64([0, 0, 0]))
    assert e.total == 0 and e.bodies.numel() == 0 and host(e.conn_bytes_first, np.uint64) == [0, 0, 0]
    out = torch.full((32,), rq.FILL, dtype=torch.uint8, device=DEV)
    e = rpc_amd.frames_request(e16, e32, dev_bytes(case.params), e64, e32, tb, out=out)
    assert int(e.total.cpu()[0]) == 0 and (out == rq.FILL).all()


def client_batch(n=304, nconn=8, seed=0x4e9):
    """About 300 entries on 8 connections: the seven methods with the params the client stubs
    build, every ninth call without params, a PING as every tenth entry, distinct 32-bit ids
    with the edges among them."""
    rng = random.Random(seed)
    ids = rng.sample(range(1, 1 << 32), n)
    ids[:3] = [0, 4294967295, 2147483648]
    types, method, params, poff, plen = [], [], bytearray(b"#"), [], []
    for i in range(n):
        ping = i % 10 == 9
        m = i % 7
        text = b"" if ping or i % 9 == 8 else json.dumps(rtc.canonical_params(rng, m), separators=(",", ":"),
                                                          ensure_ascii=False).encode()
        types.append(rq.PING if ping else rq.DATA)
        method.append(m)
        poff.append(len(params))
        plen.append(len(text))
        params += text + b"#"
    per = n // nconn
    return types, method, ids, bytes(params), poff, plen, [c * per for c in range(nconn)] + [n]


def scan_conns(stream, cbf, role):
    return rpc_amd.frames_scan(stream, i64(cbf[:-1]), i64([b - a for a, b in zip(cbf, cbf[1:])]), role=role, verify=True)


def test_inverse_and_closed_loop():
    """request -> pack -> server scan + verify -> unpack -> route with the same table: every
    frame reads OK (a PING reads CONTROL), and every call's method, id and params span give the
    inputs back.  Then on through reply -> pack -> client scan + verify -> unpack -> resolve with
    pending_ids = the request's ids: every slot is MATCHED, none stays open, nothing is deferred."""
    types, method, ids, params, poff, plen, conn = client_batch()
    n, nconn = len(ids), len(conn) - 1
    table = rpc_amd.route_table(rtc.METHODS)
    dparams = dev_bytes(params, 7)
    rqd = rpc_amd.frames_request(i16(method), i32(ids), dparams, i64(poff), i32(plen), table, types=i16(types),
                                 conn_first=i64(conn))
    st = host(rqd.status, np.uint8)
    calls = [i for i in range(n) if types[i] == rq.DATA]
    assert [i for i in range(n) if st[i] == rpc_amd.REQUEST_CALL] == calls
    assert all(st[i] == rpc_amd.REQUEST_NONE for i in range(n) if types[i] == rq.PING)
    assert host(rqd.types, np.uint16) == types
    p = rpc_amd.frames_pack(rqd.bodies, rqd.body_offsets, rqd.body_lens, types=rqd.types, conn_first=i64(conn))
    sc = scan_conns(p.stream, host(p.conn_bytes_first, np.uint64), "server")
    assert sc.nframes == n and host(sc.conn_first, np.uint64) == conn
    verdict = host(sc.verdict, np.uint8)[:n]
    assert verdict == [rpc_amd.FRAME_CONTROL if t == rq.PING else rpc_amd.FRAME_OK for t in types]
    u = rpc_amd.frames_unpack(p.stream, sc.frame_offsets[:n].contiguous(), sc.verdict[:n].contiguous(), role="server",
                              conn_first=sc.conn_first)
    rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, table, reply_types=u.reply_types, group=False)
    kind = host(rt.kind, np.uint8)
    assert kind == [rpc_amd.ROUTE_NONE if t == rq.PING else rpc_amd.ROUTE_CALL for t in types]
    got_m, got_id = host(rt.method, np.uint16), host(rt.id, np.uint32)
    body, at = u.bodies.cpu().numpy().tobytes(), host(u.body_offsets, np.uint64)
    po, pl = host(rt.params_off, np.uint32), host(rt.params_len, np.uint32)
    for i in calls:
        assert (got_m[i], got_id[i]) == (method[i], ids[i]), i
        assert body[at[i] + po[i]:at[i] + po[i] + pl[i]] == params[poff[i]:poff[i] + plen[i]], i
    assert sum(1 for i in calls if plen[i] == 0) > 20
    # the server's handlers answer {"v":<id>}; the replies go back over the wire
    values, voff, vlen = bytearray(), [], []
    for i in range(n):
        v = b'{"v":%d}' % ids[i] if types[i] == rq.DATA else b""
        voff.append(len(values))
        vlen.append(len(v))
        values += v
    rep = rpc_amd.frames_reply(rt.kind, rt.id, dev_bytes(values, 3), i64(voff), i32(vlen), reply_types=u.reply_types,
                               conn_first=sc.conn_first)
    p2 = rpc_amd.frames_pack(rep.bodies, rep.body_offsets, rep.body_lens, types=rep.types, conn_first=sc.conn_first)
    sc2 = scan_conns(p2.stream, host(p2.conn_bytes_first, np.uint64), "client")
    assert sc2.nframes == n  # (each PING came back as a PONG)
    u2 = rpc_amd.frames_unpack(p2.stream, sc2.frame_offsets[:n].contiguous(), sc2.verdict[:n].contiguous(), role="client")
    pending = [ids[i] for i in calls]  # the ids of the entries that read REQUEST_CALL
    rs = rpc_amd.frames_resolve(u2.bodies, u2.body_offsets, u2.body_lens, i32(pending), reply_types=u2.reply_types)
    torch.cuda.synchronize()
    rk = host(rs.kind, np.uint8)
    assert rk == [rpc_amd.RESOLVE_NONE if t == rq.PING else rpc_amd.RESOLVE_MATCHED for t in types]
    assert rpc_amd.RESOLVE_DEFER not in rk and int(rs.nopen.cpu()[0]) == 0
    assert host(rs.slot_entry, np.uint32) == calls
    body2, at2 = u2.bodies.cpu().numpy().tobytes(), host(u2.body_offsets, np.uint64)
    ro, rl = host(rs.result_off, np.uint32), host(rs.result_len, np.uint32)
    for i in calls:
        assert body2[at2[i] + ro[i]:at2[i] + ro[i] + rl[i]] == b'{"v":%d}' % ids[i], i
