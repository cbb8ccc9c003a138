"""The frame route and the frame reply against the reference's own dispatcher on generated
bodies (tests/route_fuzz.py; oracle/_ref/ref_dispatch is rpc_server_dispatch behind a driver of
ours).  For every body B with the reference's reply R:

    a. R is the parse error                 -> the row reads DEFER
    b. a NOT_FOUND or INVALID row           -> reply_cases.error_body(id, code, message) == R
    c. a CALL row (method, id, span)        -> B' = the canonical request with the table's name,
                                               the span's bytes as `params` (none when the span
                                               is empty) and the id; ref(B') == R, no parse error
    d. the whole chain                      -> the handler's value cut from ref(B') (or its error
                                               code as the status; for a DEFER row R itself, RAW)
                                               through the reply gives R, for every entry

c is what holds the `params` span against the member cJSON picks: a span that is off by a byte,
belongs to a later duplicate or to a key that only looks like `params` gives another answer.
Run on the plain rules (two seeds of 34,000 bodies), on the CPU emulators (12,000), on the GPU
(34,000, with the rows also held against the rules field for field), and once over the wire:
scan + verify -> unpack -> route -> reply -> pack on 64 connections."""
import numpy as np
import pytest

import reply_cases as rp
import route_cases as rc
import route_fuzz as rf
import scan_cases as sc
from test_reply_emu import T_K, reply_emu, run_emu as run_reply_emu  # noqa: F401  (reply_emu: a fixture)
from test_route_emu import S_K, S_SMALL, route_emu, run_emu as run_route_emu  # noqa: F401  (route_emu: a fixture)

SEEDS = [0xF0221, 0xF0222]
N_EMU = 12000


def test_driver_hands_over_c_strings():
    """The driver's framing: no body, an empty one, one that ends at a 0 byte for the dispatcher,
    one longer than any frame, and the order of the replies."""
    assert rf.reference([]) == []
    ping = b'{"method":"ping","id":%d}'
    bodies = [b"", ping % 1, ping % 2 + b"\0" + ping % 3, b" " * 5000 + ping % 4, b'{"method":"ping","id":5', ping % 6]
    pong = b'{"jsonrpc":"2.0","id":%d,"result":"pong"}'
    assert rf.reference(bodies) == [rf.PARSE_ERROR, pong % 1, pong % 2, pong % 4, rf.PARSE_ERROR, pong % 6]


@pytest.mark.parametrize("seed", SEEDS)
def test_corpus_reaches_both_sides(seed):
    """route_fuzz.conditions: the thresholds that keep the comparison from being empty, on the
    plain rules and the reference alone."""
    n = rf.conditions(rf.corpus(seed), rf.answers(seed), rf.ruled(seed))
    print(n)


@pytest.mark.parametrize("seed", SEEDS)
def test_rules_hold_against_the_reference(seed):
    """a to c on route_cases.route_body, d on reply_cases.want_of: the yardstick of the other
    layers against the live dispatcher, on every body of the corpus."""
    bodies, replies, rows = rf.corpus(seed).bodies, rf.answers(seed), rf.ruled(seed)
    handled = rf.hold_route(bodies, replies, rows)
    want = rp.want_of(rf.reply_case(rows, handled), None)
    rf.hold_replies(bodies, replies, want.body_offsets, want.body_lens, want.out)
    assert set(want.status) == {rp.R_RESULT, rp.R_ERROR, rp.R_RAW}


def same_rows(bodies, got, want, order, first, what):
    """A layer's rows and groups against the plain rules', field for field."""
    assert len(got) == len(want)
    for body, g, w in zip(bodies, got, want):
        assert g == w, (what, body, g, w)
    assert (order, first) == rc.groups_of(want, len(rc.METHODS)), what


@pytest.mark.parametrize("stage,mis,nul,tile,src_mis,out_mis", [(S_K, 0, 1, T_K, 0, 0), (S_SMALL, 11, 0, 256, 7, 9)])
def test_emulators_hold_against_the_reference(route_emu, reply_emu, stage, mis, nul, tile, src_mis, out_mis):  # noqa: F811
    """The route emulator at the kernel's staging size and at the small one (at an odd address,
    the bodies with nothing between them), then the reply emulator at the kernel's tile and at
    256 on that route's rows."""
    seed = SEEDS[0]
    bodies, replies = rf.corpus(seed).bodies[:N_EMU], rf.answers(seed)[:N_EMU]
    buf, entries = rc.back_to_back(bodies, nul=nul)
    rows, order, first = run_route_emu(route_emu, stage, mis, buf, entries, None, rc.IDL)
    same_rows(bodies, rows, rf.ruled(seed)[:N_EMU], order, first, (stage, mis))
    handled = rf.hold_route(bodies, replies, rows)
    assert sum(1 for r in rows if r[0] == rc.CALL and r[4]) >= 2000
    case = rf.reply_case(rows, handled)
    total, out_rows, conn, out = run_reply_emu(reply_emu, tile, src_mis, out_mis, case, None)
    rf.hold_replies(bodies, replies, [r[0] for r in out_rows], [r[1] for r in out_rows], out)
    assert conn == [0, total] == [0, sum(map(len, replies))]


# ---- the GPU ----------------------------------------------------------------------------------
def gpu_reply(rt, rows, handled, mis):
    """rpc_amd.frames_reply on the route's own device outputs: (offsets, lengths, bytes)."""
    import rpc_amd
    from test_frames_reply import entry_tensors
    from test_frames_unpack import dev_bytes, host
    case = rf.reply_case(rows, handled)
    _, _, _, st, voff, vlen = entry_tensors(case)
    r = rpc_amd.frames_reply(rt.kind, rt.id, dev_bytes(case.values, mis), voff, vlen, status=st)
    return host(r.body_offsets, np.uint64), host(r.body_lens, np.uint32), r.bodies.cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("nul,mis", [(1, 0), (1, 5), (0, 0), (0, 5)])
def test_gpu_holds_against_the_reference(nul, mis):
    """rpc_amd.frames_route on the whole corpus, with and without the 0 byte between the bodies,
    the buffer at a 16-byte boundary and 5 bytes past one: the rows and the groups are the plain
    rules', a to c hold, and rpc_amd.frames_reply on the route's own device outputs builds the
    reference's reply for every entry."""
    import torch
    import rpc_amd
    from test_frames_route import dev_bytes, dev_entries, dev_table, rows_of
    seed = SEEDS[0]
    bodies, replies = rf.corpus(seed).bodies, rf.answers(seed)
    buf, entries = rc.back_to_back(bodies, nul=nul)
    off, ln, _ = dev_entries(entries, None)
    d_buf = dev_bytes(buf, mis)
    assert d_buf.data_ptr() % 16 == mis
    rt = rpc_amd.frames_route(d_buf, off, ln, dev_table(rc.IDL))
    torch.cuda.synchronize()
    rows = rows_of(rt, len(entries))
    first = rt.group_first.cpu().numpy().view(np.uint32).tolist()
    order = rt.order.cpu().numpy().view(np.uint32)[:first[-1]].tolist()
    same_rows(bodies, rows, rf.ruled(seed), order, first, (nul, mis))
    handled = rf.hold_route(bodies, replies, rows)
    offs, lens, out = gpu_reply(rt, rows, handled, 5 - mis)
    rf.hold_replies(bodies, replies, offs, lens, out)
    assert len(out) == sum(map(len, replies))


@pytest.mark.gpu
def test_one_wire_round_answers_as_the_reference():
    """The corpus dealt over 64 connections as wire frames, PINGs in between, through scan +
    verify -> unpack (nul) -> route -> reply -> pack, the handlers' values taken from the
    reference as in d: every connection's bytes to send are exactly frame(R) for each of its
    bodies and a PONG for each PING.  (A body of 1025 bytes would close its connection at the
    scan: those stay out.)"""
    import torch
    import rpc_amd
    from test_frames_route import dev_bytes, dev_table, rows_of, to_dev
    from test_frames_unpack import host, i64
    seed, nconn = SEEDS[0], 64
    pairs = [(b, r) for b, r in zip(rf.corpus(seed).bodies, rf.answers(seed)) if len(b) <= rc.MAX_BODY]
    conns, want, dealt = [], [], []
    for c in range(nconn):
        parts, sends = [], []
        for k, (body, reply) in enumerate(pairs[c::nconn]):
            if (k + c) % 7 == 3:
                parts.append(sc.frame(typ=rc.PING))
                sends.append(sc.frame(typ=rc.PONG))
                dealt.append(None)
            parts.append(sc.frame(body))
            sends.append(sc.frame(reply))
            dealt.append((body, reply))
        conns.append(b"".join(parts))
        want.append(b"".join(sends))
    lens = [len(c) for c in conns]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev_bytes(b"".join(conns), 3)
    s = rpc_amd.frames_scan(raw, to_dev(offs), to_dev(np.array(lens, dtype=np.int64)), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, s.frame_offsets, s.verdict, role="server", nul=True, conn_first=s.conn_first)
    rt = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, dev_table(rc.IDL), reply_types=u.reply_types)
    torch.cuda.synchronize()
    assert s.nframes == len(dealt) and sum(1 for d in dealt if d is None) >= 1000
    rows = rows_of(rt, s.nframes)
    data = [i for i, d in enumerate(dealt) if d is not None]
    assert all(rows[i] == (rc.NONE, rc.NO_METHOD, 0, 0, 0) for i, d in enumerate(dealt) if d is None)
    handled = rf.hold_route([dealt[i][0] for i in data], [dealt[i][1] for i in data], [rows[i] for i in data])
    n = rt.id.numel()  # (the scan sized its arrays exactly)
    assert n == s.nframes
    values, voff, vlen, status = bytearray(b"~"), [0] * n, [0] * n, [0] * n
    for i, (st, value) in zip(data, handled):
        voff[i], vlen[i], status[i] = len(values), len(value), st
        values += value
    r = rpc_amd.frames_reply(rt.kind, rt.id, dev_bytes(values, 9), i64(voff), to_dev(np.asarray(vlen, dtype=np.int32)),
                             status=to_dev(np.asarray(status, dtype=np.int32)), reply_types=u.reply_types,
                             conn_first=s.conn_first)
    p = rpc_amd.frames_pack(r.bodies, r.body_offsets, r.body_lens, types=r.types, versions=u.versions,
                            conn_first=s.conn_first)
    cbf = host(p.conn_bytes_first, np.uint64)
    wire = p.stream.cpu().numpy().tobytes()
    assert len(cbf) == nconn + 1 and cbf[-1] == len(wire) == sum(map(len, want))
    for c in range(nconn):
        assert wire[cbf[c]:cbf[c + 1]] == want[c], c
