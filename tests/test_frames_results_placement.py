"""Frame results on the GPU with the bodies anywhere (tests/stage_cases.py), and behind late
inputs on a side stream (the harness of tests/test_frames_streams.py).  The property each
placement was built for is asserted by stage_cases.rounds first; every answer is the plain
rules' (tests/results_cases.py), bit for bit."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import results_cases as rs  # noqa: E402
import stage_cases as sc  # noqa: E402
import test_frames_results as fx  # noqa: E402
from test_frames_route import dev_bytes  # noqa: E402
from test_frames_streams import Job, behind_blocker, on, run_late, side_streams  # noqa: E402,F401


def run(buf, spans, mis, what, holds=None):
    """``holds`` asserted for the entries that reach the rounds, then one call over entries on
    ``spans`` (results_cases.placed_entries: every body inside the buffer is walked), compared
    with the plain rules."""
    if holds:
        holds(sc.walked(buf, spans), mis)
    entries, pm, se = rs.placed_entries(buf, spans)
    return fx.check(buf, entries, pm, se, mis=mis, what=what)


@pytest.mark.parametrize("mis", [0, 5, 15])
@pytest.mark.parametrize("name", sc.BATCH)
def test_batch_placements_match_plain_rules(name, mis):
    """700 reply bodies over three workgroups in reversed and shuffled memory order and in slots
    of 1,040 and 4,099 bytes; 256 lanes on one body; lanes alternating between two bodies more
    than a window apart; every prefix and suffix of one text."""
    p = sc.batch(name, sc.resolve_set()[0], sc.reply)
    want = run(p.buf, p.spans, mis, (name, mis), p.holds)
    assert {rs.OK, rs.DEFER} <= {w.status for w in want}


@pytest.mark.parametrize("name", ["reversed", "shuffled", "slots of 1040", "slots of 4099"])
def test_rows_do_not_depend_on_the_placement(name):
    """Entry i is body i in every placement and every offset in the answers is relative to the
    body, so a placed batch answers as the same bodies back to back, entry for entry."""
    bodies = sc.resolve_set()[0]
    base = sc.batch("back to back", bodies, sc.reply)
    p = sc.batch(name, bodies, sc.reply)
    assert [s[1] for s in p.spans] == [s[1] for s in base.spans]
    assert run(p.buf, p.spans, 5, name) == run(base.buf, base.spans, 5, "back to back")


@pytest.mark.parametrize("mis", [0, 1, 15])
def test_window_edges(mis):
    """Lane 0's body opens the window; lanes 1 and 2 hold a body that ends on the window's last
    byte (one round takes all three) and one byte behind it (it waits for round two)."""
    edges = sc.window_edges(sc.reply, mis)
    assert len(edges) == 12
    for p in edges:
        want = run(p.buf, p.spans, mis, (p.name, mis), p.holds)
        assert all(w.status in (rs.OK, rs.MISMATCH, rs.DEFER) for w in want)  # (each was walked)


def test_buffer_ends():
    """A body at offset 0 and a body that ends on the buffer's last byte, at every address mod
    16, and a whole buffer of 8 bytes."""
    for mis in range(16):
        p = sc.buffer_ends(sc.reply, mis)
        run(p.buf, p.spans, mis, p.name, p.holds)
    for mis in sc.WHOLE_MIS:
        p = sc.whole_buffer(sc.WHOLE, mis)
        want = run(p.buf, p.spans, mis, p.name, p.holds)
        assert [w.status for w in want] == [rs.MISMATCH]  # ({"id":7} as a whole `result` for an I32)


def test_every_placement_in_one_call():
    mis = 5
    buf, spans, _ = sc.mixture(sc.resolve_set()[0], sc.reply, mis)
    run(buf, spans, mis, "mixture")
    counts = [len(g) for g in sc.rounds(spans, sc.walked(buf, spans), mis)]
    assert counts[0] >= 128 and counts[1] == 1 and len(counts) >= 4


def results_job(mis):
    """frames_results on its own case table with 600 more replies behind it, every input late."""
    buf, entries, pm, se = rs.case_entries(pad_front=3)
    more, ents, pm2, _ = rs.back_to_back(rs.canonical_set(0x57, 300) + rs.mutation_set(0x58, 300))
    s0, e0 = len(pm), len(entries)
    entries = entries + [(e[0] + len(buf), e[1], e[2], e[3] + s0) + tuple(e[4:]) for e in ents]
    pm, se, buf = pm + pm2, se + [e0 + k for k in range(len(ents))], buf + more
    want = rs.results_entries(buf, entries, pm)
    off, ln, resolve, d_pm, d_ty = fx.dev_call(entries, pm, se)
    d_buf = dev_bytes(buf, mis)

    def call(stream):
        return rpc_amd.frames_results(d_buf, off, ln, resolve, d_pm, d_ty, stream=stream)

    def check(r):
        rows, slots, nd = fx.rows_of(r)
        assert rows == want, ("results", mis)
        assert slots == rs.results_slots(entries, want, se) and nd == rs.ndefer(want)
        assert {w.status for w in want} == set(range(7))

    late = [d_buf, off, ln, resolve.kind, resolve.slot, resolve.result_off, resolve.result_len, resolve.error_off,
            resolve.error_len, resolve.slot_entry, d_pm, d_ty]
    return Job("results table", late, call, check)


def test_client_round_with_results_one_stream_one_synchronisation():
    """test_frames_streams' client round extended by the results: request -> pack -> (the packed
    bytes as the peer's stream) scan + verify -> unpack -> resolve -> results on one side stream
    behind late inputs, each stage fed the previous stage's device tensors, one synchronisation.
    The pending ids are the request's id column and the pending methods its method column; what
    comes back are the requests themselves, so every MATCHED entry has neither member: the slot
    of each call reads ABSENT twice with its body's offset, the slot of each PONG stays open."""
    import numpy as np
    import resolve_cases as rv
    import route_cases as rc
    import values_cases as vc
    from test_frames_streams import DEV, client_round, guarded, host, same_bytes, u16, u32, u64
    w = client_round()
    n = len(w.ids)
    s = side_streams()[0]
    d_ty, d_m, d_id = u16(w.types), u16(w.method), u32(w.ids)
    d_params, d_poff, d_plen, d_conn = dev_bytes(w.params, 7), u64(w.poff), u32(w.plen), u64(w.conn)
    table = rpc_amd.route_table(rc.METHODS, device=DEV)
    rtypes = rpc_amd.result_types(rc.METHODS, vc.IDL_RESULTS, device=DEV)
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
        r = rpc_amd.frames_resolve(u.bodies, u.body_offsets, u.body_lens, d_id, reply_types=u.reply_types, stream=s)
        x = rpc_amd.frames_results(u.bodies, u.body_offsets, u.body_lens, r, d_m, rtypes, stream=s)
        return r, x, (q, p, f, u, at, ln)

    with on(s):  # (the glue's two kernels, loaded before the blocker starts)
        (d_conn[1:] - d_conn[:-1]).contiguous()
    s.synchronize()
    r, x, _ = behind_blocker(s, [d_ty, d_m, d_id, d_params, d_poff, d_plen, d_conn], round_, "client round with results")
    same_bytes(u_big, 5, w.unpack.out, "unpacked bodies")
    assert host(r.kind, np.uint8) == w.resolve.kind and host(r.slot, np.uint32) == w.resolve.slot
    assert host(r.slot_entry, np.uint32) == w.resolve.slot_entry
    entries = list(zip(w.unpack.body_offsets, w.unpack.body_lens, w.resolve.kind, w.resolve.slot, w.resolve.result_off,
                       w.resolve.result_len, w.resolve.error_off, w.resolve.error_len))
    want = rs.results_entries(w.unpack.out, entries, w.method, vc.IDL_RESULTS)
    rows, slots, nd = fx.rows_of(x)
    assert rows == want and slots == rs.results_slots(entries, want, w.resolve.slot_entry) and nd == 0
    calls = [i for i in range(n) if w.resolve.kind[i] == rv.MATCHED]
    assert len(calls) == n - n // 10 and all(want[i] == rs.Row(rs.ABSENT, 0, rs.ABSENT, 0, 0) for i in calls)
    assert [sl[0] for sl in slots] == [rs.ABSENT if i in set(calls) else 0 for i in range(n)]
    assert [slots[i][4] for i in calls] == [w.unpack.body_offsets[i] for i in calls]


@pytest.mark.parametrize("mis", [0, 7])
def test_results_behind_late_inputs(mis):
    """The call on a side stream behind a blocker and behind the copies that bring its inputs:
    every launch and the memset of the count are on that stream."""
    run_late(results_job(mis))
