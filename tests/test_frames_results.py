"""Frame results on the GPU (rpc_frames_results_device): the typed `result` and
the `error` of every matched reply, per entry and per pending slot.  Against the plain Python
rules of tests/results_cases.py on every output, bit for bit, DEFER included; resolve ->
results on the resolve's own join cases; and the round trip from columns, values -> reply ->
resolve -> results, all on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import resolve_cases as rv  # noqa: E402
import results_cases as rs  # noqa: E402
from test_frames_route import DEV, FILL, GUARD, dev_bytes, filled, to_dev  # noqa: E402


def dev_call(entries, pm, se, types=rs.TYPES):
    """(body_offsets, body_lens, FrameResolve, pending_method, result_types) of results_cases entries."""
    col = lambda j, wide, narrow: to_dev(np.array([e[j] for e in entries], dtype=wide).view(narrow))  # noqa: E731
    u32 = lambda j: col(j, np.uint32, np.int32)  # noqa: E731
    resolve = rpc_amd.FrameResolve(col(2, np.uint8, np.uint8), None, u32(4), u32(5), u32(6), u32(7), u32(3),
                                   to_dev(np.array(se, dtype=np.uint32).view(np.int32)), None, None)
    return (col(0, np.uint64, np.int64), col(1, np.uint32, np.int32), resolve,
            to_dev(np.array(pm, dtype=np.uint16).view(np.int16)), to_dev(np.array(types, dtype=np.uint8)))


def rows_of(r):
    h = lambda x, d: x.cpu().numpy().view(d).tolist()  # noqa: E731
    rows = [rs.Row(*x) for x in zip(h(r.status, np.uint8), h(r.value, np.uint64), h(r.error_status, np.uint8),
                                    h(r.error_code, np.int32), h(r.error_message, np.uint64))]
    slots = list(zip(h(r.slot_status, np.uint8), h(r.slot_value, np.uint64), h(r.slot_error_status, np.uint8),
                     h(r.slot_error_code, np.int32), h(r.slot_str_base, np.uint64)))
    return rows, slots, int(r.ndefer.cpu()[0])


def check(buf, entries, pm, se, types=rs.TYPES, mis=0, what="", stream=None):
    off, ln, resolve, d_pm, d_ty = dev_call(entries, pm, se, types)
    r = rpc_amd.frames_results(dev_bytes(buf, mis), off, ln, resolve, d_pm, d_ty, stream=stream)
    torch.cuda.synchronize()
    rows, slots, nd = rows_of(r)
    want = rs.results_entries(buf, entries, pm, types)
    assert len(rows) == len(want)
    for k, (g, w) in enumerate(zip(rows, want)):
        assert g == w, (what, k, entries[k], g, w)
    assert slots == rs.results_slots(entries, want, se), what
    assert nd == rs.ndefer(want), what
    return want


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_table_matches_plain_rules(mis):
    """The case table as one buffer (every status for every type, every kind that is not
    MATCHED, each broken schema word, RANGE for each of the three spans; the last body ends on
    the buffer's last byte; at an odd address the buffer's first block is partial too), and the
    per-slot cases."""
    buf, entries, pm, se = rs.case_entries(pad_front=3)
    want = check(buf, entries, pm, se, mis=mis, what="table")
    assert {w.status for w in want} == set(range(7))
    assert any(e[2] == rv.MATCHED and e[0] + e[1] == len(buf) and w.status == rs.OK for e, w in zip(entries, want))
    check(*rs.slot_cases(), mis=mis, what="slots")


def test_mutations_match_plain_rules():
    """The emulator's mutation set on the device: 20,000 canonical members with one byte flipped,
    inserted or deleted, or truncated, behind the canonical replies themselves (all five types
    inside every wave)."""
    canon = rs.canonical_set(0xE5017, 1500)
    muts = rs.mutation_set(0xBADE501, 20000)
    buf, entries, pm, se = rs.back_to_back(canon + muts)
    want = check(buf, entries, pm, se, mis=3, what="mutations")
    assert {w.status for w in want} == {rs.OK, rs.ABSENT, rs.MISMATCH, rs.DEFER}
    assert {w.error_status for w in want} == {rs.OK, rs.ABSENT, rs.MISMATCH, rs.DEFER}


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_around_one_workgroup(n):
    """A workgroup is 256 entries.  n == 0 still writes the per-slot outputs and the count."""
    replies = (rs.canonical_set(0x51, 200) + rs.mutation_set(0x52, 57))[:n]
    buf, entries, pm, se = rs.back_to_back(replies, nul=0)
    check(buf, entries, pm + [rs.I32] * 3, se + [rv.NO_SLOT, 0, n], mis=1, what=f"n = {n}")


def test_long_bodies_need_several_rounds():
    """300 bodies of 1,000 to 1,024 bytes, back to back from an odd offset: a workgroup's bodies
    fill several staging rounds and bodies straddle the rounds' ends; both members are walked in
    one staged body, the `error` in front of the `result` in every third."""
    def long_reply(k):  # reply k, padded to 1024 - k % 25 bytes
        if k % 5 == 4:
            make = lambda pad: (rs.I32, b"%d" % -k, rs.err(b"%d" % k, b'"' + b"e" * pad + b'"'))  # noqa: E731
        else:
            make = lambda pad: (rs.STR, b'"' + b"s" * pad + b'"', rs.err(b"-32000", b'"m"'))  # noqa: E731
        return make(1024 - k % 25 - len(rs.reply(k, *make(0)[1:])[0]))

    buf, entries, pm, se = rs.back_to_back([long_reply(k) for k in range(300)], pad_front=7)
    assert {e[1] for e in entries} == set(range(1000, 1025))
    assert len({e[0] // 32768 for e in entries}) >= 8  # (the bodies of a workgroup lie in several windows)
    want = check(buf, entries, pm, se, mis=9, what="long bodies")
    assert all(w.status == rs.OK and w.error_status == rs.OK for w in want)


def test_only_what_is_specified_is_written():
    """Every output pre-filled, with guard elements on both sides: each is written whole and
    nothing else is, and every output is optional (each left NULL in turn)."""
    buf, entries, pm, se = rs.back_to_back(rs.canonical_set(0x61, 300) + rs.mutation_set(0x62, 300))
    pm, se = pm + [rs.F64] * 5, se + [rv.NO_SLOT, 3, 10000, 599, 600]
    n, npend = len(entries), len(pm)
    want = rs.results_entries(buf, entries, pm)
    wslots = rs.results_slots(entries, want, se)
    off, ln, rv_, d_pm, d_ty = dev_call(entries, pm, se)
    d_buf = dev_bytes(buf)
    specs = [("status", np.uint8, torch.uint8, n), ("value", np.uint64, torch.int64, n),
             ("error_status", np.uint8, torch.uint8, n), ("error_code", np.uint32, torch.int32, n),
             ("error_message", np.uint64, torch.int64, n), ("slot_status", np.uint8, torch.uint8, npend),
             ("slot_value", np.uint64, torch.int64, npend), ("slot_error_status", np.uint8, torch.uint8, npend),
             ("slot_error_code", np.uint32, torch.int32, npend), ("slot_str_base", np.uint64, torch.int64, npend),
             ("ndefer", np.uint32, torch.int32, 1)]
    fill = {1: FILL, 4: FILL * 0x01010101, 8: FILL * 0x0101010101010101}
    expect = {"status": [w.status for w in want], "value": [w.value for w in want],
              "error_status": [w.error_status for w in want], "error_code": [w.error_code & 0xFFFFFFFF for w in want],
              "error_message": [w.error_message for w in want], "slot_status": [s[0] for s in wslots],
              "slot_value": [s[1] for s in wslots], "slot_error_status": [s[2] for s in wslots],
              "slot_error_code": [s[3] & 0xFFFFFFFF for s in wslots], "slot_str_base": [s[4] for s in wslots],
              "ndefer": [rs.ndefer(want)]}

    def call(given):
        outs = {k: filled(cnt, npd, td) for k, npd, td, cnt in specs}
        ptrs = [outs[k][GUARD:].data_ptr() if k in given else None for k, *_ in specs]
        rcode = _lib.rpc_frames_results_device(d_buf.data_ptr(), d_buf.numel(), off.data_ptr(), ln.data_ptr(),
                                               rv_.kind.data_ptr(), rv_.slot.data_ptr(), rv_.result_off.data_ptr(),
                                               rv_.result_len.data_ptr(), rv_.error_off.data_ptr(),
                                               rv_.error_len.data_ptr(), rv_.slot_entry.data_ptr(), n, d_pm.data_ptr(),
                                               npend, d_ty.data_ptr(), d_ty.numel(), *ptrs, None)
        assert rcode == 0
        torch.cuda.synchronize()
        for k, npd, td, cnt in specs:
            a = outs[k].cpu().numpy().view(npd)
            f = fill[np.dtype(npd).itemsize]
            assert (a[:GUARD] == f).all() and (a[GUARD + cnt:] == f).all(), k
            if k not in given:
                assert (a == f).all(), k
            else:
                assert a[GUARD:GUARD + cnt].tolist() == expect[k], (k, given)

    names = [k for k, *_ in specs]
    call(names)
    for leave in names:
        call([k for k in names if k != leave])
    call([])


def test_two_matched_entries_on_one_slot_twice():
    """What no resolve produces: two MATCHED entries naming one slot, in two workgroups.  The
    slot is the entry's that slot_entry names, both times."""
    replies = [(rs.I32, b"%d" % k, None) for k in range(600)]
    buf, entries, pm, se = rs.back_to_back(replies)
    entries[590] = entries[590][:3] + (7,) + entries[590][4:]    # slot 7 is named by entries 7 and 590
    entries[300] = entries[300][:3] + (200,) + entries[300][4:]  # and slot 200 by 200 and 300
    se[7], se[200] = 590, 200
    first = check(buf, entries, pm, se, what="first")
    slots = rs.results_slots(entries, first, se)
    assert slots[7][1] == 590 and slots[200][1] == 200 and slots[590][0] == 0 and slots[300][0] == 0
    assert check(buf, entries, pm, se, what="second") == first


def test_resolve_then_results():
    """frames_resolve's own device outputs go into frames_results unchanged, on the resolve's
    join cases: colliding ids, an id in two slots, duplicates across workgroups."""
    for name, call in rv.join_calls().items():
        d_buf = dev_bytes(call.buf)
        off = to_dev(np.array(call.offs, dtype=np.uint64).view(np.int64))
        ln = to_dev(np.array(call.lens, dtype=np.uint32).view(np.int32))
        pend = to_dev(np.array(call.pending, dtype=np.uint32).view(np.int32))
        pm = [s % 5 for s in range(len(call.pending))]
        d_pm = to_dev(np.array(pm, dtype=np.uint16).view(np.int16))
        d_ty = rpc_amd.result_types(["m%d" % k for k in range(5)], list(range(5)), device=DEV)
        rr = rpc_amd.frames_resolve(d_buf, off, ln, pend)
        r = rpc_amd.frames_results(d_buf, off, ln, rr, d_pm, d_ty)
        torch.cuda.synchronize()
        w = call.expect()
        entries = list(zip(call.offs, call.lens, w.kind, w.slot, w.result_off, w.result_len, w.error_off, w.error_len))
        want = rs.results_entries(call.buf, entries, pm, list(range(5)))
        rows, slots, nd = rows_of(r)
        assert rows == want, name
        assert slots == rs.results_slots(entries, want, w.slot_entry), name
        assert nd == rs.ndefer(want), name
        assert [s[0] != 0 for s in slots] == [e != rv.NO_SLOT for e in w.slot_entry], name


def test_round_trip_from_columns():
    """values (RESULT form) -> reply -> resolve -> results, all on the device, on
    tests/values_numbers.py's lists (2,000 of each) and the other four types: an I32, I64, BOOL
    or STR slot comes back unchanged, an F64 slot is the bits of Python's float() of the values'
    text, and DEFER appears only on doubles above 1.797693134862315e308 (the subnormals the
    values deferred come back as the error they were answered with)."""
    import random
    import struct
    import values_cases as vc
    import values_numbers as vn
    rng = random.Random(0x21)
    rows = [(rs.F64, b) for _, bs in vn.corpus().items() for b in rng.sample(bs, min(2000, len(bs)))]
    rows += [(rs.I32, rng.choice([rng.randrange(-2**31, 2**31), -2**31, 2**31 - 1, 0]) & rs.M64) for _ in range(2000)]
    rows += [(rs.I64, rng.choice([rng.randrange(-2**63, 2**63), -2**63, 2**63 - 1, 0]) & rs.M64) for _ in range(2000)]
    rows += [(rs.BOOL, k & 1) for k in range(2000)]
    strings, texts = bytearray(), []
    for k in range(2000):
        s = "".join(rng.choice("abcxyz0189 _-/é中{}[]:,") for _ in range(rng.randrange(0, 40))).encode()
        rows.append((rs.STR, len(strings) | len(s) << 32))
        strings += s + b"|"
        texts.append(s)
    rng.shuffle(rows)
    n = len(rows)
    rtypes = rpc_amd.result_types(["m%d" % k for k in range(5)], [rs.I32, rs.I64, rs.F64, rs.BOOL, rs.STR], device=DEV)
    method = to_dev(np.array([t for t, _ in rows], dtype=np.int16))
    slots = to_dev(np.array([v for _, v in rows], dtype=np.uint64).view(np.int64).reshape(1, n))
    ids = np.random.default_rng(5).permutation(n).astype(np.uint32) * 7 + 1
    v = rpc_amd.frames_values(method, slots, rtypes, strings=to_dev(np.frombuffer(bytes(strings), dtype=np.uint8).copy()))
    rp = rpc_amd.frames_reply(None, to_dev(ids.view(np.int32)), v.values, v.value_offsets, v.value_lens,
                              status=v.reply_status)
    order = np.random.default_rng(6).permutation(n)  # slot s waits for entry order[s]
    rr = rpc_amd.frames_resolve(rp.bodies, rp.body_offsets, rp.body_lens, to_dev(ids[order].view(np.int32)))
    pm = to_dev(np.array([rows[e][0] for e in order], dtype=np.int16))
    x = rpc_amd.frames_results(rp.bodies, rp.body_offsets, rp.body_lens, rr, pm, rtypes)
    torch.cuda.synchronize()
    got, slots_got, nd = rows_of(x)
    vst = v.status.cpu().numpy().tolist()
    bodies = rp.bodies.cpu().numpy().tobytes()
    boff = rp.body_offsets.cpu().numpy().tolist()
    assert rr.kind.cpu().numpy().tolist() == [rv.MATCHED] * n
    defers = 0
    for i, ((t, slot), g) in enumerate(zip(rows, got)):
        if vst[i] == vc.DEFER:  # a subnormal: the values deferred, the reply is -32603
            assert t == rs.F64 and (g.status, g.value, g.error_status, g.error_code) == (rs.ABSENT, 0, rs.OK, -32603), i
            continue
        assert vst[i] == vc.OK and g.error_status == rs.ABSENT, i
        if t == rs.F64:
            text = vc.f64_text(slot)
            if text == b"null":  # NaN, the infinities
                assert (g.status, g.value) == (rs.MISMATCH, 0), (i, hex(slot))
            elif g.status == rs.DEFER:
                defers += 1
                assert g.value == 0 and abs(struct.unpack("<d", struct.pack("<Q", slot))[0]) > 1.797693134862315e308, hex(slot)
            else:
                assert (g.status, g.value) == (rs.OK, rs.f64(text)), (i, hex(slot), text)
        elif t == rs.STR:
            at, ln = g.value & 0xFFFFFFFF, g.value >> 32
            assert g.status == rs.OK and bodies[boff[i] + at:boff[i] + at + ln] == strings[slot & 0xFFFFFFFF:][:slot >> 32], i
        else:
            assert (g.status, g.value) == (rs.OK, slot), (i, t, slot)
    assert nd == defers and defers > 0  # (the sample holds all of above_max15: the DEFER branch is reached)
    assert sum(1 for i, (t, _) in enumerate(rows) if vst[i] == vc.DEFER) >= 10  # (and the subnormals' path)
    for s, e in enumerate(order.tolist()):  # the completions, by slot
        assert slots_got[s] == (got[e].status, got[e].value, got[e].error_status, got[e].error_code, boff[e]), s
    print("round trip: %d rows, %d DEFER" % (n, defers))


def test_a_stream_of_its_own():
    buf, entries, pm, se = rs.back_to_back(rs.canonical_set(0x57, 700))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check(buf, entries, pm, se, what="stream", stream=s)
