"""Frame route on the GPU (rpc_frames_route_device): the JSON-RPC envelope of
every delivered body, the method index and the groups.  Against the plain Python rules of
tests/route_cases.py field for field, DEFER included; and scan + verify -> unpack -> route on
wire bytes built here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import route_cases as rc  # noqa: E402
import scan_cases as sc  # noqa: E402

DEV = "cuda:0"
GUARD = 8  # elements on both sides of every output
FILL = 0xA5


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bytes(blob, mis=0):
    """blob on the device, its first byte mis bytes past a 16-byte boundary, and no byte of the
    allocation behind its last one."""
    a = np.zeros(mis + len(blob), dtype=np.uint8)
    a[mis:] = np.frombuffer(bytes(blob), dtype=np.uint8)
    return to_dev(a)[mis:]


def dev_table(table):
    names = to_dev(np.frombuffer(table.names, dtype=np.uint8).copy())
    offs = to_dev(np.array(table.offs, dtype=np.uint32).view(np.int32))
    return rpc_amd.RouteTable(names, offs, table.nmethods)


def dev_entries(entries, types):
    off = to_dev(np.array([e[0] for e in entries], dtype=np.uint64).view(np.int64))
    ln = to_dev(np.array([e[1] for e in entries], dtype=np.uint32).view(np.int32))
    ty = None if types is None else to_dev(np.array(types, dtype=np.uint16).view(np.int16))
    return off, ln, ty


def rows_of(r, n):
    cols = [r.kind.cpu().numpy().view(np.uint8), r.method.cpu().numpy().view(np.uint16),
            r.id.cpu().numpy().view(np.uint32), r.params_off.cpu().numpy().view(np.uint32),
            r.params_len.cpu().numpy().view(np.uint32)]
    return [tuple(int(c[i]) for c in cols) for i in range(n)]


def gpu_route(buf, entries, types, table, mis=0):
    """(rows, order, group_first) of rpc_amd.frames_route."""
    off, ln, ty = dev_entries(entries, types)
    r = rpc_amd.frames_route(dev_bytes(buf, mis), off, ln, dev_table(table), reply_types=ty)
    torch.cuda.synchronize()
    first = r.group_first.cpu().numpy().view(np.uint32).tolist()
    order = r.order.cpu().numpy().view(np.uint32)[:first[-1]].tolist()
    return rows_of(r, len(entries)), order, first


def check(buf, entries, types, table, mis, what):
    rows, order, first = gpu_route(buf, entries, types, table, mis)
    want = rc.route_entries(buf, entries, table, types)
    for i, (g, w) in enumerate(zip(rows, want)):
        assert g == w, (what, i, entries[i], buf[entries[i][0]:entries[i][0] + entries[i][1]][:80], g, w)
    worder, wfirst = rc.groups_of(want, table.nmethods)
    assert first == wfirst and order == worder, what
    return want


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_table_matches_plain_rules(mis):
    """The case table as one buffer (every kind; the buffer's last block is partial and, at an
    odd address, its first one too), with and without reply types, and the other tables."""
    buf, entries, types = rc.case_entries(pad_front=3)
    want = check(buf, entries, types, rc.IDL, mis, "table")
    assert {w[0] for w in want} == {rc.NONE, rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER, rc.RANGE}
    check(buf, entries, None, rc.IDL, mis, "table, every entry DATA")
    for name, table, bodies in rc.table_cases():
        b, e = rc.back_to_back(bodies, nul=0)
        check(b, e, None, table, mis, name)


def test_mutations_match_plain_rules():
    """The emulator's mutation set on the device: about 20,000 canonical requests with one byte
    flipped, inserted or deleted, or truncated, behind the canonical requests themselves; no
    canonical request defers."""
    canon = rc.canonical_set(0xC0FFEE, 900)
    muts = rc.mutation_set(0xBADC0DE, 20000)
    buf, entries = rc.back_to_back(canon + muts)
    want = check(buf, entries, None, rc.IDL, 3, "mutations")
    assert all(w[0] != rc.DEFER for w in want[:len(canon)])
    assert {w[0] for w in want} == {rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER}


def group_set():
    """1,500 entries over six workgroups: three of the seven methods, unknown methods, invalid
    requests, entries of no group; methods 1, 3, 4, 6 and DEFER stay empty."""
    rng = np.random.default_rng(0x6209)
    bodies, types = [], []
    for k in range(1500):
        pick = int(rng.integers(0, 8))
        rid = int(rng.integers(0, 2**32))
        if pick < 5:
            m = (0, 2, 5, 5, 2)[pick]
            bodies.append(rc.canonical(rc.METHODS[m].decode(), {"k": k}, rid))
        elif pick == 5:
            bodies.append(rc.canonical("nope", None, rid))
        else:
            bodies.append(b'{"id":%d}' % rid)
        types.append(rc.PING if pick == 7 else rc.DATA)
    return bodies, types


def test_groups_are_a_stable_sort():
    bodies, types = group_set()
    buf, entries = rc.back_to_back(bodies)
    entries[700] = (len(buf) + 5, 9)  # RANGE: in no group
    want = check(buf, entries, types, rc.IDL, 0, "groups")
    _, first = rc.groups_of(want, 7)
    sizes = [b - a for a, b in zip(first, first[1:])]
    assert all(sizes[g] > 64 for g in (0, 2, 5, 7, 8)) and all(sizes[g] == 0 for g in (1, 3, 4, 6, 9))
    assert first[-1] < len(entries) - 100  # NONE and RANGE entries are left out
    # one wave, one workgroup and one entry more than a workgroup
    for n in (1, 64, 256, 257):
        check(buf, entries[:n], types[:n], rc.IDL, 0, f"groups, n = {n}")


def filled(n, np_dtype, torch_dtype):
    """n + 2 GUARD elements of FILL bytes; the call gets the address of element GUARD."""
    t = torch.full(((n + 2 * GUARD) * np.dtype(np_dtype).itemsize,), FILL, dtype=torch.uint8, device=DEV)
    return t.view(torch_dtype)


def test_only_what_is_specified_is_written():
    """Every output pre-filled, with guard elements on both sides: entries are written whole,
    d_order only up to the last group's end, nothing else; and every output is optional."""
    bodies, types = group_set()
    buf, entries = rc.back_to_back(bodies)
    n = len(entries)
    want = rc.route_entries(buf, entries, rc.IDL, types)
    worder, wfirst = rc.groups_of(want, 7)
    off, ln, ty = dev_entries(entries, types)
    d_buf, tab = dev_bytes(buf), dev_table(rc.IDL)
    specs = [("kind", np.uint8, torch.uint8, n), ("method", np.uint16, torch.int16, n), ("id", np.uint32, torch.int32, n),
             ("params_off", np.uint32, torch.int32, n), ("params_len", np.uint32, torch.int32, n),
             ("order", np.uint32, torch.int32, n), ("group_first", np.uint32, torch.int32, 7 + 4)]
    fill = {1: FILL, 2: FILL * 0x0101, 4: FILL * 0x01010101}

    def call(given):
        outs = {k: filled(cnt, npd, td) for k, npd, td, cnt in specs}
        ptrs = [outs[k][GUARD:].data_ptr() if k in given else None for k, *_ in specs]
        rcode = _lib.rpc_frames_route_device(d_buf.data_ptr(), d_buf.numel(), off.data_ptr(), ln.data_ptr(),
                                             ty.data_ptr(), n, tab.names.data_ptr(), tab.names.numel(),
                                             tab.offsets.data_ptr(), tab.nmethods, *ptrs, None)
        assert rcode == 0
        torch.cuda.synchronize()
        got = {}
        for k, npd, td, cnt in specs:
            a = outs[k].cpu().numpy().view(npd)
            f = fill[np.dtype(npd).itemsize]
            assert (a[:GUARD] == f).all() and (a[GUARD + cnt:] == f).all(), k
            if k not in given:
                assert (a == f).all(), k
            got[k] = a[GUARD:GUARD + cnt]
        return got

    every = [k for k, *_ in specs]
    got = call(every)
    cols = list(zip(*want))
    for j, k in enumerate(every[:5]):
        assert got[k].tolist() == list(cols[j]), k
    assert got["group_first"].tolist() == wfirst
    assert got["order"][:wfirst[-1]].tolist() == worder
    assert (got["order"][wfirst[-1]:] == fill[4]).all()  # behind the last group: not written
    for given in (["kind"], ["id", "params_len"], ["order", "group_first"], ["method", "order", "group_first"], []):
        part = call(given)
        for j, k in enumerate(every[:5]):
            if k in given:
                assert part[k].tolist() == list(cols[j]), (k, given)
        if "order" in given:
            assert part["group_first"].tolist() == wfirst and part["order"][:wfirst[-1]].tolist() == worder


def test_no_entries():
    tab = dev_table(rc.IDL)
    first = filled(11, np.uint32, torch.int32)
    order = filled(1, np.uint32, torch.int32)
    assert _lib.rpc_frames_route_device(None, 0, None, None, None, 0, tab.names.data_ptr(), tab.names.numel(),
                                        tab.offsets.data_ptr(), 7, None, None, None, None, None,
                                        order[GUARD:].data_ptr(), first[GUARD:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    a = first.cpu().numpy().view(np.uint32)
    assert (a[GUARD:GUARD + 11] == 0).all() and (a[:GUARD] == 0xA5A5A5A5).all() and (a[GUARD + 11:] == 0xA5A5A5A5).all()
    assert (order.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    r = rpc_amd.frames_route(torch.empty(0, dtype=torch.uint8, device=DEV), e, e.to(torch.int32), tab)
    assert r.group_first.cpu().tolist() == [0] * 11 and r.kind.numel() == 0


@pytest.mark.parametrize("nul", [True, False])
def test_scan_unpack_route_on_wire_bytes(nul):
    """Three connections of wire frames built here: requests, PINGs in between, a frame with a
    bad CRC (it closes its connection: the requests behind it are not reached) and a trailing
    partial frame.  Every entry that is not a delivered body reads NONE; the delivered ones read
    what the rules say of their bodies."""
    reqs = rc.canonical_set(0x77, 40) + [b'{"method":"ping","id":01}', b"[1,2,3]", b'{"id":3}']
    conns, want_bodies = [], []
    for c in range(3):
        parts, bodies = [], []
        for k, body in enumerate(reqs[c::3]):
            if k % 4 == 1:
                parts.append(sc.frame(typ=rc.PING))
                bodies.append(None)
            if c == 1 and k == 9:
                parts.append(sc.frame(body, crc=0x12345678))
                bodies.append(None)
                parts += [sc.frame(b) for b in reqs[:3]]  # not reached
                bodies += [None] * 3
                break
            parts.append(sc.frame(body))
            bodies.append(body)
        if c == 2:
            parts.append(sc.frame(reqs[0])[:20])  # a partial frame: left for the next read
        conns.append(b"".join(parts))
        want_bodies += bodies
    lens = [len(c) for c in conns]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    raw = dev_bytes(b"".join(conns))
    s = rpc_amd.frames_scan(raw, to_dev(offs), to_dev(np.array(lens, dtype=np.int64)), role="server", verify=True)
    u = rpc_amd.frames_unpack(raw, s.frame_offsets, s.verdict, role="server", nul=nul, conn_first=s.conn_first)
    r = rpc_amd.frames_route(u.bodies, u.body_offsets, u.body_lens, dev_table(rc.IDL), reply_types=u.reply_types)
    torch.cuda.synchronize()
    assert s.nframes == len(want_bodies)
    rows = rows_of(r, s.nframes)
    for i, (row, body) in enumerate(zip(rows, want_bodies)):
        assert row == ((rc.NONE, rc.NO_METHOD, 0, 0, 0) if body is None else rc.route_body(body)), (i, body, row)
    assert sum(1 for b in want_bodies if b is None) >= 10
    assert {row[0] for row in rows} == {rc.NONE, rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER}
    first = r.group_first.cpu().tolist()
    order = r.order.cpu().tolist()[:first[-1]]
    assert (order, first) == rc.groups_of(rows, 7)
