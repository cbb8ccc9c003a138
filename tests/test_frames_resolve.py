"""Frame resolve on the GPU (rpc_frames_resolve_device): the JSON-RPC reply
envelope of every delivered body, matched to the pending ids.  Against the plain Python rules of
tests/resolve_cases.py field for field, DEFER included; and a loopback on wire bytes built on
the device: route -> reply -> pack -> scan + verify -> unpack -> resolve."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import resolve_cases as rc  # noqa: E402
import route_cases as rtc  # noqa: E402

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


def dev_call(call, mis=0):
    off = to_dev(np.array(call.offs, dtype=np.uint64).view(np.int64))
    ln = to_dev(np.array(call.lens, dtype=np.uint32).view(np.int32))
    ty = None if call.types is None else to_dev(np.array(call.types, dtype=np.uint16).view(np.int16))
    pend = to_dev(np.array(call.pending, dtype=np.uint32).view(np.int32))
    return dev_bytes(call.buf, mis), off, ln, pend, ty


def u32(x):
    return x.cpu().numpy().view(np.uint32).tolist()


def resolved_of(r):
    nopen = int(r.nopen.cpu()[0])
    return rc.Resolved(r.kind.cpu().numpy().tolist(), u32(r.id), u32(r.result_off), u32(r.result_len),
                       u32(r.error_off), u32(r.error_len), u32(r.slot), u32(r.slot_entry), u32(r.open)[:nopen])


def same(got, want, what):
    for field in rc.Resolved._fields:
        g, w = getattr(got, field), getattr(want, field)
        bad = [i for i, (a, b) in enumerate(zip(g, w)) if a != b]
        assert not bad and len(g) == len(w), (what, field, len(g), len(w), bad[:5], [(g[i], w[i]) for i in bad[:5]])


def check(call, mis=0, what=""):
    bodies, off, ln, pend, ty = dev_call(call, mis)
    r = rpc_amd.frames_resolve(bodies, off, ln, pend, reply_types=ty)
    torch.cuda.synchronize()
    want = call.expect()
    same(resolved_of(r), want, what)
    return want


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_table_matches_plain_rules(mis):
    """The case table as one call: every key in upper, lower and mixed case, a wrong-type id in
    front of a good one, both members and neither, null values, ids 0 and 4294967295, the three
    limits.  Without a NUL the last body ends at the buffer's last byte, whose block is partial
    (and at an odd address the first one too)."""
    for nul in (0, 1):
        _, call = rc.case_call(nul=nul)
        want = check(call, mis, "table nul=%d" % nul)
        assert set(want.kind) == {rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE, rc.INVALID, rc.DEFER}


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_two_staging_rounds(mis):
    """40 bodies of 1,024 B do not fit one round of 32 KiB."""
    want = check(rc.big_bodies_call(), mis, "40 bodies of 1,024 B")
    assert set(want.kind) == {rc.MATCHED} and not want.open


@pytest.mark.parametrize("name", sorted(rc.join_calls()))
def test_join_shapes(name):
    """64 pending ids in one cell of a table whose run wraps, an id held by slots 3 and 9, three
    replies to one id at entries 1, 255 and 256, a reply nobody waits for, npending 0 / 1 / 2 /
    257, no entries, a non-DATA entry with a garbage offset, spans outside the buffer and an
    offset near 2^64."""
    check(rc.join_calls()[name], 0, name)


@pytest.mark.parametrize("n", [1, 256, 257])
def test_entry_counts(n):
    """One lane, one full workgroup, one lane of a second workgroup; the ids a shuffled range."""
    rng = np.random.default_rng(n)
    ids = rng.permutation(n).tolist()
    bodies = [rc.reply(i, result={"v": i}) for i in ids]
    pending = rng.permutation(n).tolist()
    want = check(rc.Call(*rc.pack_bodies(bodies, nul=0), None, pending), 5, "n=%d" % n)
    assert set(want.kind) == {rc.MATCHED} and not want.open
    assert [want.slot_entry[s] for s in range(n)] == [ids.index(pending[s]) for s in range(n)]


def test_mutations_match_plain_rules():
    """The emulator's mutation set on the device, behind the canonical replies themselves; no
    canonical reply defers."""
    canon = rc.canonical_set(0xC0FFEE, 900)
    muts = rc.mutation_set(0xBADC0DE, 20000)
    buf, offs, lens = rc.pack_bodies(canon + muts, nul=1)
    ids = [rc.decode_body(b)[1] for b in canon[::2]] + [1, 2, 3]
    want = check(rc.Call(buf, offs, lens, None, ids), 3, "mutations")
    assert all(k in (rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE) for k in want.kind[:len(canon)])
    assert set(want.kind) == {rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE, rc.INVALID, rc.DEFER}


OUTPUTS = ["kind", "id", "result_off", "result_len", "error_off", "error_len", "slot", "slot_entry", "open"]


@pytest.mark.parametrize("absent", OUTPUTS + ["all"])
def test_each_output_is_optional_and_nothing_else_is_written(absent):
    """Each output NULL in turn (d_open and d_nopen go together), and all of them: the others are
    what the full call gives, and no output is written outside its n or npending elements."""
    _, call = rc.case_call(nul=1)
    want = call.expect()
    n, npending = len(call.offs), len(call.pending)
    bodies, off, ln, pend, _ = dev_call(call)
    size = {"kind": n, "slot_entry": npending, "open": npending}
    outs = {}
    for k in OUTPUTS + ["nopen"]:
        dt = torch.uint8 if k == "kind" else torch.int32
        outs[k] = torch.full((size.get(k, 1 if k == "nopen" else n) + 2 * GUARD,), FILL, dtype=dt, device=DEV)
    gone = set(OUTPUTS + ["nopen"]) if absent == "all" else {absent} | ({"nopen"} if absent == "open" else set())
    ptr = lambda k: None if k in gone else outs[k][GUARD:].data_ptr()  # noqa: E731
    rc_ = _lib.rpc_frames_resolve_device(bodies.data_ptr(), bodies.numel(), off.data_ptr(), ln.data_ptr(), None, n,
                                         pend.data_ptr(), npending, ptr("kind"), ptr("id"), ptr("result_off"),
                                         ptr("result_len"), ptr("error_off"), ptr("error_len"), ptr("slot"),
                                         ptr("slot_entry"), ptr("open"), ptr("nopen"), None)
    assert rc_ == 0
    torch.cuda.synchronize()
    assert rpc_amd.device_status() == 0
    for k in OUTPUTS + ["nopen"]:
        host = outs[k].cpu().numpy()
        host = host if k == "kind" else host.view(np.uint32)
        fill = FILL  # (torch.full fills elements, not bytes)
        count = len(host) - 2 * GUARD
        assert (host[:GUARD] == fill).all() and (host[GUARD + count:] == fill).all(), k
        body = host[GUARD:GUARD + count].tolist()
        if k in gone:
            assert all(v == fill for v in body), k
        elif k == "nopen":
            assert body == [len(want.open)]
        elif k == "open":
            assert body[:len(want.open)] == want.open and all(v == fill for v in body[len(want.open):])
        else:
            assert body == getattr(want, k), k


def test_no_entries_leaves_every_slot_open():
    pend = to_dev(np.array([9, 8, 7], dtype=np.uint32).view(np.int32))
    empty64 = torch.empty(0, dtype=torch.int64, device=DEV)
    empty32 = torch.empty(0, dtype=torch.int32, device=DEV)
    r = rpc_amd.frames_resolve(torch.empty(0, dtype=torch.uint8, device=DEV), empty64, empty32, pend)
    torch.cuda.synchronize()
    assert u32(r.slot_entry) == [rc.NO_SLOT] * 3 and u32(r.open) == [0, 1, 2] and int(r.nopen.cpu()[0]) == 3


def test_einval_on_the_device_too():
    assert _lib.rpc_frames_resolve_device(None, 0, None, None, None, 0xFFFFFFFF, None, 0, *([None] * 11)) == -22
    assert _lib.rpc_frames_resolve_device(None, 0, None, None, None, 0, None, (1 << 24) + 1, *([None] * 11)) == -22


def test_loopback_route_reply_pack_scan_unpack_resolve():
    """A server's round and a client's on one device.  300 requests with ids a shuffled range, on
    two connections, go route -> reply -> pack on the server side; the wire bytes go scan + verify
    (role="client") -> unpack -> resolve on the client side.  Every slot is matched, nothing stays
    open, and every result span is the value the handler gave."""
    n = 300
    rng = np.random.default_rng(0x10095)
    ids = rng.permutation(n).tolist()
    reqs = [rtc.canonical("echo_i64", {"x": i}, i) for i in ids]
    rbuf, rentries = rtc.back_to_back(reqs)
    i64 = lambda a: to_dev(np.asarray(a, dtype=np.uint64).view(np.int64))  # noqa: E731
    i32 = lambda a: to_dev(np.asarray(a, dtype=np.uint32).view(np.int32))  # noqa: E731
    table = rpc_amd.route_table(rtc.METHODS)
    rt = rpc_amd.frames_route(dev_bytes(rbuf), i64([e[0] for e in rentries]), i32([e[1] for e in rentries]), table,
                              group=False)
    assert (rt.kind.cpu().numpy() == rpc_amd.ROUTE_CALL).all()
    # the handlers: request id i gets the value {"v":[i, "i"]}
    values = [json.dumps({"v": [i, str(i)]}, separators=(",", ":")).encode() for i in ids]
    vbuf, ventries = rtc.back_to_back(values, nul=0)
    conn = i64([0, 100, n])
    rep = rpc_amd.frames_reply(rt.kind, rt.id, dev_bytes(vbuf, 3), i64([e[0] for e in ventries]),
                               i32([e[1] for e in ventries]), conn_first=conn)
    p = rpc_amd.frames_pack(rep.bodies, rep.body_offsets, rep.body_lens, types=rep.types, conn_first=conn)
    cbf = p.conn_bytes_first.cpu().numpy().view(np.uint64)
    sc = rpc_amd.frames_scan(p.stream, i64(cbf[:2]), i64([cbf[1] - cbf[0], cbf[2] - cbf[1]]), role="client", verify=True)
    assert sc.nframes == n
    u = rpc_amd.frames_unpack(p.stream, sc.frame_offsets, sc.verdict, role="client", nul=True)
    pending = rng.permutation(n).tolist()  # slot s waits for id pending[s]
    r = rpc_amd.frames_resolve(u.bodies, u.body_offsets[:n].contiguous(), u.body_lens[:n].contiguous(), i32(pending),
                               reply_types=u.reply_types[:n].contiguous())
    torch.cuda.synchronize()
    got = resolved_of(r)
    assert got.kind == [rc.MATCHED] * n and got.open == [] and int(r.nopen.cpu()[0]) == 0
    assert got.id == ids and got.error_len == [0] * n
    assert sorted(got.slot_entry) == list(range(n)) and got.slot == [pending.index(i) for i in ids]
    body = u.bodies.cpu().numpy().tobytes()
    at = u.body_offsets.cpu().numpy().view(np.uint64)
    for e in range(n):
        a = int(at[e]) + got.result_off[e]
        assert body[a:a + got.result_len[e]] == values[e], e
