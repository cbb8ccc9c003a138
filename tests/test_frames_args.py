"""Frame args on the GPU (rpc_frames_args_device): the declared parameters of
every routed request as typed slots.  Against the plain Python rules of tests/args_cases.py on
all three outputs, DEFER included; and route -> args on request bodies built here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import args_cases as ac  # noqa: E402
import route_cases as rc  # noqa: E402
from test_frames_route import DEV, FILL, GUARD, dev_bytes, filled, to_dev  # noqa: E402


def dev_schema(schema):
    """An args_cases.Schema, broken words and all, as rpc_amd.ArgsSchema."""
    u32 = lambda ws: to_dev(np.array(ws, dtype=np.uint32).view(np.int32))  # noqa: E731
    return rpc_amd.ArgsSchema(u32(schema.first), to_dev(np.array(schema.types, dtype=np.uint8)), u32(schema.noff),
                              to_dev(np.frombuffer(schema.names, dtype=np.uint8).copy()), schema.nmethods,
                              len(schema.types), 0)


def dev_entries(entries):
    """(body_offsets, body_lens, FrameRoute) of args_cases entries."""
    col = lambda j, wide, narrow: to_dev(np.array([e[j] for e in entries], dtype=wide).view(narrow))  # noqa: E731
    route = rpc_amd.FrameRoute(col(2, np.uint8, np.uint8), col(3, np.uint16, np.int16), None, col(4, np.uint32, np.int32),
                               col(5, np.uint32, np.int32), None, None)
    return col(0, np.uint64, np.int64), col(1, np.uint32, np.int32), route


def rows_of(r, n):
    st = r.status.cpu().numpy().view(np.uint8)
    rs = r.reply_status.cpu().numpy().view(np.int32)
    sl = r.slots.cpu().numpy().view(np.uint64)
    assert sl.shape == (r.slots.shape[0], n)
    return [(int(st[i]), int(rs[i]), tuple(int(x) for x in sl[:, i])) for i in range(n)]


def check(buf, entries, schema=ac.IDL, width=ac.MAX_PARAMS, mis=0, what="", stream=None):
    off, ln, route = dev_entries(entries)
    r = rpc_amd.frames_args(dev_bytes(buf, mis), off, ln, route, dev_schema(schema), width=width, stream=stream)
    torch.cuda.synchronize()
    rows = rows_of(r, len(entries))
    want = ac.args_entries(buf, entries, schema, width)
    for k, (g, w) in enumerate(zip(rows, want)):
        e = entries[k]
        assert g == w, (what, k, e, buf[e[0] + e[4]:e[0] + e[4] + e[5]][:80] if e[0] < len(buf) else b"", g, w)
    return want


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_table_matches_plain_rules(mis):
    """The case table as one buffer (every status and every kind that is not CALL; the last span
    ends on the buffer's last byte; at an odd address the buffer's first block is partial too),
    at width 8 and 3, and the other schemas: 0 and 8 parameters, width 1, the empty name, a
    repeated name, every broken schema word."""
    buf, entries = ac.case_entries(pad_front=3)
    want = check(buf, entries, mis=mis, what="table")
    assert {w[0] for w in want} == {ac.NONE, ac.OK, ac.INVALID, ac.DEFER, ac.RANGE, ac.BAD_SCHEMA}
    assert {e[2] for e in entries} >= {0, 1, 2, 3, 4, 5, 6, 255}
    assert any(e[2] == rc.CALL and e[0] + e[4] + e[5] == len(buf) and e[5] for e in entries)
    check(buf, entries, width=3, mis=mis, what="table, width 3")
    for name, schema, width, b, e, _ in ac.schema_cases():
        check(b, e, schema, width, mis, name)


def test_mutations_match_plain_rules():
    """The emulator's mutation set on the device: 20,000 canonical params with one byte flipped,
    inserted or deleted, or truncated, behind the canonical params themselves (all seven
    methods inside every wave); every canonical span decodes."""
    canon = ac.canonical_set(0xA265, 1400)
    muts = ac.mutation_set(0xBADA265, 20000)
    buf, entries = ac.back_to_back(canon + muts)
    want = check(buf, entries, mis=3, what="mutations")
    assert all(w[0] == ac.OK for w in want[:len(canon)])
    assert {m for m, _ in canon[:64]} == set(range(7))
    assert {w[0] for w in want} == {ac.OK, ac.INVALID, ac.DEFER}


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_around_one_workgroup(n):
    reqs = (ac.canonical_set(0x51, 200) + ac.mutation_set(0x52, 57))[:n]
    buf, entries = ac.back_to_back(reqs, nul=0)
    check(buf, entries, mis=1, what=f"n = {n}")


def test_long_bodies_need_several_rounds():
    """300 bodies of 1,000 bytes, back to back from an odd offset: a workgroup's spans fill
    several staging rounds and spans straddle the rounds' ends."""
    rng = np.random.default_rng(0x1000)
    reqs = []
    for k in range(300):
        if k % 5 == 4:  # a long extra member in front of the parameters
            span = b'{"pad":"%s","a":%d,"b":-2.5e-3,"ok":true}' % (b"p" * 900, k)
            reqs.append((ac.X, span))
        else:
            text = bytes(rng.choice(np.frombuffer(b"abcdefghij klmnop\xc3\xa9", dtype=np.uint8), 1000))
            reqs.append((ac.S, b'{"s":"' + text[:1000 - 61 - len(b"%d" % k)] + b'"}'))
    buf, entries = ac.back_to_back(reqs, pad_front=7, nul=1)
    assert sum(1 for e in entries if e[1] == 1000) >= 200
    starts = {(e[0] + e[4]) // 32768 for e in entries}
    assert len(starts) >= 8  # (the spans of a workgroup lie in several windows)
    want = check(buf, entries, mis=9, what="long bodies")
    assert all(w[0] == ac.OK for w in want)


def test_a_stream_of_its_own():
    buf, entries = ac.back_to_back(ac.canonical_set(0x57, 700))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check(buf, entries, what="stream", stream=s)


def test_only_what_is_specified_is_written():
    """Every output pre-filled, with guard elements on both sides: each is written whole and
    nothing else is, and every output is optional (each left NULL in turn)."""
    buf, entries = ac.back_to_back(ac.canonical_set(0x61, 300) + ac.mutation_set(0x62, 300))
    n, width = len(entries), 5
    want = ac.args_entries(buf, entries, ac.IDL, width)
    off, ln, route = dev_entries(entries)
    d_buf, sc = dev_bytes(buf), dev_schema(ac.IDL)
    specs = [("slots", np.uint64, torch.int64, width * n), ("status", np.uint8, torch.uint8, n),
             ("reply_status", np.uint32, torch.int32, n)]
    fill = {1: FILL, 4: FILL * 0x01010101, 8: FILL * 0x0101010101010101}

    def call(given):
        outs = {k: filled(cnt, npd, td) for k, npd, td, cnt in specs}
        ptrs = [outs[k][GUARD:].data_ptr() if k in given else None for k, *_ in specs]
        rcode = _lib.rpc_frames_args_device(d_buf.data_ptr(), d_buf.numel(), off.data_ptr(), ln.data_ptr(),
                                            route.kind.data_ptr(), route.method.data_ptr(), route.params_off.data_ptr(),
                                            route.params_len.data_ptr(), n, sc.first.data_ptr(), sc.nmethods,
                                            sc.types.data_ptr(), sc.name_off.data_ptr(), sc.nparams, sc.names.data_ptr(),
                                            sc.names.numel(), width, *ptrs, None)
        assert rcode == 0
        torch.cuda.synchronize()
        for k, npd, td, cnt in specs:
            a = outs[k].cpu().numpy().view(npd)
            f = fill[np.dtype(npd).itemsize]
            assert (a[:GUARD] == f).all() and (a[GUARD + cnt:] == f).all(), k
            if k not in given:
                assert (a == f).all(), k
                continue
            got = a[GUARD:GUARD + cnt]
            if k == "slots":
                assert got.reshape(width, n).T.tolist() == [list(w[2]) for w in want], given
            else:
                assert got.tolist() == [w[1] & 0xFFFFFFFF if k == "reply_status" else w[0] for w in want], (k, given)

    for given in (["slots", "status", "reply_status"], ["status", "reply_status"], ["slots", "reply_status"],
                  ["slots", "status"], ["slots"], []):
        call(given)


def test_route_then_args():
    """frames_route's own device outputs go into frames_args unchanged; one list builds the
    table and the schema; an F64 column reads as float64."""
    methods = [(name.decode(), [(p.decode(), t) for p, t in params]) for name, params in ac.IDL_METHODS]
    table = rpc_amd.route_table([m for m, _ in methods], device=DEV)
    schema = rpc_amd.args_schema(methods, device=DEV)
    assert (schema.nmethods, schema.nparams, schema.width) == (7, 10, 3)
    bodies = [ac.request(ac.IDL_METHODS[m][0], span, rid=k)[0] for k, (m, span) in enumerate(ac.canonical_set(0x71, 400))]
    bodies += [b'{"method":"nope","id":1}', b"[1]", b'{"method":"mul_double","params":{"a":1.5,"b":"x"},"id":2}',
               b'{"method":"mul_double","params":{"a":1.5,"b":-0.25},"id":3}']
    buf, ents = rc.back_to_back(bodies)
    off = to_dev(np.array([e[0] for e in ents], dtype=np.int64))
    ln = to_dev(np.array([e[1] for e in ents], dtype=np.int32))
    d_buf = dev_bytes(buf)
    rt = rpc_amd.frames_route(d_buf, off, ln, table)
    r = rpc_amd.frames_args(d_buf, off, ln, rt, schema)
    torch.cuda.synchronize()
    routed = rc.route_entries(buf, ents)
    entries = [(o, n, row[0], row[1], row[3], row[4]) for (o, n), row in zip(ents, routed)]
    assert rows_of(r, len(ents)) == ac.args_entries(buf, entries, ac.IDL, 3)
    assert r.status.cpu().tolist()[-4:] == [ac.NONE, ac.NONE, ac.INVALID, ac.OK]
    assert r.reply_status.cpu().tolist()[-2:] == [-32602, 0]
    assert r.slots[:2, -1].view(torch.float64).cpu().tolist() == [1.5, -0.25]


def test_no_entries():
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    i32 = e.to(torch.int32)
    route = rpc_amd.FrameRoute(e.to(torch.uint8), e.to(torch.int16), None, i32, i32, None, None)
    r = rpc_amd.frames_args(torch.empty(0, dtype=torch.uint8, device=DEV), e, i32, route, dev_schema(ac.IDL), width=2)
    assert r.status.numel() == 0 and tuple(r.slots.shape) == (2, 0)
