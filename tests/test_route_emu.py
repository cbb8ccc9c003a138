"""CPU emulation of the frame route (tests/cpu_emu/route_emu.cpp) against the plain rules
(tests/route_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_route.h -- the precheck, the strict automaton, the method compare, the
bucket and rank helpers -- and runs the staging rounds, the walk over the staged bytes and the
three grouping passes as the kernels run them, at the kernel's staging size and at a small one
(so that bodies straddle the edges of a round), with the body buffer at aligned and at odd
addresses.  Its readers abort on any byte outside [0, bodies_bytes), outside what a round
staged, or outside the table."""
import os
import re
import subprocess

import pytest

import route_cases as rc
import stage_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_route.h")


def kernel_constant(name):
    m = re.search(r"constexpr uint32_t %s = (\d+);" % name, open(ROUTE_H).read())
    assert m, f"{name} not found in {ROUTE_H}"
    return int(m.group(1))


S_K = kernel_constant("kRouteStage")
S_SMALL = 1088  # a multiple of 16 that just holds one body at any alignment: almost every round is cut
#: (staging bytes, low address bits of the body buffer)
SHAPES = [(S_K, 0), (S_K, 5), (S_SMALL, 0), (S_SMALL, 11), (S_SMALL, 15)]


@pytest.fixture(scope="module")
def route_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("route_emu")
    exe, src = str(d / "route_emu"), os.path.join(REPO, "tests", "cpu_emu", "route_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(route_emu, stage, mis, buf, entries, types, table):
    """(rows, order, group_first) of one emulator run."""
    exe, d = route_emu
    bp, ep, np_, op = (str(d / n) for n in ("bodies.bin", "entries.txt", "names.bin", "offs.txt"))
    open(bp, "wb").write(buf)
    tt = types if types is not None else [0] * len(entries)
    open(ep, "w").write("".join("%d %d %d\n" % (o, ln, t) for (o, ln), t in zip(entries, tt)))
    open(np_, "wb").write(table.names)
    open(op, "w").write("".join("%d\n" % o for o in table.offs))
    p = subprocess.run([exe, str(stage), str(mis), "0" if types is None else "1", bp, ep, np_, op],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    rows = [tuple(map(int, ln.split())) for ln in lines[:len(entries)]]
    order = [int(x) for x in lines[len(entries)].split()[1:]]
    first = [int(x) for x in lines[len(entries) + 1].split()[1:]]
    return rows, order, first


def check(route_emu, stage, mis, buf, entries, types, table, what):
    rows, order, first = run_emu(route_emu, stage, mis, buf, entries, types, table)
    want = rc.route_entries(buf, entries, table, types)
    for i, (g, w) in enumerate(zip(rows, want)):
        assert g == w, (what, i, entries[i], buf[entries[i][0]:entries[i][0] + entries[i][1]][:80], g, w)
    assert len(rows) == len(want)
    worder, wfirst = rc.groups_of(want, table.nmethods)
    assert first == wfirst and order == worder, what
    return want


def test_rules_on_the_stated_cases():
    """The plain rules give each case of the table the kind written beside it, every kind
    occurs, and the limit cases sit exactly on their limits."""
    for name, body, kind in rc.CASES:
        got = rc.route_body(body)
        assert kind is None or got[0] == kind, (name, got)
    buf, entries, types = rc.case_entries()
    kinds = {r[0] for r in rc.route_entries(buf, entries, types=types)}
    assert kinds == {rc.NONE, rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER, rc.RANGE}
    by_name = {n: b for n, b, _ in rc.CASES}
    assert rc.Strict(by_name["tokens 256"]).tokens == 256 and rc.Strict(by_name["tokens 255"]).tokens == 255
    assert len(by_name["length 1024"]) == 1024 and len(by_name["length 1025"]) == 1025
    assert rc.route_body(by_name["id 007"])[0] == rc.DEFER
    assert rc.route_body(by_name["id max"])[2] == 4294967295
    assert rc.route_body(by_name["duplicate id"])[2] == 0  # the first id, a string, wins
    b = by_name["params array"]
    _, m, rid, po, pl = rc.route_body(b)
    assert b[po:po + pl] == b'[1,[2,{"a":"]"}]]' and rc.METHODS[m] == b"is_even" and rid == 1
    b = by_name["params number last"]
    assert b[rc.route_body(b)[3]:][:rc.route_body(b)[4]] == b"12"
    b = by_name["params string"]
    assert b[rc.route_body(b)[3]:][:rc.route_body(b)[4]] == b'"a\\"}b"'


@pytest.mark.parametrize("stage,mis", SHAPES)
def test_table_matches_plain_rules(route_emu, stage, mis):
    """The case table as one buffer, with and without reply types, and the other tables: 0 and
    256 methods, duplicate names, prefixes, broken offset words."""
    buf, entries, types = rc.case_entries(pad_front=3)
    check(route_emu, stage, mis, buf, entries, types, rc.IDL, "table")
    check(route_emu, stage, mis, buf, entries, None, rc.IDL, "table, every entry DATA")
    for name, table, bodies in rc.table_cases():
        b, e = rc.back_to_back(bodies)
        want = check(route_emu, stage, mis, b, e, None, table, name)
        if name == "no methods":
            assert all(w[0] in (rc.NOT_FOUND, rc.INVALID) for w in want)
        if name == "256 methods":
            assert [w[1] for w in want[3:6]] == [255, 0, 25]
        if name == "duplicate names":
            assert want[0][:2] == (rc.CALL, 0)
        if name in ("prefix first", "prefix last"):
            assert {w[0] for w in want[:2]} == {rc.CALL} and want[0][1] != want[1][1]
        if name == "empty name":
            assert want[2][:2] == (rc.CALL, 1)
        if name == "non-monotone word":
            assert want[0][:2] == (rc.CALL, 2) and want[1][0] == rc.NOT_FOUND and want[4][0] == rc.NOT_FOUND
        if name == "word leaves the names":
            assert want[0][:2] == (rc.CALL, 1) and want[4][0] == rc.NOT_FOUND
    check(route_emu, stage, mis, b"", [], None, rc.IDL, "no entries")


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 7)])
def test_mutations_match_plain_rules(route_emu, stage, mis):
    """About 20,000 canonical requests with one byte flipped, inserted or deleted, or truncated,
    and the canonical requests themselves: field for field, DEFER included.  No canonical request
    defers; the mutations reach every kind a body can have."""
    canon = rc.canonical_set(0xC0FFEE, 900)
    muts = rc.mutation_set(0xBADC0DE, 20000)
    buf, entries = rc.back_to_back(canon + muts, nul=1)
    want = check(route_emu, stage, mis, buf, entries, None, rc.IDL, "mutations")
    assert all(w[0] != rc.DEFER for w in want[:len(canon)])
    assert {w[0] for w in want[:len(canon)]} == {rc.CALL, rc.NOT_FOUND, rc.INVALID}
    assert {w[0] for w in want[len(canon):]} == {rc.CALL, rc.NOT_FOUND, rc.INVALID, rc.DEFER}
    routed = sum(1 for w in want[len(canon):] if w[0] != rc.DEFER)
    assert 1000 < routed < 19000  # both sides of the strict subset are exercised


@pytest.mark.parametrize("stage,odd", [(S_K, 5), (S_SMALL, 11)])
def test_placements_match_plain_rules(route_emu, stage, odd, monkeypatch):
    """Bodies anywhere (tests/stage_cases.py): memory order reversed and shuffled, fixed slots, all
    lanes on one span and on two far apart, every prefix and suffix of one text, bodies that end
    on a window's last byte and one byte behind it, bodies on the buffer's first and last byte at
    every address, and all of them in one call.  Each input has the property it was built for
    (by stage_cases.rounds, at the kernel's staging size); rows and groups are the plain rules',
    and the emulator's rounds are the ones stage_cases.rounds gives at the stage in use, with no
    block read bytewise that lies wholly inside the buffer."""
    bodies = sc.route_set()
    trace = str(route_emu[1] / "rounds.txt")
    monkeypatch.setenv("RPC_EMU_STAGE_TRACE", trace)

    def check_placed(emu, stage, mis, buf, spans, types, table, what):
        want = check(emu, stage, mis, buf, spans, types, table, what)
        assert sc.read_trace(trace) == sc.trace(spans, sc.walked(buf, spans), mis, len(buf), stage), what
        return want

    for mis in (0, odd):
        for name in sc.BATCH:
            p = sc.batch(name, bodies, sc.request)
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(route_emu, stage, mis, p.buf, p.spans, None, rc.IDL, (name, mis))
            if name == "nested":
                assert {w[2] for w in want} == {0, 4000000031} and len({w for w in want}) == 2
        for p in sc.window_edges(sc.request, mis, stage):
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(route_emu, stage, mis, p.buf, p.spans, None, rc.IDL, (p.name, mis))
            assert [w[2] for w in want] == [4000000001, 4000000002, 4000000002]
        buf, spans, placed = sc.mixture(bodies, sc.request, mis)
        want = check_placed(route_emu, stage, mis, buf, spans, None, rc.IDL, ("mixture", mis))
        assert want == [rc.route_body(b) for b in placed]
        counts = [len(g) for g in sc.rounds(spans, sc.walked(buf, spans), mis)]
        assert counts[0] >= 128 and counts[1] == 1 and len(counts) >= 4
    for mis in range(16):
        ends = [sc.buffer_ends(sc.request, mis)] + [sc.whole_buffer(sc.WHOLE, mis)] * (mis in sc.WHOLE_MIS)
        for p in ends:
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(route_emu, stage, mis, p.buf, p.spans, None, rc.IDL, p.name)
            assert [w[2] for w in want] in ([4000000003, 4000000004], [7])
