"""CPU emulation of the frame args (tests/cpu_emu/args_emu.cpp) against the plain rules
(tests/args_cases.py).  The emulator compiles the kernel's own source,
rpc_amd/csrc/frames_args.h -- the precheck, the strict walk with its key compares, the
conversions -- and runs the staging rounds over the `params` spans, the walk over the staged
bytes and the slot stores as the kernel runs them, at the kernel's staging size and at a small
one (so that spans straddle the edges of a round), with the body buffer at aligned and at odd
addresses.  Its readers abort on any byte outside [0, bodies_bytes), outside what a round
staged, or outside the schema's arrays."""
import os
import subprocess

import pytest

import args_cases as ac
import route_cases as rc
import stage_cases as sc
from test_route_emu import S_K, S_SMALL, SHAPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def args_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("args_emu")
    exe, src = str(d / "args_emu"), os.path.join(REPO, "tests", "cpu_emu", "args_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(args_emu, stage, mis, buf, entries, schema=ac.IDL, width=ac.MAX_PARAMS):
    """(status, reply_status, slots) per entry of one emulator run."""
    exe, d = args_emu
    bp, ep, sp = (str(d / n) for n in ("bodies.bin", "entries.txt", "schema.txt"))
    open(bp, "wb").write(buf)
    open(ep, "w").write("".join("%d %d %d %d %d %d\n" % e for e in entries))
    words = lambda tag, ws: tag + "".join(" %d" % w for w in ws) + "\n"  # noqa: E731
    open(sp, "w").write(words("first", schema.first) + words("types", schema.types) + words("noff", schema.noff) +
                        "names " + schema.names.hex() + "\n")
    p = subprocess.run([exe, "run", str(stage), str(mis), str(width), bp, ep, sp], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = []
    for ln in p.stdout.splitlines():
        f = ln.split()
        rows.append((int(f[0]), int(f[1]), tuple(int(x) for x in f[2:])))
    return rows


def span_of(buf, e):
    return buf[e[0] + e[4]:e[0] + e[4] + e[5]][:80] if e[0] < len(buf) else b""


def check(args_emu, stage, mis, buf, entries, schema=ac.IDL, width=ac.MAX_PARAMS, what=""):
    rows = run_emu(args_emu, stage, mis, buf, entries, schema, width)
    want = ac.args_entries(buf, entries, schema, width)
    assert len(rows) == len(want)
    for k, (g, w) in enumerate(zip(rows, want)):
        assert g == w, (what, k, entries[k], span_of(buf, entries[k]), g, w)
    return want


def test_rules_on_the_stated_cases():
    """The plain rules give each case of the table the status and the slots written beside it,
    every status occurs, and the limit cases sit exactly on their limits."""
    buf, entries = ac.back_to_back([(m, span) for _, m, span, _, _ in ac.CASES])
    got = ac.args_entries(buf, entries)
    for (name, m, span, status, slots), (st, reply, sl), e in zip(ac.CASES, got, entries):
        assert st == status, (name, st)
        assert reply == {ac.OK: 0, ac.INVALID: -32602}.get(status, -32603), name
        if slots is not None:
            assert sl == tuple(slots + [0] * (8 - len(slots))), (name, sl)
        if status != ac.OK:
            assert sl == (0,) * 8, name
        if m == ac.S and status == ac.OK:  # a STR slot is the bytes between the quotes
            at, ln = sl[0] & 0xFFFFFFFF, sl[0] >> 32
            assert b'{"s":"' + buf[e[0] + at:e[0] + at + ln] + b'"}' == span, name
    buf, entries = ac.case_entries()
    assert {r[0] for r in ac.args_entries(buf, entries)} == {ac.NONE, ac.OK, ac.INVALID, ac.DEFER, ac.RANGE, ac.BAD_SCHEMA}
    by_name = {c[0]: c[2] for c in ac.CASES}
    assert [ac.Span(by_name["tokens %d" % k]).tokens for k in (255, 256)] == [255, 256]
    assert [len(by_name["span %d" % k]) for k in (1024, 1025)] == [1024, 1025]
    for name, schema, width, buf, entries, want in ac.schema_cases():
        assert [r[0] for r in ac.args_entries(buf, entries, schema, width)] == want, name


@pytest.mark.parametrize("stage,mis", SHAPES)
def test_table_matches_plain_rules(args_emu, stage, mis):
    """The case table as one buffer, at width 8 and at width 3, and the other schemas: 0 and 8
    parameters, width 1, the empty name, a repeated name, every broken schema word."""
    buf, entries = ac.case_entries(pad_front=3)
    check(args_emu, stage, mis, buf, entries, what="table")
    check(args_emu, stage, mis, buf, entries, width=3, what="table, width 3")
    for name, schema, width, b, e, _ in ac.schema_cases():
        check(args_emu, stage, mis, b, e, schema, width, name)
    check(args_emu, stage, mis, b"", [], what="no entries")


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 7)])
def test_mutations_match_plain_rules(args_emu, stage, mis):
    """20,000 canonical params with one byte flipped, inserted or deleted, or truncated, and
    the canonical params themselves: field for field, DEFER included.  Every canonical span
    decodes; the mutations reach both sides of the strict subset."""
    canon = ac.canonical_set(0xA265, 1400)
    muts = ac.mutation_set(0xBADA265, 20000)
    buf, entries = ac.back_to_back(canon + muts, nul=1)
    want = check(args_emu, stage, mis, buf, entries, what="mutations")
    assert all(w[0] == ac.OK for w in want[:len(canon)])
    n = {s: sum(1 for w in want[len(canon):] if w[0] == s) for s in (ac.OK, ac.INVALID, ac.DEFER)}
    assert sum(n.values()) == len(muts) and min(n.values()) >= 1000, n


@pytest.mark.parametrize("stage,odd", [(S_K, 5), (S_SMALL, 11)])
def test_placements_match_plain_rules(args_emu, stage, odd, monkeypatch):
    """`params` spans anywhere (tests/stage_cases.py): memory order reversed and shuffled, fixed
    slots, all lanes on one span and on two far apart, every prefix and suffix of one text, spans
    that end on a window's last byte and one byte behind it, spans on the buffer's first and last
    byte at every address, and all of them in one call; each as a body of its own and inside a
    body that starts up to 40 bytes earlier, with entries of other kinds and garbage offsets on
    some lanes.  Each input has the property it was built for (by stage_cases.rounds, at the
    kernel's staging size); status, reply status and slots are the plain rules', and the
    emulator's rounds are the ones stage_cases.rounds gives at the stage in use, with no block read
    bytewise that lies wholly inside the buffer."""
    trace = str(args_emu[1] / "rounds.txt")
    monkeypatch.setenv("RPC_EMU_STAGE_TRACE", trace)

    def check_placed(emu, stage, mis, buf, entries, schema=ac.IDL, width=ac.MAX_PARAMS, what=""):
        want = check(emu, stage, mis, buf, entries, schema, width, what)
        spans = [(e[0] + e[4], e[5]) for e in entries]
        assert sc.read_trace(trace) == sc.trace(spans, sc.args_walked(buf, entries, schema), mis, len(buf), stage), what
        return want

    n_of = lambda want: [w[2][0] for w in want]  # noqa: E731
    for mis in (0, odd):
        for name in sc.BATCH:
            p, methods = sc.args_batch(name)
            strangers = sc.STRANGERS if len(p.spans) == len(sc.args_set()) else ()
            for lead in (False, True):
                entries = sc.args_entries(p.spans, methods, lead, strangers)
                p.holds(sc.args_walked(p.buf, entries), mis)
                want = check_placed(args_emu, stage, mis, p.buf, entries, what=(name, mis, lead))
                assert all(want[t][0] == ac.NONE for t in strangers)
                if name == "nested":
                    assert sorted(set(n_of(want))) == [0, 2000000031] and sum(w[0] == ac.DEFER for w in want) == len(want) - 2
        for p in sc.window_edges(sc.params, mis, stage):
            for lead in (False, True):
                entries = sc.args_entries(p.spans, [ac.N] * 3, lead)
                p.holds(sc.args_walked(p.buf, entries), mis)
                want = check_placed(args_emu, stage, mis, p.buf, entries, what=(p.name, mis, lead))
                assert n_of(want) == [2000000001, 2000000002, 2000000002]
        buf, spans, methods = sc.args_mixture(mis)
        entries = sc.args_entries(spans, methods, True, sc.STRANGERS)
        check_placed(args_emu, stage, mis, buf, entries, what=("mixture", mis))
        counts = [len(g) for g in sc.rounds(spans, sc.args_walked(buf, entries), mis)]
        assert counts[0] >= 128 and counts[1] == 1 and len(counts) >= 4
    for mis in range(16):
        p = sc.buffer_ends(sc.params, mis)
        for lead in (False, True):
            entries = sc.args_entries(p.spans, [ac.N] * 2, lead)
            p.holds(sc.args_walked(p.buf, entries), mis)
            want = check_placed(args_emu, stage, mis, p.buf, entries, what=(p.name, lead))
            assert n_of(want) == [2000000003, 2000000004]
        if mis in sc.WHOLE_MIS:
            p = sc.whole_buffer(sc.WHOLE, mis)
            entries = sc.args_entries(p.spans, [0])
            p.holds(sc.args_walked(p.buf, entries, sc.ID_SCHEMA), mis)
            want = check_placed(args_emu, stage, mis, p.buf, entries, sc.ID_SCHEMA, 1, p.name)
            assert want == [(ac.OK, 0, (7,))]
