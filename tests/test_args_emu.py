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
