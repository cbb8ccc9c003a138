"""CPU emulation of the frame results (tests/cpu_emu/results_emu.cpp) against the plain rules
(tests/results_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_results.h -- the precheck, the walk over the two member spans with the args'
automaton and conversions, the per-slot test -- and runs the staging rounds over the bodies, the
walk over the staged bytes, the slot stores and the count as the kernels run them, at the
kernel's staging size and at a small one (so that bodies straddle the edges of a round), with
the body buffer at aligned and at odd addresses.  Its readers abort on any byte outside
[0, bodies_bytes), outside what a round staged, or outside the schema's arrays, and it aborts
when a slot is written by no lane or by two."""
import os
import subprocess

import pytest

import resolve_cases as rv
import results_cases as rs
import stage_cases as sc
from test_route_emu import S_K, S_SMALL, SHAPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("results_emu")
    exe, src = str(d / "results_emu"), os.path.join(REPO, "tests", "cpu_emu", "results_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(results_emu, stage, mis, buf, entries, pm, se, types=rs.TYPES):
    """(rows, slots, ndefer) of one emulator run."""
    exe, d = results_emu
    bp, ep, sp = (str(d / n) for n in ("bodies.bin", "entries.txt", "schema.txt"))
    open(bp, "wb").write(buf)
    open(ep, "w").write("".join("%d %d %d %d %d %d %d %d\n" % e for e in entries))
    words = lambda tag, ws: tag + "".join(" %d" % w for w in ws) + "\n"  # noqa: E731
    open(sp, "w").write(words("pending", pm) + words("types", types) + words("slot_entry", se))
    p = subprocess.run([exe, "run", str(stage), str(mis), bp, ep, sp], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [tuple(int(x) for x in ln.split()) for ln in p.stdout.splitlines()]
    n = len(entries)
    assert len(lines) == n + len(pm) + 1
    return [rs.Row(*r) for r in lines[:n]], lines[n:n + len(pm)], lines[-1][0]


def check(results_emu, stage, mis, buf, entries, pm, se, types=rs.TYPES, what=""):
    rows, slots, nd = run_emu(results_emu, stage, mis, buf, entries, pm, se, types)
    want = rs.results_entries(buf, entries, pm, types)
    for k, (g, w) in enumerate(zip(rows, want)):
        assert g == w, (what, k, entries[k], g, w)
    assert slots == rs.results_slots(entries, want, se), what
    assert nd == rs.ndefer(want), what
    return want



@pytest.mark.parametrize("stage,mis", SHAPES)
def test_table_matches_plain_rules(results_emu, stage, mis):
    """The case table as one buffer with every other status behind it, the per-slot cases, and
    the empty call."""
    check(results_emu, stage, mis, *rs.case_entries(pad_front=3), what="table")
    check(results_emu, stage, mis, *rs.slot_cases(), what="slots")
    check(results_emu, stage, mis, b"", [], [rs.I32] * 3, [rv.NO_SLOT, 0, 5], what="no entries")
    check(results_emu, stage, mis, b"", [], [], [], types=[], what="nothing at all")


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 7)])
def test_mutations_match_plain_rules(results_emu, stage, mis):
    """20,000 canonical members with one byte flipped, inserted or deleted, or truncated, and the
    canonical replies themselves: field for field, DEFER included.  The mutations reach every
    status of the walk."""
    canon = rs.canonical_set(0xE5017, 1500)
    muts = rs.mutation_set(0xBADE501, 20000)
    buf, entries, pm, se = rs.back_to_back(canon + muts)
    want = check(results_emu, stage, mis, buf, entries, pm, se, what="mutations")
    n = {s: sum(1 for w in want[len(canon):] if s in (w.status, w.error_status)) for s in (rs.OK, rs.MISMATCH, rs.DEFER)}
    assert min(n.values()) >= 500, n  # (the generator's reach, computed by the rules alone)


@pytest.mark.parametrize("stage,odd", [(S_K, 5), (S_SMALL, 11)])
def test_placements_match_plain_rules(results_emu, stage, odd, monkeypatch):
    """Bodies anywhere (tests/stage_cases.py): memory order reversed and shuffled, fixed slots, all
    lanes on one body and on two far apart, every prefix and suffix of one text, bodies that end
    on a window's last byte and one byte behind it, bodies on the buffer's first and last byte at
    every address, and all of them in one call.  Each input has the property it was built for
    (by stage_cases.rounds, at the kernel's staging size); every answer is the plain rules', and
    the emulator's rounds are the ones stage_cases.rounds gives at the stage in use, with no
    block read bytewise that lies wholly inside the buffer."""
    bodies, _ = sc.resolve_set()
    trace = str(results_emu[1] / "rounds.txt")
    monkeypatch.setenv("RPC_EMU_STAGE_TRACE", trace)

    def check_placed(buf, spans, mis, what):
        entries, pm, se = rs.placed_entries(buf, spans)
        want = check(results_emu, stage, mis, buf, entries, pm, se, what=what)
        assert sc.read_trace(trace) == sc.trace(spans, sc.walked(buf, spans), mis, len(buf), stage), what
        return want

    for mis in (0, odd):
        for name in sc.BATCH:
            p = sc.batch(name, bodies, sc.reply)
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(p.buf, p.spans, mis, (name, mis))
            assert {rs.OK, rs.DEFER} <= {w.status for w in want}, name
        for p in sc.window_edges(sc.reply, mis, stage):
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(p.buf, p.spans, mis, (p.name, mis))
            assert all(w.status in (rs.OK, rs.MISMATCH, rs.DEFER) for w in want), p.name  # (each was walked)
        buf, spans, placed = sc.mixture(bodies, sc.reply, mis)
        check_placed(buf, spans, mis, ("mixture", mis))
        counts = [len(g) for g in sc.rounds(spans, sc.walked(buf, spans), mis)]
        assert counts[0] >= 128 and counts[1] == 1 and len(counts) >= 4
    for mis in range(16):
        ends = [sc.buffer_ends(sc.reply, mis)] + [sc.whole_buffer(sc.WHOLE, mis)] * (mis in sc.WHOLE_MIS)
        for p in ends:
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(p.buf, p.spans, mis, p.name)
            assert all(w.status in (rs.OK, rs.MISMATCH) for w in want), p.name
