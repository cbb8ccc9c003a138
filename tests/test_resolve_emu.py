"""CPU emulation of the frame resolve (tests/cpu_emu/resolve_emu.cpp) against the plain rules
(tests/resolve_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_resolve.h and the shared walk of frames_route.h -- the precheck, the strict
automaton with the reply's key policy, the table's hash, insert and probe -- and runs the
staging rounds, the walk over the staged bytes and the table, probe and finish passes as the
kernels run them, at the kernel's staging size and at a small one (so that bodies straddle the
edges of a round), with the body buffer at aligned and at odd addresses, visiting entries and
slots ascending and descending.  Its readers abort on any byte outside [0, bodies_bytes), outside
what a round staged, outside the table or outside the pending ids."""
import os
import re
import subprocess

import pytest

import resolve_cases as rc
import stage_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_route.h")
RESOLVE_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_resolve.h")


def kernel_constant(path, name):
    m = re.search(r"constexpr uint32_t %s = (0x[0-9A-Fa-f]+|\d+)u?;" % name, open(path).read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1), 0)


S_K = kernel_constant(ROUTE_H, "kRouteStage")
S_SMALL = 1088  # a multiple of 16 that just holds one body at any alignment: almost every round is cut
#: (staging bytes, low address bits of the body buffer)
SHAPES = [(S_K, 0), (S_K, 5), (S_SMALL, 0), (S_SMALL, 11), (S_SMALL, 15)]


@pytest.fixture(scope="module")
def resolve_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("resolve_emu")
    exe, src = str(d / "resolve_emu"), os.path.join(REPO, "tests", "cpu_emu", "resolve_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(resolve_emu, stage, mis, call, descending):
    exe, d = resolve_emu
    bp, ep, pp = (str(d / n) for n in ("bodies.bin", "entries.txt", "pending.txt"))
    open(bp, "wb").write(call.buf)
    tt = call.types if call.types is not None else [0] * len(call.offs)
    open(ep, "w").write("".join("%d %d %d\n" % e for e in zip(call.offs, call.lens, tt)))
    open(pp, "w").write("".join("%d\n" % i for i in call.pending))
    p = subprocess.run([exe, str(stage), str(mis), "0" if call.types is None else "1", "1" if descending else "0",
                        bp, ep, pp], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    n = len(call.offs)
    cols = list(zip(*[map(int, ln.split()) for ln in lines[:n]])) if n else [()] * 7
    return rc.Resolved(*[list(c) for c in cols], [int(x) for x in lines[n].split()[1:]],
                       [int(x) for x in lines[n + 1].split()[1:]])


def check(resolve_emu, stage, mis, call, what):
    """Both visiting orders give the rules' outputs, field for field."""
    want = call.expect()
    for descending in (False, True):
        got = run_emu(resolve_emu, stage, mis, call, descending)
        for field in rc.Resolved._fields:
            g, w = getattr(got, field), getattr(want, field)
            bad = [i for i, (a, b) in enumerate(zip(g, w)) if a != b]
            assert not bad and len(g) == len(w), (what, descending, field, bad[:5],
                                                  [(g[i], w[i]) for i in bad[:5]])
    return want


def test_the_hash_is_the_headers():
    assert kernel_constant(RESOLVE_H, "kResolveHashMul") == rc.HASH_MUL
    assert kernel_constant(RESOLVE_H, "kResolveNoSlot") == rc.NO_SLOT


def test_rules_on_the_stated_cases():
    """The plain rules give the cases the issue spells out the answers it spells out."""
    c = rc.CASES
    kind = lambda k: rc.decode_body(c[k])[0]  # noqa: E731
    assert kind("wrong_type_id_first") == rc.INVALID and rc.decode_body(c["good_id_first"])[:2] == (rc.UNKNOWN, 5)
    assert all(kind(k) == rc.INVALID for k in ("id_absent", "id_string", "id_null", "id_true", "id_array",
                                               "id_object", "empty_object", "nested_only"))
    assert all(kind(k) == rc.DEFER for k in ("id_over", "id_over_long", "id_edge_hi", "id_signed", "id_fraction",
                                             "id_exponent", "id_leading_zero", "key_backslash", "len_over",
                                             "depth_over", "tokens_over", "string_result_u", "zero_byte",
                                             "array_root", "scalar_root", "trailing_garbage", "truncated"))
    assert all(kind(k) == rc.UNKNOWN for k in ("len_max", "depth_ok", "tokens_ok", "string_result_high",
                                               "nested_key_backslash", "whitespace"))
    assert rc.decode_body(c["id_max"])[1] == 4294967295 and rc.decode_body(c["id_zero"])[:2] == (rc.UNKNOWN, 0)
    span = lambda k, j: c[k][rc.decode_body(c[k])[j]:][:rc.decode_body(c[k])[j + 1]]  # noqa: E731
    assert span("both", 2) == b"1" and span("both", 4) == b'{"code":1}'
    assert rc.decode_body(c["neither"])[2:] == (0, 0, 0, 0)
    assert span("null_result", 2) == b"null" and span("null_error", 4) == b"null"
    assert span("first_result_wins", 2) == b"1" and span("first_error_wins", 4) == b'"a"'
    assert span("nested_id_ignored", 2) == b'{"id":99,"error":1}' and rc.decode_body(c["nested_id_ignored"])[4:] == (0, 0)
    assert span("whitespace", 2) == b'[ 1 , { "a" : null } ]' and span("whitespace", 4) == b"false"
    assert span("number_results", 2) == b"-1.5e+10" and span("empty_string_result", 2) == b'""'
    for w in ("id", "result", "error"):
        for k in range(4):
            b = c["case_%s_%d" % (w, k)]
            assert rc.decode_body(b)[1] == 100 + k and span("case_%s_%d" % (w, k), 2) == b'{"a":[1]}'
            assert span("case_%s_%d" % (w, k), 4) == b'"e"'
    j = rc.join_calls()
    e = j["id_in_two_slots"].expect()
    assert e.slot == [3, 11, 3] and e.kind == [rc.MATCHED, rc.MATCHED, rc.DUPLICATE] and 9 in e.open
    e = j["three_replies"].expect()
    assert [e.kind[i] for i in (1, 255, 256)] == [rc.MATCHED, rc.DUPLICATE, rc.DUPLICATE] and not e.open
    e = j["types_and_ranges"].expect()
    assert e.kind == [rc.MATCHED, rc.NONE, rc.MATCHED, rc.RANGE, rc.RANGE, rc.RANGE, rc.MATCHED, rc.NONE]
    assert e.open == [2] and e.slot_entry == [6, 2, rc.NO_SLOT, 0]  # (pending 4, 3, 2, 1; the reply to 2 is a PING's)


@pytest.mark.parametrize("stage,mis", SHAPES)
def test_table_matches_plain_rules(resolve_emu, stage, mis):
    """The case table as one call (NUL behind each body and none), and the 1,024-byte bodies."""
    for nul in (1, 0):
        _, call = rc.case_call(nul=nul)
        want = check(resolve_emu, stage, mis, call, "table nul=%d" % nul)
        assert set(want.kind) == {rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE, rc.INVALID, rc.DEFER}
    want = check(resolve_emu, stage, mis, rc.big_bodies_call(), "40 bodies of 1,024 B")
    assert set(want.kind) == {rc.MATCHED} and not want.open


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 13)])
def test_join_shapes_match_plain_rules(resolve_emu, stage, mis):
    """Collisions in a run that wraps, an id in two slots, three replies to one id across two
    workgroups, strangers, npending 0 / 1 / 2 / 257, no entries, non-DATA entries and ranges."""
    for name, call in rc.join_calls().items():
        check(resolve_emu, stage, mis, call, name)


@pytest.mark.parametrize("stage,mis", [(S_K, 0), (S_SMALL, 7)])
def test_mutations_match_plain_rules(resolve_emu, stage, mis):
    """Canonical replies, and 20,000 replies with one byte flipped, inserted or deleted, or cut
    short: field for field, DEFER included.  No canonical reply defers; the mutations reach every
    kind a body can have."""
    canon = rc.canonical_set(0xC0FFEE, 900)
    muts = rc.mutation_set(0xBADC0DE, 20000)
    buf, offs, lens = rc.pack_bodies(canon + muts, nul=1)
    ids = [rc.decode_body(b)[1] for b in canon[::2]] + [1, 2, 3]
    want = check(resolve_emu, stage, mis, rc.Call(buf, offs, lens, None, ids), "mutations")
    assert all(k in (rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE) for k in want.kind[:len(canon)])
    assert set(want.kind[len(canon):]) == {rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE, rc.INVALID, rc.DEFER}
    decoded = sum(1 for k in want.kind[len(canon):] if k not in (rc.DEFER, rc.INVALID))
    assert 1000 < decoded < 19000  # both sides of the strict subset are exercised


def placed_call(p, pending):
    return rc.Call(p.buf, [s[0] for s in p.spans], [s[1] for s in p.spans], None, pending)


@pytest.mark.parametrize("stage,odd", [(S_K, 5), (S_SMALL, 11)])
def test_placements_match_plain_rules(resolve_emu, stage, odd, monkeypatch):
    """Bodies anywhere (tests/stage_cases.py): memory order reversed and shuffled, fixed slots, all
    lanes on one span and on two far apart, every prefix and suffix of one text, bodies that end
    on a window's last byte and one byte behind it, bodies on the buffer's first and last byte at
    every address, and all of them in one call.  Each input has the property it was built for
    (by stage_cases.rounds, at the kernel's staging size); the whole Resolved tuple, the join
    included, is the plain rules', and the emulator's rounds are the ones stage_cases.rounds gives
    at the stage in use, with no block read bytewise that lies wholly inside the buffer."""
    bodies, pending = sc.resolve_set()
    trace = str(resolve_emu[1] / "rounds.txt")
    monkeypatch.setenv("RPC_EMU_STAGE_TRACE", trace)

    def check_placed(emu, stage, mis, call, what):
        want = check(emu, stage, mis, call, what)
        spans = list(zip(call.offs, call.lens))
        assert sc.read_trace(trace) == sc.trace(spans, sc.walked(call.buf, spans), mis, len(call.buf), stage), what
        return want

    edge_ids = [4000000001 + k for k in (3, 1, 30, 2, 21, 10, 0, 12)]  # (not 11 and 20: nobody waits for them)
    for mis in (0, odd):
        for name in sc.BATCH:
            p = sc.batch(name, bodies, sc.reply)
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(resolve_emu, stage, mis, placed_call(p, pending + edge_ids), (name, mis))
            if name == "one body":  # the first lane of a workgroup takes the slot, the others find it taken
                taken = [rc.MATCHED] + [rc.DUPLICATE] * 255
                assert want.kind == taken + [rc.UNKNOWN] * 256 + taken
            if name == "two bodies":
                assert want.kind == [rc.UNKNOWN, rc.MATCHED] + [rc.UNKNOWN, rc.DUPLICATE] * 127
            if name == "nested":
                assert sorted(set(want.id)) == [0, 4000000031] and want.kind.count(rc.DEFER) == len(p.spans) - 2
        for p in sc.window_edges(sc.reply, mis, stage):
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(resolve_emu, stage, mis, placed_call(p, edge_ids), (p.name, mis))
            assert want.id == [4000000001, 4000000002, 4000000002]
            assert want.kind == [rc.MATCHED, rc.MATCHED, rc.DUPLICATE]
        buf, spans, placed = sc.mixture(bodies, sc.reply, mis)
        call = rc.Call(buf, [s[0] for s in spans], [s[1] for s in spans], None, pending + edge_ids)
        want = check_placed(resolve_emu, stage, mis, call, ("mixture", mis))
        assert list(zip(want.id, want.result_off, want.result_len, want.error_off, want.error_len)) == \
            [rc.decode_body(b)[1:] for b in placed]
        counts = [len(g) for g in sc.rounds(spans, sc.walked(buf, spans), mis)]
        assert counts[0] >= 128 and counts[1] == 1 and len(counts) >= 4
    for mis in range(16):
        ends = [sc.buffer_ends(sc.reply, mis)] + [sc.whole_buffer(sc.WHOLE, mis)] * (mis in sc.WHOLE_MIS)
        for p in ends:
            p.holds(sc.walked(p.buf, p.spans), mis)
            want = check_placed(resolve_emu, stage, mis, placed_call(p, edge_ids + [7]), p.name)
            assert want.id in ([4000000003, 4000000004], [7]) and set(want.kind) == {rc.MATCHED}
