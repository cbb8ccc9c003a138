"""CPU emulation of the frame carry (tests/cpu_emu/carry_emu.cpp) against the plain rules
(tests/carry_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_carry.h with the frames_pack.h helpers it reuses -- the rule, the pieces
aligned to the destination's address, the funnel shift and the byte masks, the chunk counts
and the chunk -> connection searches -- and runs both routes as the kernels run them, the long
one at the kernel's kCarryChunk and at a 256-byte chunk, with the stream and the next buffer
at aligned and at odd addresses.  Its stream reader aborts on any byte outside
[0, stream_bytes); its writer aborts on any byte outside a tail that is to be written, stored
twice, or left out."""
import os
import re
import subprocess

import pytest

import carry_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARRY_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_carry.h")


def kernel_constant(name):
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(CARRY_H).read())
    assert m, f"{name} not found in {CARRY_H}"
    return int(m.group(1))


C_K = kernel_constant("kCarryChunk")
SHORT_ROOM = kernel_constant("kCarryShortRoom")
#: (chunk, lanes per connection or 0 for the long route, low address bits of the stream, of the next buffer)
ROUTES = [(C_K, 16, 0, 0), (C_K, 64, 5, 9), (C_K, 16, 11, 3), (256, 0, 0, 0), (256, 0, 7, 250), (C_K, 0, 3, 16381)]


@pytest.fixture(scope="module")
def carry_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("carry_emu")
    exe, src = str(d / "carry_emu"), os.path.join(REPO, "tests", "cpu_emu", "carry_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(carry_emu, chunk, group, src_mis, next_mis, case):
    exe, d = carry_emu
    bp, cp, op = (str(d / n) for n in ("stream.bin", "conn.txt", "out.bin"))
    open(bp, "wb").write(case.stream)
    nl = case.new_len if case.new_len is not None else [0] * len(case.conns)
    open(cp, "w").write("".join("%d %d %d %d %d %d\n" % (*c, at, n) for c, at, n in zip(case.conns, case.next_at, nl)))
    p = subprocess.run([exe, str(chunk), str(group), str(case.room), str(int(case.use_state)), str(src_mis),
                        str(next_mis), str(case.next_bytes), bp, cp, op], capture_output=True, text=True)
    assert p.returncode == 0, (case.name, chunk, group, src_mis, next_mis, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    rows = [tuple(map(int, ln.split())) for ln in lines[:len(case.conns)]]
    return rows, int(lines[len(case.conns)].split()[1]), open(op, "rb").read()


def check(carry_emu, chunk, group, src_mis, next_mis, case):
    want = cc.want_of(case)
    rows, carried, out = run_emu(carry_emu, chunk, group, src_mis, next_mis, case)
    what = (case.name, chunk, group, src_mis, next_mis)
    assert [r[0] for r in rows] == want.next_off, what
    assert [r[1] for r in rows] == want.next_len, what
    assert [r[2] for r in rows] == want.status, what
    assert carried == want.carried, what
    assert out == want.next, what
    return want


@pytest.mark.parametrize("chunk,group,src_mis,next_mis", ROUTES)
def test_table_matches_plain_rules(carry_emu, chunk, group, src_mis, next_mis):
    """Every (source mod 16, destination mod 16) pair at tails of 0 .. 1035 bytes, on both
    routes: byte for byte and word for word."""
    case = cc.table_case()
    want = check(carry_emu, chunk, group, src_mis, next_mis, case)
    assert set(want.status) == {cc.OK} and len(case.conns) == 16 * 16 * len(cc.TABLE_TAILS)
    pairs = {((off + used) % 16, no % 16, ln - used) for (off, ln, used, _), no in zip(case.conns, want.next_off)}
    assert pairs == {(s, d, t) for s in range(16) for d in range(16) for t in cc.TABLE_TAILS}
    assert want.carried == 256 * sum(cc.TABLE_TAILS)


@pytest.mark.parametrize("use_state", [True, False])
@pytest.mark.parametrize("chunk,group,src_mis,next_mis", ROUTES)
def test_contract_corners(carry_emu, chunk, group, src_mis, next_mis, use_state):
    """The stream's and the next buffer's edges, tail == room and one more, connections that
    wrap 2^64, consumed == len + 1, closed connections with garbage words (which the guarded
    reader would catch), and the same without a state array."""
    case, names = cc.corner_case()
    case = case._replace(use_state=use_state)
    want = check(carry_emu, chunk, group, src_mis, next_mis, case)
    st = dict(zip(names, zip(want.status, want.next_off, want.next_len)))
    n = len(case.stream)
    assert st["dst_starts_at_0"] == (cc.OK, 0, 37 + 5)
    assert st["tail_gt_at"] == (cc.NO_ROOM, 0, 0)
    assert st["src_starts_at_0"][0] == cc.OK and case.conns[names.index("src_starts_at_0")][0] == 0
    end = case.conns[names.index("src_ends_at_end")]
    assert st["src_ends_at_end"][0] == cc.OK and end[0] + end[1] == n
    assert st["tail_eq_room"][0] == cc.OK and st["tail_eq_room"][2] == case.room + 2
    assert st["tail_eq_room_plus_1"] == (cc.NO_ROOM, 0, 0)
    assert st["empty_at_stream_end"][0] == cc.OK and st["empty_at_stream_end"][2] == 4
    for k in ("off_past_end", "len_past_end", "off_len_wrap", "len_wrap", "consumed_gt_len"):
        assert st[k] == (cc.INVALID, 0, 0), k
    assert st["consumed_eq_len"][0] == cc.OK and st["consumed_eq_len"][2] == 3
    assert st["closed_garbage"] == ((cc.CLOSED if use_state else cc.INVALID), 0, 0)
    assert st["closed_plain"][0] == st["state_other"][0] == (cc.CLOSED if use_state else cc.OK)
    for k in ("at_past_next", "new_len_wrap", "ends_past_next_end"):
        assert st[k] == (cc.NO_ROOM, 0, 0), k
    last = names.index("ends_at_next_end")
    assert st["ends_at_next_end"][0] == cc.OK and case.next_at[last] + case.new_len[last] == case.next_bytes


@pytest.mark.parametrize("src_mis,next_mis", [(0, 0), (9, 255), (15, 1)])
def test_long_route_small_chunk(carry_emu, src_mis, next_mis):
    """Tails of chunk - 1, chunk, chunk + 1 and 3 chunks + 5 bytes (and 0, 1, 17) at a 256-byte
    chunk, ending anywhere in a chunk; every tail 0; no new lengths."""
    case = cc.long_case(256, cc.long_tails(256), cc.ROOM)
    want = check(carry_emu, 256, 0, src_mis, next_mis, case)
    assert set(want.status) == {cc.OK} and want.carried == sum(cc.long_tails(256))
    zero = cc.long_case(256, [0] * 9, cc.ROOM)
    assert check(carry_emu, 256, 0, src_mis, next_mis, zero).carried == 0
    check(carry_emu, 256, 0, src_mis, next_mis, case._replace(new_len=None))


@pytest.mark.parametrize("src_mis,next_mis", [(0, 0), (13, 16379)])
def test_long_route_kernel_chunk(carry_emu, src_mis, next_mis):
    """One tail of two chunks + 5 bytes at the kernel's chunk, beside short ones; a room below
    it refuses that tail alone."""
    tails = [40, 2 * C_K + 5, 0, 700]
    case = cc.long_case(C_K, tails, 2 * C_K + 5)
    want = check(carry_emu, C_K, 0, src_mis, next_mis, case)
    assert set(want.status) == {cc.OK} and want.carried == sum(tails)
    less = check(carry_emu, C_K, 0, src_mis, next_mis, case._replace(room=2 * C_K + 4))
    assert less.status == [cc.OK, cc.NO_ROOM, cc.OK, cc.OK] and less.carried == 740


def test_thresholds_in_the_header():
    """The short route covers the default room; the table's longest tail is what the scan's
    stop rule allows with the cap in force."""
    assert SHORT_ROOM >= cc.ROOM >= 12 + 1024 - 1 == max(cc.TABLE_TAILS) and cc.ROOM % 16 == 0
