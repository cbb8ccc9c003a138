"""CPU emulation of the frame pack (tests/cpu_emu/pack_emu.cpp) against the plain rules
(tests/pack_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_pack.h -- the sizing rule, the entry searches, the piece resolver
with its funnel shift and masks -- and runs size, scan, per-tile search, per-piece
resolve and store as the kernels run them, at the kernels' kPackTile and at a 256-byte
tile, with the source buffer and the output at aligned and at odd addresses.  Its
source reader aborts on any byte outside [0, bodies_bytes); its writer aborts on any
byte outside a frame that is to be written, stored twice, or left out."""
import os
import re
import subprocess

import pytest

import pack_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_pack.h")
LIFT = 4


def kernel_constant(name):
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(PACK_H).read())
    assert m, f"{name} not found in {PACK_H}"
    return int(m.group(1))


T_K = kernel_constant("kPackTile")
#: (tile, low address bits of the source buffer, low address bits of the output)
SHAPES = [(T_K, 0, 0), (T_K, 5, 9), (256, 0, 0), (256, 11, 3), (256, 0, 15)]


@pytest.fixture(scope="module")
def pack_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("pack_emu")
    exe, src = str(d / "pack_emu"), os.path.join(REPO, "tests", "cpu_emu", "pack_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(pack_emu, T, src_mis, out_mis, case, out_cap):
    exe, d = pack_emu
    bp, ep, cp, op = (str(d / n) for n in ("bodies.bin", "entries.txt", "conn.txt", "out.bin"))
    open(bp, "wb").write(case.bodies)
    open(ep, "w").write("".join("%d %d %d %d\n" % e for e in case.entries))
    if case.conn_first is not None:
        open(cp, "w").write("".join("%d\n" % k for k in case.conn_first))
    p = subprocess.run([exe, str(T), str(LIFT if case.lift_cap else 0), str(-1 if out_cap is None else out_cap),
                        str(src_mis), str(out_mis), bp, ep, cp if case.conn_first is not None else "-", op],
                       capture_output=True, text=True)
    assert p.returncode == 0, (case.name, out_cap, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    total = int(lines[0].split()[1])
    rows = [tuple(map(int, ln.split())) for ln in lines[1:1 + len(case.entries)]]
    conn = [int(x) for x in lines[1 + len(case.entries)].split()[1:]]
    return total, rows, conn, open(op, "rb").read()


def check(pack_emu, T, src_mis, out_mis, case):
    for cap in case.out_caps:
        want = pc.expected(case.bodies, case.entries, case.conn_first, case.lift_cap, cap)
        total, rows, conn, out = run_emu(pack_emu, T, src_mis, out_mis, case, cap)
        what = (case.name, T, src_mis, out_mis, cap)
        assert total == want.total, what
        assert [r[0] for r in rows] == want.offsets, what
        assert [r[1] for r in rows] == want.verdict, what
        assert [r[2] for r in rows] == want.crc, what
        assert conn == want.conn_bytes_first, what
        assert out == want.out, what
    return want


@pytest.mark.parametrize("T,src_mis,out_mis", SHAPES)
def test_table_matches_plain_rules(pack_emu, T, src_mis, out_mis):
    """Every alignment pair at six lengths, headers split at every inner position across a
    tile edge, a body ending on one, a piece over three frames, runs of heartbeats and of
    entries that emit nothing, bodies at both ends of the source and one past it, empty
    connections at both ends of the CSR: byte for byte."""
    case = pc.table_case(T, out_mis)
    want = check(pack_emu, T, src_mis, out_mis, case)
    # the categories, asserted on the plain rules' own output
    v = want.verdict
    assert {pc.OK, pc.CONTROL, pc.TOO_LARGE, pc.MALFORMED, pc.SKIPPED} <= set(v)
    assert v[0] == pc.SKIPPED and v[-1] == pc.SKIPPED and want.total < (1 << 20)
    starts = {(o + out_mis) % T for o, f in zip(want.offsets, want.frames) if len(f) > pc.HDR}
    assert {T - k for k in range(1, pc.HDR)} <= starts
    assert any((o + len(f) + out_mis) % T == 0 for o, f in zip(want.offsets, want.frames) if f)
    pairs = {(e[2] % 16, (o + pc.HDR + out_mis) % 16, e[3]) for e, o, f in zip(case.entries, want.offsets, want.frames)
             if f and e[0] == pc.DATA and e[2] >= 6000}
    assert {(s, d, ln) for s in range(16) for d in range(16) for ln in (0, 1, 15, 16, 17, 1024)} <= pairs
    three = [i for i in range(1, len(v) - 1) if v[i] == pc.CONTROL and (want.offsets[i] + out_mis) % 16 == 1
             and want.frames[i - 1] and want.frames[i + 1]]
    assert three
    assert case.conn_first[:2] == [0, 0] and case.conn_first[-1] == case.conn_first[-2] == len(case.entries)


@pytest.mark.parametrize("T,src_mis,out_mis", SHAPES)
def test_capacity_single_entries_and_lifted_cap(pack_emu, T, src_mis, out_mis):
    """out_cap at the total, one byte less, inside a header, inside a body and 0; n = 1
    of each kind; RPC_FRAMES_LIFT_CAP with one body of 3 tiles + 5 bytes."""
    for case in pc.small_cases(T, out_mis):
        check(pack_emu, T, src_mis, out_mis, case)
    cap = next(c for c in pc.small_cases(T, out_mis) if c.name == "capacity")
    full = pc.expected(cap.bodies, cap.entries, cap.conn_first)
    less = pc.expected(cap.bodies, cap.entries, cap.conn_first, out_cap=full.total - 1)
    last = max(i for i, f in enumerate(full.frames) if f)
    assert [i for i in range(len(cap.entries)) if less.verdict[i] != full.verdict[i]] == [last]
    assert less.offsets == full.offsets and less.total == full.total  # the layout never depends on out_cap
