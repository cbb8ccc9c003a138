"""CPU emulation of the frame unpack (tests/cpu_emu/unpack_emu.cpp) against the plain rules
(tests/unpack_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_unpack.h with the frames_pack.h helpers it reuses -- the sizing rule,
the entry searches, the piece resolver with its funnel shift and masks -- and runs size,
scan, per-tile search, per-piece resolve and store as the kernels run them, at the kernels'
kPackTile and at a 256-byte tile, with the stream and the output at aligned and at odd
addresses.  Its stream reader aborts on any byte outside [0, stream_bytes); its writer
aborts on any byte outside an entry that is to be written, stored twice, or left out."""
import os
import re
import subprocess

import pytest

import unpack_cases as uc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_pack.h")
FLAGS = {"server": 1, "client": 2}
LIFT = 4


def kernel_constant(name):
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(PACK_H).read())
    assert m, f"{name} not found in {PACK_H}"
    return int(m.group(1))


T_K = kernel_constant("kPackTile")
#: (tile, low address bits of the stream, low address bits of the output)
SHAPES = [(T_K, 0, 0), (T_K, 5, 9), (256, 0, 0), (256, 11, 3), (256, 0, 15)]
VARIANTS = [("server", 1), ("server", 0), ("client", 1), ("client", 0)]


@pytest.fixture(scope="module")
def unpack_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("unpack_emu")
    exe, src = str(d / "unpack_emu"), os.path.join(REPO, "tests", "cpu_emu", "unpack_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(unpack_emu, T, src_mis, out_mis, case, out_cap):
    exe, d = unpack_emu
    bp, ep, cp, op = (str(d / n) for n in ("stream.bin", "entries.txt", "conn.txt", "out.bin"))
    open(bp, "wb").write(case.stream)
    open(ep, "w").write("".join("%d %d\n" % e for e in case.entries))
    if case.conn_first is not None:
        open(cp, "w").write("".join("%d\n" % k for k in case.conn_first))
    p = subprocess.run([exe, str(T), str(FLAGS[case.role] | (LIFT if case.lift_cap else 0)), str(case.nul),
                        str(-1 if out_cap is None else out_cap), str(src_mis), str(out_mis), bp, ep,
                        cp if case.conn_first is not None else "-", op], capture_output=True, text=True)
    assert p.returncode == 0, (case.name, case.role, case.nul, out_cap, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    total = int(lines[0].split()[1])
    rows = [tuple(map(int, ln.split())) for ln in lines[1:1 + len(case.entries)]]
    conn = [int(x) for x in lines[1 + len(case.entries)].split()[1:]]
    return total, rows, conn, open(op, "rb").read()


def check(unpack_emu, T, src_mis, out_mis, case):
    for cap in case.out_caps:
        want = uc.want_of(case, cap)
        total, rows, conn, out = run_emu(unpack_emu, T, src_mis, out_mis, case, cap)
        what = (case.name, case.role, case.nul, T, src_mis, out_mis, cap)
        assert total == want.total, what
        assert [r[0] for r in rows] == want.body_offsets, what
        assert [r[1] for r in rows] == want.body_lens, what
        assert [r[2] for r in rows] == want.reply_types, what
        assert [r[3] for r in rows] == want.versions, what
        assert [r[4] for r in rows] == want.verdict, what
        assert conn == want.conn_bytes_first, what
        assert out == want.out, what
    return want


def table_categories(case, want, T, out_mis):
    """The categories of the table, asserted on the plain rules' own output."""
    role, nul = case.role, case.nul
    v = want.verdict
    assert set(uc.NOT_DELIVERED) | {uc.OK, uc.CONTROL} <= set(v)
    assert want.total < (1 << 20) and len(case.stream) < (1 << 20)
    lens = [ln for ln in uc.TABLE_LENS if ln or role == "server"]  # (an empty body is never delivered to a client)
    pairs = {((o + uc.HDR) % 16, (at + out_mis) % 16, ln)
             for (o, vi), at, ln, vo in zip(case.entries, want.body_offsets, want.body_lens, v) if vo == uc.OK}
    assert {(s, d, ln) for s in range(16) for d in range(16) for ln in lens} <= pairs
    ends = {(at + len(c) + out_mis) % T for at, c in zip(want.body_offsets, want.chunks) if c}
    starts = {(at + out_mis) % T for at, c in zip(want.body_offsets, want.chunks) if c}
    assert 0 in ends and 0 in starts and (not nul or 1 in ends)
    assert sum(1 for x in v if x == uc.CONTROL) >= 40
    ones = sum(1 for c in want.chunks if len(c) == 1)
    assert ones >= uc.EMPTY_RUN if (role == "server" and nul) else True
    assert case.conn_first[:2] == [0, 0] and case.conn_first[-1] == case.conn_first[-2]
    assert case.entries[-1] == (len(case.stream), uc.MALFORMED)
    types = set(want.reply_types)
    assert types == ({uc.DATA, uc.PONG, uc.NONE} if role == "server" else {uc.DATA, uc.NONE})


@pytest.mark.parametrize("role,nul", VARIANTS)
@pytest.mark.parametrize("T,src_mis,out_mis", SHAPES)
def test_table_matches_plain_rules(unpack_emu, T, src_mis, out_mis, role, nul):
    """Every alignment pair at six lengths, an entry ending on a tile edge and one starting on
    it, 40 heartbeats, 2000 empty bodies (1-byte entries, 16 per piece), every verdict that
    delivers nothing, padding entries, empty connections at both ends of the CSR: byte for
    byte and word for word."""
    case = uc.table_case(T, out_mis, role, nul)
    want = check(unpack_emu, T, src_mis, out_mis, case)
    table_categories(case, want, T, out_mis)


@pytest.mark.parametrize("role,nul", VARIANTS)
@pytest.mark.parametrize("T,src_mis,out_mis", SHAPES)
def test_capacity_lies_and_lifted_cap(unpack_emu, T, src_mis, out_mis, role, nul):
    """out_cap at the total, one byte less, inside a body, on a NUL and 0; n = 1 of each kind;
    verdicts the stream contradicts; RPC_FRAMES_LIFT_CAP with one body of 3 tiles + 5 bytes."""
    for case in uc.small_cases(T, out_mis, role, nul):
        check(unpack_emu, T, src_mis, out_mis, case)
    for case in uc.lying_cases(role, nul):
        want = check(unpack_emu, T, src_mis, out_mis, case)
        assert want.verdict[1] == uc.MALFORMED and want.reply_types[1] == uc.NONE and not want.chunks[1], case.name
        assert want.verdict[0] == want.verdict[2] == uc.OK
    cap = next(c for c in uc.small_cases(T, out_mis, role, nul) if c.name == "capacity")
    full, less = uc.want_of(cap, None), uc.want_of(cap, uc.want_of(cap, None).total - 1)
    last = max(i for i, c in enumerate(full.chunks) if c)
    assert [i for i in range(len(cap.entries)) if less.verdict[i] != full.verdict[i]] == [last]
    assert less.reply_types[last] == uc.NONE and full.reply_types[last] == uc.DATA
    assert less.body_offsets == full.body_offsets and less.total == full.total  # the layout never depends on out_cap
    assert less.body_lens == full.body_lens and less.versions == full.versions
