"""CPU emulation of the frame scan (tests/cpu_emu/scan_emu.cpp) against the plain walk
(tests/scan_cases.py).  The emulator compiles the kernels' own source,
rpc_amd/csrc/frames_scan.h -- the one-header step, the tile maps, compose and
resolve -- and runs tile pass, up-sweep, down-sweep, count and emit stage by stage,
at the kernels' T and G and at two small instantiations (T = 2048, G = 4, where a
~1 MiB connection needs five levels; T = 1036 = E, G = 2, the smallest legal tile).
Its tile reader aborts on a byte outside the tile and its 7-byte halo."""
import os
import re
import subprocess

import numpy as np
import pytest

import scan_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_H = os.path.join(REPO, "rpc_amd", "csrc", "frames_scan.h")
SERVER, CLIENT, LIFT = 1, 2, 4


def kernel_constant(name):
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, open(SCAN_H).read())
    assert m, f"{name} not found in {SCAN_H}"
    return int(m.group(1))


T_K, G_K = kernel_constant("kScanTile"), kernel_constant("kScanGroup")
SHAPES = [(T_K, G_K), (2048, 4), (sc.E, 2)]


@pytest.fixture(scope="module")
def scan_emu(tmp_path_factory):
    """The emulator, with AddressSanitizer and UBSan where this g++ links them."""
    d = tmp_path_factory.mktemp("scan_emu")
    exe, src = str(d / "scan_emu"), os.path.join(REPO, "tests", "cpu_emu", "scan_emu.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or b"usage" not in subprocess.run([exe], capture_output=True).stderr:  # (does it start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe, d


def run_emu(scan_emu, T, G, flags, tiled_min, tile_cap, blob, offs, lens):
    exe, d = scan_emu
    sp, cp = str(d / "stream.bin"), str(d / "conns.txt")
    open(sp, "wb").write(blob)
    open(cp, "w").write("".join(f"{o} {n}\n" for o, n in zip(offs.tolist(), lens.tolist())))
    p = subprocess.run([exe, str(T), str(G), str(flags), str(tiled_min), str(tile_cap), sp, cp], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    head = dict(zip(lines[0].split()[::2], map(int, lines[0].split()[1::2])))
    fo, first, consumed, state = [], [0], [], []
    for ln in lines[1:]:
        v = ln.split()
        state.append(int(v[0]))
        consumed.append(int(v[1]))
        assert int(v[2]) == len(v) - 3
        fo += [int(x) for x in v[3:]]
        first.append(len(fo))
    return head, fo, first, consumed, state


def check(scan_emu, T, G, role, lift, tiled_min, tile_cap, blob, offs, lens):
    flags = (SERVER if role == "server" else CLIENT) | (LIFT if lift else 0)
    head, fo, first, consumed, state = run_emu(scan_emu, T, G, flags, tiled_min, tile_cap, blob, offs, lens)
    wfo, _, wfirst, wconsumed, wstate, cats = sc.expected(blob, offs, lens, role, lift, tile=T)
    assert first == wfirst
    assert fo == wfo
    assert consumed == wconsumed
    assert state == wstate
    return head, cats


def edge_conns(rng, T, role):
    conns = [sc.crafted_conn(rng, T, role, ending) for ending in ("clean", "in_header", "in_body", "close")]
    conns += [b"", sc.frame(b"x" * 30)[:11], sc.frame(b""), sc.filler(rng, T, role), sc.filler(rng, T + 12, role),
              sc.filler(rng, 2 * T, role), sc.filler(rng, 2 * T, role) + b"\x00" * 11]
    conns += [sc.random_conn(rng, int(rng.integers(0, 4 * T)), role) for _ in range(24)]
    return conns


@pytest.mark.parametrize("role", ["server", "client"])
@pytest.mark.parametrize("T,G", SHAPES)
def test_tiled_scan_matches_plain_walk(scan_emu, T, G, role):
    """Every tile-edge case on the true chain, decoys off it, every ending; with a
    connection outside the stream.  Each category is asserted on the plain walk's
    own output."""
    rng = np.random.default_rng(T * 7 + G + (role == "client"))
    blob, offs, lens = sc.layout(rng, edge_conns(rng, T, role))
    offs = np.concatenate([offs, np.array([len(blob) - 5, 2**63], dtype=np.uint64)])
    lens = np.concatenate([lens, np.array([100, 1], dtype=np.uint64)])
    cap = len(blob) // T + len(offs) + 1
    head, cats = check(scan_emu, T, G, role, False, T, cap, blob, offs, lens)
    assert head["tiles"] > 0
    for far in range(1, 12):
        assert cats.get("split_far_%d" % far), far
    for k in ("exit_0", "exit_1035", "control_straddles", "close_last_in_tile", "end_in_header", "end_in_body",
              "end_clean", "decoys", "control", "close_too_large"):
        assert cats.get(k), (k, cats)
    if role == "client":
        assert cats.get("close_empty"), cats
    # the same stream with too little workspace for all of them (the rest walks
    # serially), with none at all, and with only the longest connections tiled
    for tiled_min, some in ((T, 40), (T, 0), (3 * T, cap)):
        check(scan_emu, T, G, role, False, tiled_min, some, blob, offs, lens)


def test_small_instantiation_needs_many_levels(scan_emu):
    """T = 2048, G = 4: a ~1 MiB connection (513 tiles) takes five levels; beside it
    connections of exactly G^k tiles +- 1, whose groups end on connection edges."""
    rng = np.random.default_rng(99)
    T, G = 2048, 4
    conns = [sc.filler(rng, (1 << 20) + 100, "server") + sc.frame(b"abc")[:9]]
    conns += [sc.filler(rng, T * n + d, "server") for n in (3, 4, 16) for d in (0, 12, -13)]
    blob, offs, lens = sc.layout(rng, conns)
    head, cats = check(scan_emu, T, G, "server", False, T, len(blob) // T + len(conns) + 1, blob, offs, lens)
    assert head["levels"] >= 4 and head["tiles"] >= 513, head
    assert cats.get("decoys") and cats.get("end_in_header")


@pytest.mark.parametrize("role", ["server", "client"])
def test_lifted_cap_walks_serially(scan_emu, role):
    """RPC_FRAMES_LIFT_CAP: bodies over the cap are walked through, nothing is tiled."""
    rng = np.random.default_rng(5 + (role == "client"))
    conns = [sc.random_conn(rng, int(rng.integers(0, 20000)), role, lift_cap=True) for _ in range(40)]
    blob, offs, lens = sc.layout(rng, conns)
    head, cats = check(scan_emu, 2048, 4, role, True, 2048, 1000, blob, offs, lens)
    assert head["tiles"] == 0
    assert cats.get("data") and cats.get("end_in_body")
