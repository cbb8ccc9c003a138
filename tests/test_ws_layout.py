"""The workspace carver (rpc_amd/csrc/workspace.h) on the host: tests/cpu_emu/ws_layout_check.cpp
carves five arrays, one per element size 1 / 2 / 4 / 8 / 16, at every combination of the
counts 0, 1, 63, 64, 65, 4095 and 2^20, and checks that the measuring pass and the carving
pass agree, that the arrays are 256-aligned, in order, disjoint and inside the block, that a
block one byte short is refused for good, that a count near SIZE_MAX / sizeof(T) is refused
without wrapping, and that rest() is exactly what is left."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_layout(tmp_path):
    """With AddressSanitizer and UBSan where this g++ links them (the program touches the
    first and last byte of every array it carves)."""
    exe, src = str(tmp_path / "ws_layout_check"), os.path.join(REPO, "tests", "cpu_emu", "ws_layout_check.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:  # (does it link and start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == "ok %d layouts" % 7 ** 5
