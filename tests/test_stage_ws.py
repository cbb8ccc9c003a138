"""Every frame stage's workspace layout (the xxx_ws_layout function beside each stage's Args in
rpc_amd/csrc/frames*.h) over the carver of rpc_amd/csrc/workspace.h, on the host:
tests/cpu_emu/stage_ws_check.cpp measures and carves each layout under every combination of its
conditions, at nine counts and three scan sizes, and checks that the arrays are 256-aligned, in
order, disjoint, inside the block and at least as long as the kernels index them, and that a block
one byte short is refused."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One line per layout: the stage and the layouts checked (counts x scan sizes x conditions).
EXPECTED = """ok verify 9 layouts
ok stamp 9 layouts
ok pack 27 layouts
ok unpack 27 layouts
ok carry 27 layouts
ok route 81 layouts
ok reply 27 layouts
ok values 81 layouts
ok request 27 layouts
ok resolve 432 layouts
ok scan 81 layouts
ok scan_tiled 27 layouts"""


def test_stage_ws_layouts(tmp_path):
    """With AddressSanitizer and UBSan where this g++ links them (the program touches the
    first and last byte of every array it carves)."""
    exe, src = str(tmp_path / "stage_ws_check"), os.path.join(REPO, "tests", "cpu_emu", "stage_ws_check.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:  # (does it link and start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == EXPECTED
