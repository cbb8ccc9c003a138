"""The frame request's workspace layout (request_ws_layout of rpc_amd/csrc/frames_request.h) over
the carver of rpc_amd/csrc/workspace.h, on the host: tests/cpu_emu/request_ws_check.cpp measures
and carves it at nine entry counts and three scan sizes and checks that the six arrays are
256-aligned, in order, disjoint, inside the block and as long as the kernels index them, and that
a block one byte short is refused."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_request_ws_layout(tmp_path):
    """With AddressSanitizer and UBSan where this g++ links them (the program touches the
    first and last byte of every array it carves)."""
    exe, src = str(tmp_path / "request_ws_check"), os.path.join(REPO, "tests", "cpu_emu", "request_ws_check.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True)
    if san.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:  # (does it link and start?)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == "ok 27 layouts"
