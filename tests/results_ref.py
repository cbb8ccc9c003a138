"""What the reference's generated client would read from a reply, behind
tests/dropin/ref_results.c: built into a directory of the caller's (a temporary one; nothing
enters the tree) from the reference's client/rpc_codec.c and third_party/cJSON.c, compiled in
place.  Where the reference tree is absent, build() returns None.

``client_value`` restates the five lines of client/gen/rpc_client_gen.c over the driver's facts:
the string; strtoll of a string or (int64_t)valuedouble; (int32_t)valuedouble; valuedouble;
cJSON_IsTrue of a bool -- and the default in every other case."""
import math
import os
import struct
import subprocess
from typing import NamedTuple, Optional

import args_cases as ac
from resolve_ref import ref_dir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "tests", "dropin", "ref_results.c")


def build(directory) -> Optional[str]:
    ref = ref_dir()
    srcs = [os.path.join(ref, "client", "rpc_codec.c"), os.path.join(ref, "third_party", "cJSON.c")]
    if not all(os.path.exists(s) for s in srcs):
        return None
    exe = os.path.join(str(directory), "ref_results")
    inc = ["-I" + os.path.join(ref, *p) for p in (("client",), ("client", "third_party"), ("third_party",), ())]
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", *inc, "-o", exe, DRIVER, *srcs, "-lm"], check=True)
    return exe


class Node(NamedTuple):
    there: bool
    is_string: bool
    is_number: bool
    is_bool: bool
    is_true: bool
    bits: int                # of valuedouble
    strtoll: int             # of valuestring (signed), 0 without one
    string: Optional[bytes]  # valuestring


class Facts(NamedTuple):
    rc: int  # rpc_codec_decode_response's: 0 or -1
    result: Node
    code: Node
    message: Node


def run(exe, bodies):
    blob = b"".join(struct.pack("<I", len(b)) + bytes(b) for b in bodies)
    out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
    res, at = [], 0

    def node():
        nonlocal at
        there, s, n, b, t, bits, ll, ln = struct.unpack_from("<5BQqI", out, at)
        at += 25
        text = None
        if ln != 0xFFFFFFFF:
            text, at = out[at:at + ln], at + ln
        return Node(bool(there), bool(s), bool(n), bool(b), bool(t), bits, ll, text)

    for _ in bodies:
        (rc,) = struct.unpack_from("<i", out, at)
        at += 4
        res.append(Facts(rc, node(), node(), node()))
    assert at == len(out)
    return res


def client_value(t, node):
    """What the generated function for result type t returns: ("str", bytes or None), or
    ("bits", the 64-bit pattern of the integer or the double), or None where the C cast is
    undefined (the value does not fit the integer type)."""
    d = struct.unpack("<d", struct.pack("<Q", node.bits))[0]
    if t == ac.STR:
        return "str", node.string if node.there and node.is_string else None
    if t == ac.BOOL:
        return "bits", 1 if node.there and node.is_bool and node.is_true else 0
    if t == ac.I64 and node.there and node.is_string:
        return "bits", node.strtoll & ac.M64
    if not (node.there and node.is_number):
        return "bits", 0
    if t == ac.F64:
        return "bits", node.bits
    fits = -2.0**31 - 1 < d < 2.0**31 if t == ac.I32 else -2.0**63 <= d < 2.0**63  # (trunc(d) is in the type)
    if math.isnan(d) or not fits:
        return None
    return "bits", int(d) & ac.M64
