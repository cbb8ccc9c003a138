"""The reference client's own request encoder behind tests/dropin/ref_encode.c: built into a
directory of the caller's (a temporary one; nothing enters the tree) from the reference's
client/rpc_codec.c and third_party/cJSON.c, compiled in place.  Where the reference tree is
absent, build() returns None."""
import os
import re
import struct
import subprocess
from typing import NamedTuple, Optional

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "tests", "dropin", "ref_encode.c")
NONE = 0xFFFFFFFF


def ref_dir():
    """REF_DIR of the environment, else oracle/Makefile's default."""
    m = re.search(r"^REF_DIR \?= (\S+)", open(os.path.join(REPO, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REF_DIR") or m.group(1)


def build(directory) -> Optional[str]:
    ref = ref_dir()
    srcs = [os.path.join(ref, "client", "rpc_codec.c"), os.path.join(ref, "third_party", "cJSON.c")]
    if not all(os.path.exists(s) for s in srcs):
        return None
    exe = os.path.join(str(directory), "ref_encode")
    inc = ["-I" + os.path.join(ref, *p) for p in (("client",), ("client", "third_party"), ("third_party",), ())]
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", *inc, "-o", exe, DRIVER, *srcs, "-lm"], check=True)
    return exe


class Encoded(NamedTuple):
    printed: Optional[bytes]  # cJSON_PrintUnformatted of the parsed params; None: no params, or not parsed
    request: Optional[bytes]  # what rpc_codec_encode_request returned


def run(exe, triples):
    """triples: (name, params text or None, id)."""
    def text(b):
        return struct.pack("<I", NONE) if b is None else struct.pack("<I", len(b)) + bytes(b)
    blob = b"".join(text(name) + text(params) + struct.pack("<I", rid) for name, params, rid in triples)
    out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
    res, at = [], 0

    def member():
        nonlocal at
        (n,) = struct.unpack_from("<I", out, at)
        at += 4
        if n == NONE:
            return None
        at += n
        return out[at - n:at]

    for _ in triples:
        res.append(Encoded(member(), member()))
    assert at == len(out)
    return res
