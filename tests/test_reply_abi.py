"""rpc_frames_reply_device's argument checks, which are made before any device is touched
(include/rpccrc.h), the n == 0 call with nothing to write, and the REPLY_* constants against
the header: through rpc_amd._lib, no GPU needed.  Pointers that must only be non-NULL are
given a dummy address: a call that returns RPCCRC_EINVAL never looks at them."""
import os
import re

import rpc_amd
from rpc_amd import _lib

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpccrc.h")


def reply(kind=P, rid=P, status=P, reply_types=P, n=4, values=P, values_bytes=64, value_offsets=P, value_lens=P,
          conn_first=None, nconn=0, out=None, out_cap=0, body_offsets=None, body_lens=None, types_out=None,
          reply_status=None, conn_bytes_first=None, total=None):
    return _lib.rpc_frames_reply_device(kind, rid, status, reply_types, n, values, values_bytes, value_offsets,
                                        value_lens, conn_first, nconn, out, out_cap, body_offsets, body_lens, types_out,
                                        reply_status, conn_bytes_first, total, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert reply(n=0xFFFFFFFF) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_too_many_entries():
    assert reply(n=0xFFFFFFFF) == EINVAL
    assert reply(n=1 << 40) == EINVAL


def test_entries_need_ids():
    assert reply(rid=None) == EINVAL
    assert reply(rid=None, kind=None, status=None, reply_types=None) == EINVAL


def test_entries_need_value_offsets_and_lengths():
    assert reply(value_offsets=None) == EINVAL
    assert reply(value_lens=None) == EINVAL
    assert reply(value_offsets=None, value_lens=None, values=None, values_bytes=0) == EINVAL


def test_values_bytes_need_values():
    assert reply(values=None, values_bytes=1) == EINVAL
    assert reply(n=0, values=None, values_bytes=12) == EINVAL


def test_out_cap_needs_out():
    assert reply(out=None, out_cap=1) == EINVAL
    assert reply(n=0, out=None, out_cap=12) == EINVAL


def test_conn_bytes_first_needs_conn_first():
    assert reply(conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL
    assert reply(n=0, conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL


def test_nconn_needs_conn_first():
    assert reply(nconn=3, conn_first=None) == EINVAL
    assert reply(n=0, nconn=1, conn_first=None) == EINVAL


def test_no_entries_and_nothing_to_write_needs_no_device():
    assert reply(n=0) == OK
    assert reply(n=0, kind=None, rid=None, status=None, reply_types=None, values=None, values_bytes=0, value_offsets=None,
                 value_lens=None) == OK
    assert reply(n=0, body_offsets=P, body_lens=P, types_out=P, reply_status=P) == OK  # (n entries of each)
    assert reply(n=0, conn_first=P, nconn=5) == OK
    assert reply(n=0, out=P, out_cap=100) == OK


def test_constants_are_the_headers():
    text = open(HEADER).read()
    names = ("NONE", "RESULT", "ERROR", "RAW", "RANGE", "NO_ROOM")
    for k, name in enumerate(names):
        m = re.search(r"#define RPC_REPLY_%s (\d+)u\b" % name, text)
        assert m and int(m.group(1)) == k == getattr(rpc_amd, "REPLY_" + name), name
    assert len(re.findall(r"#define RPC_REPLY_\w+ ", text)) == len(names)


def test_binding_is_listed():
    assert "rpc_frames_reply_device" in _lib.EXPORTS
    assert re.search(r"\brpc_frames_reply_device\s*;", open(os.path.join(os.path.dirname(HEADER), "..", "rpc_amd", "csrc",
                                                                        "exports.map")).read())
