"""rpc_frames_request_device's argument checks, which are made before any device is touched
(include/rpccrc.h), the n == 0 call with nothing to write, and the REQUEST_* constants against
the header: through rpc_amd._lib, no GPU needed.  Pointers that must only be non-NULL are
given a dummy address: a call that returns RPCCRC_EINVAL never looks at them."""
import os
import re

import rpc_amd
from rpc_amd import _lib

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpccrc.h")


def request(method=P, rid=P, types=P, n=4, names=P, method_bytes=16, method_off=P, nmethods=3, params=P, params_bytes=64,
            params_offsets=P, params_lens=P, conn_first=None, nconn=0, out=None, out_cap=0, body_offsets=None,
            body_lens=None, types_out=None, request_status=None, conn_bytes_first=None, total=None):
    return _lib.rpc_frames_request_device(method, rid, types, n, names, method_bytes, method_off, nmethods, params,
                                          params_bytes, params_offsets, params_lens, conn_first, nconn, out, out_cap,
                                          body_offsets, body_lens, types_out, request_status, conn_bytes_first, total,
                                          None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert request(n=0xFFFFFFFF) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_too_many_entries():
    assert request(n=0xFFFFFFFF) == EINVAL
    assert request(n=1 << 40) == EINVAL


def test_table_over_the_routes_limits():
    assert request(nmethods=rpc_amd.ROUTE_MAX_METHODS + 1) == EINVAL
    assert request(method_bytes=rpc_amd.ROUTE_MAX_METHOD_BYTES + 1) == EINVAL
    assert request(n=0, nmethods=rpc_amd.ROUTE_MAX_METHODS + 1) == EINVAL
    assert request(n=0, method_bytes=rpc_amd.ROUTE_MAX_METHOD_BYTES + 1) == EINVAL
    assert request(n=0, nmethods=rpc_amd.ROUTE_MAX_METHODS, method_bytes=rpc_amd.ROUTE_MAX_METHOD_BYTES) == OK


def test_entries_need_methods_ids_offsets_and_lengths():
    assert request(method=None) == EINVAL
    assert request(rid=None) == EINVAL
    assert request(params_offsets=None) == EINVAL
    assert request(params_lens=None) == EINVAL
    assert request(method=None, rid=None, types=None, params_offsets=None, params_lens=None, params=None,
                   params_bytes=0) == EINVAL


def test_params_bytes_need_params():
    assert request(params=None, params_bytes=1) == EINVAL
    assert request(n=0, params=None, params_bytes=12) == EINVAL


def test_methods_need_offsets_and_bytes_need_names():
    assert request(method_off=None) == EINVAL
    assert request(names=None) == EINVAL
    assert request(n=0, method_off=None, nmethods=1) == EINVAL
    assert request(n=0, names=None, method_bytes=1) == EINVAL
    assert request(n=0, names=None, method_bytes=0, method_off=None, nmethods=0) == OK


def test_out_cap_needs_out():
    assert request(out=None, out_cap=1) == EINVAL
    assert request(n=0, out=None, out_cap=12) == EINVAL


def test_conn_bytes_first_needs_conn_first():
    assert request(conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL
    assert request(n=0, conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL


def test_nconn_needs_conn_first():
    assert request(nconn=3, conn_first=None) == EINVAL
    assert request(n=0, nconn=1, conn_first=None) == EINVAL


def test_no_entries_and_nothing_to_write_needs_no_device():
    assert request(n=0) == OK
    assert request(n=0, method=None, rid=None, types=None, params=None, params_bytes=0, params_offsets=None,
                   params_lens=None) == OK
    assert request(n=0, body_offsets=P, body_lens=P, types_out=P, request_status=P) == OK  # (n entries of each)
    assert request(n=0, conn_first=P, nconn=5) == OK
    assert request(n=0, out=P, out_cap=100) == OK


def test_constants_are_the_headers():
    text = open(HEADER).read()
    names = ("NONE", "CALL", "RAW", "BAD_METHOD", "RANGE", "NO_ROOM")
    for k, name in enumerate(names):
        m = re.search(r"#define RPC_REQUEST_%s (\d+)u\b" % name, text)
        assert m and int(m.group(1)) == k == getattr(rpc_amd, "REQUEST_" + name), name
    assert len(re.findall(r"#define RPC_REQUEST_\w+ ", text)) == len(names)


def test_binding_is_listed():
    assert "rpc_frames_request_device" in _lib.EXPORTS
    assert re.search(r"\brpc_frames_request_device\s*;", open(os.path.join(os.path.dirname(HEADER), "..", "rpc_amd", "csrc",
                                                                          "exports.map")).read())
    assert "frames_request" in rpc_amd.__all__ and "FrameRequest" in rpc_amd.__all__
