"""rpc_frames_route_device's argument checks, which are made before any device is touched
(include/rpccrc.h), the optional outputs and the n == 0 call with nothing to write: through
rpc_amd._lib, no GPU needed.  Pointers that must only be non-NULL are given a dummy address: a
call that returns RPCCRC_EINVAL never looks at them."""
import re
import os

from rpc_amd import _lib
import rpc_amd

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def route(bodies=P, bodies_bytes=64, offs=P, lens=P, types=P, n=4, names=P, method_bytes=10, moff=P, nmethods=2,
          kind=None, method=None, rid=None, params_off=None, params_len=None, order=None, group_first=None):
    return _lib.rpc_frames_route_device(bodies, bodies_bytes, offs, lens, types, n, names, method_bytes, moff, nmethods,
                                        kind, method, rid, params_off, params_len, order, group_first, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert route(n=0xFFFFFFFF) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_too_many_entries():
    assert route(n=0xFFFFFFFF) == EINVAL
    assert route(n=1 << 40) == EINVAL


def test_table_limits():
    assert route(nmethods=257) == EINVAL
    assert route(method_bytes=4097) == EINVAL
    assert route(n=0, nmethods=257) == EINVAL
    assert route(n=0, method_bytes=4097) == EINVAL
    assert route(n=0, nmethods=256, method_bytes=4096) == OK


def test_needed_pointers():
    assert route(offs=None) == EINVAL
    assert route(lens=None) == EINVAL
    assert route(bodies=None, bodies_bytes=1) == EINVAL
    assert route(moff=None, nmethods=1) == EINVAL
    assert route(names=None, method_bytes=1) == EINVAL
    assert route(n=0, bodies=None, bodies_bytes=1) == EINVAL
    assert route(n=0, moff=None, nmethods=1) == EINVAL
    assert route(n=0, names=None, method_bytes=1) == EINVAL


def test_order_outputs_come_as_a_pair():
    assert route(order=P) == EINVAL
    assert route(group_first=P) == EINVAL
    assert route(n=0, order=P) == EINVAL
    assert route(n=0, group_first=P) == EINVAL
    assert route(order=P, kind=P, rid=P) == EINVAL


def test_no_entries_and_nothing_to_write_needs_no_device():
    assert route(n=0) == OK
    assert route(n=0, bodies=None, bodies_bytes=0, offs=None, lens=None, types=None, names=None, method_bytes=0,
                 moff=None, nmethods=0) == OK
    assert route(n=0, kind=P, method=P, rid=P, params_off=P, params_len=P) == OK  # (n entries of each)
    assert route(n=0, types=None) == OK


def test_binding_and_constants():
    assert "rpc_frames_route_device" in _lib.EXPORTS
    header = open(os.path.join(REPO, "include", "rpccrc.h")).read()
    for name in ("NONE", "CALL", "NOT_FOUND", "INVALID", "DEFER", "RANGE", "NO_METHOD", "MAX_BODY", "MAX_DEPTH",
                 "MAX_TOKENS", "MAX_METHODS", "MAX_METHOD_BYTES"):
        m = re.search(r"#define RPC_ROUTE_%s (0x[0-9A-Fa-f]+|\d+)u" % name, header)
        assert m and int(m.group(1), 0) == getattr(rpc_amd, "ROUTE_" + name), name
    assert [rpc_amd.ROUTE_NONE, rpc_amd.ROUTE_CALL, rpc_amd.ROUTE_NOT_FOUND, rpc_amd.ROUTE_INVALID, rpc_amd.ROUTE_DEFER,
            rpc_amd.ROUTE_RANGE] == [0, 1, 2, 3, 4, 5]
    assert rpc_amd.ROUTE_NO_METHOD == 0xFFFF and rpc_amd.ROUTE_MAX_BODY == rpc_amd.MAX_BODY_LEN == 1024
    assert (rpc_amd.ROUTE_MAX_DEPTH, rpc_amd.ROUTE_MAX_TOKENS) == (32, 256)
