"""rpc_frames_args_device's argument checks, which are made before any device is touched
(include/rpccrc.h), and the n == 0 call: through rpc_amd._lib, no GPU needed.  Pointers that
must only be non-NULL are given a dummy address: a call that returns RPCCRC_EINVAL never looks
at them."""
import ctypes
import os
import re

from rpc_amd import _lib
import rpc_amd

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def args(bodies=P, bodies_bytes=64, offs=P, lens=P, kind=P, method=P, poff=P, plen=P, n=4, first=P, nmethods=2, types=P,
         noff=P, nparams=3, names=P, name_bytes=5, width=2, slots=None, status=None, reply_status=None):
    return _lib.rpc_frames_args_device(bodies, bodies_bytes, offs, lens, kind, method, poff, plen, n, first, nmethods,
                                       types, noff, nparams, names, name_bytes, width, slots, status, reply_status, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert args(n=0xFFFFFFFF) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_too_many_entries():
    assert args(n=0xFFFFFFFF) == EINVAL
    assert args(n=1 << 40) == EINVAL


def test_schema_limits():
    assert args(nmethods=257) == EINVAL
    assert args(nparams=1025) == EINVAL
    assert args(name_bytes=4097) == EINVAL
    assert args(n=0, nmethods=257) == EINVAL
    assert args(n=0, nparams=1025) == EINVAL
    assert args(n=0, name_bytes=4097) == EINVAL
    assert args(n=0, nmethods=256, nparams=1024, name_bytes=4096, width=8) == OK


def test_width():
    for n in (0, 4):
        assert args(n=n, width=0) == EINVAL
        assert args(n=n, width=9) == EINVAL
        assert args(n=n, width=0xFFFFFFFF) == EINVAL
    assert args(n=0, width=1) == OK


def test_needed_pointers():
    for name in ("offs", "lens", "kind", "method", "poff", "plen"):
        assert args(**{name: None}) == EINVAL, name
    assert args(bodies=None, bodies_bytes=1) == EINVAL
    assert args(first=None, nmethods=1) == EINVAL
    assert args(types=None, nparams=1) == EINVAL
    assert args(noff=None, nparams=1) == EINVAL
    assert args(names=None, name_bytes=1) == EINVAL
    assert args(n=0, bodies=None, bodies_bytes=1) == EINVAL
    assert args(n=0, first=None, nmethods=1) == EINVAL
    assert args(n=0, types=None, nparams=1) == EINVAL
    assert args(n=0, noff=None, nparams=1) == EINVAL
    assert args(n=0, names=None, name_bytes=1) == EINVAL


def test_no_entries_needs_no_device():
    assert args(n=0) == OK
    assert args(n=0, bodies=None, bodies_bytes=0, offs=None, lens=None, kind=None, method=None, poff=None, plen=None,
                first=None, nmethods=0, types=None, noff=None, nparams=0, names=None, name_bytes=0) == OK
    assert args(n=0, slots=P, status=P, reply_status=P) == OK  # (n entries of each)


def test_symbol_binding_and_constants():
    assert "rpc_frames_args_device" in _lib.EXPORTS
    lib = os.path.join(REPO, "rpc_amd", "lib", "librpccrc.so")
    assert ctypes.CDLL(lib).rpc_frames_args_device  # (the dynamic symbol table has it)
    header = open(os.path.join(REPO, "include", "rpccrc.h")).read()
    for name in ("ARGS_NONE", "ARGS_OK", "ARGS_INVALID", "ARGS_DEFER", "ARGS_RANGE", "ARGS_BAD_SCHEMA", "ARG_I32", "ARG_I64",
                 "ARG_F64", "ARG_BOOL", "ARG_STR", "ARGS_MAX_PARAMS", "ARGS_MAX_SCHEMA_PARAMS", "ARGS_MAX_NAME_BYTES"):
        m = re.search(r"#define RPC_%s (0x[0-9A-Fa-f]+|\d+)u" % name, header)
        assert m and int(m.group(1), 0) == getattr(rpc_amd, name), name
    assert [rpc_amd.ARGS_NONE, rpc_amd.ARGS_OK, rpc_amd.ARGS_INVALID, rpc_amd.ARGS_DEFER, rpc_amd.ARGS_RANGE,
            rpc_amd.ARGS_BAD_SCHEMA] == [0, 1, 2, 3, 4, 5]
    assert (rpc_amd.ARGS_MAX_PARAMS, rpc_amd.ARGS_MAX_SCHEMA_PARAMS, rpc_amd.ARGS_MAX_NAME_BYTES) == (8, 1024, 4096)
