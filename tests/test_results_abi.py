"""rpc_frames_results_device's argument checks, which are made before any device is touched
(include/rpccrc.h), and the n == 0 call: through rpc_amd._lib, no GPU needed.  Pointers that
must only be non-NULL are given a dummy address: a call that returns RPCCRC_EINVAL never looks
at them."""
import ctypes
import os
import re

from rpc_amd import _lib
import rpc_amd
import results_cases as rs

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_OUTS = ("slot_status", "slot_value", "slot_error_status", "slot_error_code", "slot_str_base")


def results(bodies=P, bodies_bytes=64, offs=P, lens=P, kind=P, slot=P, roff=P, rlen=P, eoff=P, elen=P, slot_entry=P, n=4,
            pending_method=P, npending=3, types=P, nmethods=2, status=None, value=None, error_status=None,
            error_code=None, error_message=None, slot_status=None, slot_value=None, slot_error_status=None,
            slot_error_code=None, slot_str_base=None, ndefer=None):
    return _lib.rpc_frames_results_device(bodies, bodies_bytes, offs, lens, kind, slot, roff, rlen, eoff, elen, slot_entry,
                                          n, pending_method, npending, types, nmethods, status, value, error_status,
                                          error_code, error_message, slot_status, slot_value, slot_error_status,
                                          slot_error_code, slot_str_base, ndefer, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert results(n=0xFFFFFFFF) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_too_many_entries():
    assert results(n=0xFFFFFFFF) == EINVAL
    assert results(n=1 << 40) == EINVAL


def test_limits():
    for n in (0, 4):
        assert results(n=n, npending=(1 << 24) + 1) == EINVAL
        assert results(n=n, npending=0xFFFFFFFF) == EINVAL
        assert results(n=n, nmethods=257) == EINVAL
    assert results(n=0, npending=1 << 24, nmethods=256) == OK


def test_needed_pointers():
    for name in ("offs", "lens", "kind", "slot", "roff", "rlen", "eoff", "elen"):
        assert results(**{name: None}) == EINVAL, name
    for n in (0, 4):
        assert results(n=n, bodies=None, bodies_bytes=1) == EINVAL
        assert results(n=n, pending_method=None, npending=1) == EINVAL
        assert results(n=n, types=None, nmethods=1) == EINVAL


def test_a_slot_output_needs_slot_entry():
    for n in (0, 4):
        for name in SLOT_OUTS:
            assert results(n=n, slot_entry=None, **{name: P}) == EINVAL, name
            assert results(n=n, slot_entry=None, npending=0, pending_method=None, **{name: P}) == EINVAL, name
        assert results(n=n, slot_entry=None, **{name: P for name in SLOT_OUTS}) == EINVAL
    assert results(n=0, slot_entry=None) == OK  # (the per-entry outputs need none)


def test_no_entries_needs_no_device():
    assert results(n=0) == OK
    assert results(n=0, bodies=None, bodies_bytes=0, offs=None, lens=None, kind=None, slot=None, roff=None, rlen=None,
                   eoff=None, elen=None, slot_entry=None, pending_method=None, npending=0, types=None, nmethods=0) == OK
    assert results(n=0, status=P, value=P, error_status=P, error_code=P, error_message=P) == OK  # (n entries of each)
    assert results(n=0, npending=0, pending_method=None, **{name: P for name in SLOT_OUTS}) == OK  # (npending of each)


def test_symbol_binding_and_constants():
    assert "rpc_frames_results_device" in _lib.EXPORTS
    lib = os.path.join(REPO, "rpc_amd", "lib", "librpccrc.so")
    assert ctypes.CDLL(lib).rpc_frames_results_device  # (the dynamic symbol table has it)
    assert re.search(r"^\s*rpc_frames_results_device;", open(os.path.join(REPO, "rpc_amd", "csrc", "exports.map")).read(),
                     re.M)
    header = open(os.path.join(REPO, "include", "rpccrc.h")).read()
    assert "RPCCRC_API int rpc_frames_results_device(" in header
    names = ("RESULTS_NONE", "RESULTS_OK", "RESULTS_ABSENT", "RESULTS_MISMATCH", "RESULTS_DEFER", "RESULTS_RANGE",
             "RESULTS_BAD_SCHEMA")
    for name in names:
        m = re.search(r"#define RPC_%s (0x[0-9A-Fa-f]+|\d+)u" % name, header)
        assert m and int(m.group(1), 0) == getattr(rpc_amd, name), name
    assert [getattr(rpc_amd, name) for name in names] == list(range(7))
    assert [rs.NONE, rs.OK, rs.ABSENT, rs.MISMATCH, rs.DEFER, rs.RANGE, rs.BAD_SCHEMA] == list(range(7))
    assert rpc_amd.frames_results and rpc_amd.FrameResults._fields[:2] == ("status", "value")
