"""The frame resolve's C-ABI without a GPU (rpc_frames_resolve_device, include/rpccrc.h): the
symbol is exported, declared and bound, every RPCCRC_EINVAL of the header is returned before a
device is touched (the pointers given here are never valid device pointers, and on a machine
without a GPU any call that reached the device layer would read RPCCRC_ENODEV instead), and the
header's constants are the Python ones."""
import os
import re

import resolve_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "rpccrc.h")
MAP = os.path.join(REPO, "rpc_amd", "csrc", "exports.map")
NAME = "rpc_frames_resolve_device"
OK, EINVAL = 0, -22
P = 0x1000  # a non-NULL pointer nobody dereferences


def call(bodies=P, bodies_bytes=64, offs=P, lens=P, types=None, n=4, pending=P, npending=4, kind=P, rid=P,
         roff=P, rlen=P, eoff=P, elen=P, slot=P, slot_entry=P, opened=P, nopen=P):
    from rpc_amd import _lib
    return _lib.rpc_frames_resolve_device(bodies, bodies_bytes, offs, lens, types, n, pending, npending, kind, rid,
                                          roff, rlen, eoff, elen, slot, slot_entry, opened, nopen, None)


def test_symbol_is_exported_declared_and_bound():
    from rpc_amd import _lib
    assert NAME in _lib.EXPORTS and hasattr(_lib.lib, NAME)
    assert re.search(r"^\s*%s;" % NAME, open(MAP).read(), re.M)
    hdr = open(HDR).read()
    m = re.search(r"RPCCRC_API int %s\(([^;]*)\);" % NAME, hdr)
    assert m, "the header does not declare it"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["const uint8_t *d_bodies", "uint64_t bodies_bytes", "const uint64_t *d_body_offsets",
                    "const uint32_t *d_body_lens", "const uint16_t *d_reply_types", "uint64_t n",
                    "const uint32_t *d_pending_ids", "uint32_t npending", "uint8_t *d_kind", "uint32_t *d_id",
                    "uint32_t *d_result_off", "uint32_t *d_result_len", "uint32_t *d_error_off",
                    "uint32_t *d_error_len", "uint32_t *d_slot", "uint32_t *d_slot_entry", "uint32_t *d_open",
                    "uint32_t *d_nopen", "void *stream"]
    assert len(_lib.rpc_frames_resolve_device.argtypes) == len(args)


def test_every_einval_comes_before_any_device():
    assert _errno_name(EINVAL) == "invalid argument"
    assert call(n=0xFFFFFFFF) == EINVAL
    assert call(n=1 << 40) == EINVAL
    assert call(npending=rc.MAX_PENDING + 1) == EINVAL
    assert call(npending=0xFFFFFFFF) == EINVAL
    assert call(offs=None) == EINVAL
    assert call(lens=None) == EINVAL
    assert call(bodies=None) == EINVAL
    assert call(pending=None) == EINVAL
    assert call(opened=None) == EINVAL
    assert call(nopen=None) == EINVAL
    # the same with every output left out: the checks do not hang on one
    assert call(n=0xFFFFFFFF, kind=None, rid=None, roff=None, rlen=None, eoff=None, elen=None, slot=None,
                slot_entry=None, opened=None, nopen=None) == EINVAL


def test_nothing_to_do_needs_no_device():
    """n == 0 with none of d_slot_entry / d_open / d_nopen: RPCCRC_OK with no device touched, with
    or without pending ids, NULL arrays allowed where nothing would be read."""
    none = dict(slot_entry=None, opened=None, nopen=None)
    assert call(n=0, **none) == OK
    assert call(n=0, offs=None, lens=None, bodies=None, bodies_bytes=0, **none) == OK
    assert call(n=0, npending=0, pending=None, **none) == OK
    assert call(n=0, npending=0, pending=None, kind=None, rid=None, roff=None, rlen=None, eoff=None, elen=None,
                slot=None, **none) == OK


def _errno_name(code):
    from rpc_amd import _lib
    return _lib.rpc_crc32_strerror(code).decode()


def test_header_constants_are_the_python_ones():
    import rpc_amd
    hdr = open(HDR).read()

    def const(name):
        m = re.search(r"#define RPC_RESOLVE_%s (\S+)" % name, hdr)
        assert m, name
        text = m.group(1)
        if name == "MAX_PENDING":
            assert re.search(r"#define RPC_RESOLVE_MAX_PENDING \(1u << 24\)", hdr)
            return 1 << 24
        return int(text.rstrip("u"), 0)

    names = ["NONE", "MATCHED", "UNKNOWN", "DUPLICATE", "INVALID", "DEFER", "RANGE", "NO_SLOT", "MAX_PENDING"]
    for name in names:
        assert const(name) == getattr(rpc_amd, "RESOLVE_" + name) == getattr(rc, name), name
        assert "RESOLVE_" + name in rpc_amd.__all__
    assert len({const(k) for k in names[:7]}) == 7
    assert "frames_resolve" in rpc_amd.__all__ and "FrameResolve" in rpc_amd.__all__
    assert rpc_amd.FrameResolve._fields == ("kind", "id", "result_off", "result_len", "error_off", "error_len", "slot",
                                            "slot_entry", "open", "nopen")
