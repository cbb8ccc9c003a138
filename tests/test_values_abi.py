"""rpc_frames_values_device's argument checks, which are made before any device is touched
(include/rpccrc.h), the n == 0 call with nothing to write, and the VALUES_* constants against
the header: through rpc_amd._lib, no GPU needed.  Pointers that must only be non-NULL are
given a dummy address: a call that returns RPCCRC_EINVAL never looks at them."""
import os
import re

import rpc_amd
from rpc_amd import _lib

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpccrc.h")
RESULT, PARAMS = rpc_amd.VALUES_FORM_RESULT, rpc_amd.VALUES_FORM_PARAMS


def values(form=RESULT, mode=None, status=None, method=P, slots=P, width=1, n=4, rtypes=P, first=P, nmethods=3, ptypes=P,
           noff=P, nparams=5, names=P, name_bytes=9, strings=P, strings_bytes=64, str_base=None, texts=P, texts_bytes=64,
           text_offsets=P, text_lens=P, out=None, out_cap=0, value_offsets=None, value_lens=None, state=None,
           reply_status=None, ndefer=None, total=None):
    return _lib.rpc_frames_values_device(form, mode, status, method, slots, width, n, rtypes, first, nmethods, ptypes, noff,
                                         nparams, names, name_bytes, strings, strings_bytes, str_base, texts, texts_bytes,
                                         text_offsets, text_lens, out, out_cap, value_offsets, value_lens, state,
                                         reply_status, ndefer, total, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert values(n=0xFFFFFFFF) == EINVAL


def test_form():
    for form in (2, -1, 7):
        assert values(form=form) == EINVAL and values(form=form, n=0) == EINVAL


def test_too_many_items():
    assert values(n=0xFFFFFFFF) == EINVAL and values(n=1 << 40) == EINVAL
    assert values(form=PARAMS, n=0x20000000, width=8) == EINVAL  # (n * width items)
    assert values(form=PARAMS, n=0x7FFFFFFF, width=3) == EINVAL


def test_width_and_limits():
    assert values(width=0) == EINVAL and values(width=9) == EINVAL and values(n=0, width=0) == EINVAL
    assert values(nmethods=257) == EINVAL
    assert values(form=PARAMS, nparams=1025) == EINVAL and values(form=PARAMS, name_bytes=4097) == EINVAL


def test_entries_need_methods_and_slots():
    assert values(method=None) == EINVAL and values(slots=None) == EINVAL
    assert values(form=PARAMS, method=None) == EINVAL


def test_schema_pointers_by_form():
    assert values(rtypes=None) == EINVAL
    assert values(form=PARAMS, first=None) == EINVAL
    assert values(form=PARAMS, ptypes=None) == EINVAL and values(form=PARAMS, noff=None) == EINVAL
    assert values(form=PARAMS, names=None) == EINVAL
    # the other form's arrays are not looked at
    assert values(n=0, form=PARAMS, rtypes=None) == OK
    assert values(n=0, first=None, ptypes=None, noff=None, names=None) == OK


def test_bytes_need_buffers():
    assert values(strings=None) == EINVAL and values(texts=None) == EINVAL
    assert values(out=None, out_cap=1) == EINVAL and values(n=0, out=None, out_cap=12) == EINVAL


def test_no_entries_and_nothing_to_write_needs_no_device():
    assert values(n=0) == OK
    assert values(n=0, method=None, slots=None, strings=None, strings_bytes=0, texts=None, texts_bytes=0, rtypes=None,
                  nmethods=0, text_offsets=None, text_lens=None) == OK
    assert values(n=0, value_offsets=P, value_lens=P, state=P, reply_status=P) == OK  # (n entries of each)
    assert values(n=0, out=P, out_cap=100) == OK


def test_constants_are_the_headers():
    text = open(HEADER).read()
    names = ("NONE", "OK", "TEXT", "DEFER", "RANGE", "BAD_SCHEMA", "NO_ROOM")
    for k, name in enumerate(names):
        m = re.search(r"#define RPC_VALUES_%s (\d+)u\b" % name, text)
        assert m and int(m.group(1)) == k == getattr(rpc_amd, "VALUES_" + name), name
    for k, name in enumerate(("MODE_NONE", "MODE_ENCODE", "MODE_TEXT")):
        m = re.search(r"#define RPC_VALUES_%s (\d+)u\b" % name, text)
        assert m and int(m.group(1)) == k == getattr(rpc_amd, "VALUES_" + name), name
    for k, name in enumerate(("FORM_RESULT", "FORM_PARAMS")):
        m = re.search(r"#define RPC_VALUES_%s (\d+)\b" % name, text)
        assert m and int(m.group(1)) == k == getattr(rpc_amd, "VALUES_" + name), name
    assert len(re.findall(r"#define RPC_VALUES_\w+ ", text)) == len(names) + 5


def test_binding_is_listed():
    assert "rpc_frames_values_device" in _lib.EXPORTS
    assert re.search(r"\brpc_frames_values_device\s*;", open(os.path.join(os.path.dirname(HEADER), "..", "rpc_amd", "csrc",
                                                                         "exports.map")).read())
    assert "frames_values" in rpc_amd.__all__ and "FrameValues" in rpc_amd.__all__ and "result_types" in rpc_amd.__all__
