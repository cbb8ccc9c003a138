"""rpc_frames_carry_device's argument checks, which are made before any device is touched
(include/rpccrc.h), and the nconn == 0 call with nothing to write: through rpc_amd._lib, no
GPU needed.  Pointers that must only be non-NULL are given a dummy address: a call that
returns RPCCRC_EINVAL never looks at them."""
import numpy as np
import pytest

import rpc_amd
from rpc_amd import _lib

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address


def carry(stream=P, stream_bytes=64, conn_off=P, conn_len=P, consumed=P, state=P, nconn=4, nxt=P, next_bytes=4096,
          next_at=P, room=1040, new_len=P, next_off=P, next_len=P, status=P, carried=P):
    return _lib.rpc_frames_carry_device(stream, stream_bytes, conn_off, conn_len, consumed, state, nconn, nxt, next_bytes,
                                        next_at, room, new_len, next_off, next_len, status, carried, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert carry(nconn=0xFFFFFFFF) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_too_many_connections():
    assert carry(nconn=0xFFFFFFFF) == EINVAL
    assert carry(nconn=1 << 40) == EINVAL
    assert carry(nconn=(1 << 64) - 1) == EINVAL


@pytest.mark.parametrize("name", ["conn_off", "conn_len", "consumed", "next_at", "next_off", "next_len"])
def test_connections_need_their_arrays(name):
    assert carry(**{name: None}) == EINVAL
    assert carry(**{name: None}, nconn=1, state=None, new_len=None, status=None, carried=None) == EINVAL
    assert carry(**{name: None}, room=1 << 20) == EINVAL  # (either route)


def test_stream_bytes_need_stream():
    assert carry(stream=None, stream_bytes=1) == EINVAL
    assert carry(nconn=0, stream=None, stream_bytes=12) == EINVAL


def test_next_bytes_need_next():
    assert carry(nxt=None, next_bytes=1) == EINVAL
    assert carry(nconn=0, nxt=None, next_bytes=12, carried=None) == EINVAL


def test_no_connections_and_no_carried_needs_no_device():
    assert carry(nconn=0, carried=None) == OK
    assert carry(nconn=0, carried=None, stream=None, stream_bytes=0, nxt=None, next_bytes=0, conn_off=None,
                 conn_len=None, consumed=None, state=None, next_at=None, new_len=None, next_off=None, next_len=None,
                 status=None) == OK
    assert carry(nconn=0, carried=None, room=0) == OK
    assert carry(nconn=0, carried=None, room=(1 << 64) - 1) == OK


def test_binding_and_constants():
    assert "rpc_frames_carry_device" in _lib.EXPORTS
    assert (rpc_amd.CARRY_OK, rpc_amd.CARRY_CLOSED, rpc_amd.CARRY_INVALID, rpc_amd.CARRY_NO_ROOM) == (0, 1, 2, 3)
    assert rpc_amd.CARRY_ROOM == 1040 >= rpc_amd.RPC_HEADER_LEN + rpc_amd.MAX_BODY_LEN - 1


def test_carry_slots():
    """room bytes in front of every connection's new bytes, starts aligned, back to back."""
    at, total = rpc_amd.carry_slots([5, 0, 61, 1])
    assert at.dtype == np.int64 and at.tolist() == [1040, 2096, 3136, 4240] and total == 4241
    at, total = rpc_amd.carry_slots([100, 3], room=7, align=1)
    assert at.tolist() == [7, 114] and total == 117
    at, total = rpc_amd.carry_slots([])
    assert at.size == 0 and total == 0
    with pytest.raises(ValueError):
        rpc_amd.carry_slots([-1])
