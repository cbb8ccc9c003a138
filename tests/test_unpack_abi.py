"""rpc_frames_unpack_device's argument checks, which are made before any device is
touched (include/rpccrc.h), and the n == 0 call with nothing to write: through
rpc_amd._lib, no GPU needed.  Pointers that must only be non-NULL are given a dummy
address: a call that returns RPCCRC_EINVAL never looks at them."""
from rpc_amd import _lib

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
SERVER, CLIENT, LIFT = 0x1, 0x2, 0x4


def unpack(stream=P, stream_bytes=64, offs=P, verdict=P, n=4, conn_first=None, nconn=0, flags=SERVER, nul=1, out=None,
           out_cap=0, body_offsets=None, body_lens=None, reply_types=None, versions=None, verdict_out=None,
           conn_bytes_first=None, total=None):
    return _lib.rpc_frames_unpack_device(stream, stream_bytes, offs, verdict, n, conn_first, nconn, flags, nul, out,
                                         out_cap, body_offsets, body_lens, reply_types, versions, verdict_out,
                                         conn_bytes_first, total, None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert unpack(flags=0x8) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_unknown_flag_bits():
    for flags in (SERVER | 0x8, CLIENT | 0x10, SERVER | LIFT | 0x40, -1):
        assert unpack(flags=flags) == EINVAL


def test_exactly_one_role_bit():
    for flags in (0, LIFT, SERVER | CLIENT, SERVER | CLIENT | LIFT):
        assert unpack(flags=flags) == EINVAL
        assert unpack(n=0, flags=flags) == EINVAL


def test_nul_is_0_or_1():
    for nul in (2, -1, 256):
        assert unpack(nul=nul) == EINVAL
        assert unpack(n=0, nul=nul) == EINVAL


def test_too_many_entries():
    assert unpack(n=0xFFFFFFFF) == EINVAL
    assert unpack(n=1 << 40) == EINVAL


def test_entries_need_offsets_and_verdicts():
    assert unpack(offs=None) == EINVAL
    assert unpack(verdict=None) == EINVAL
    assert unpack(offs=None, verdict=None, flags=CLIENT | LIFT) == EINVAL


def test_stream_bytes_need_stream():
    assert unpack(stream=None, stream_bytes=1) == EINVAL
    assert unpack(n=0, stream=None, stream_bytes=12) == EINVAL


def test_out_cap_needs_out():
    assert unpack(out=None, out_cap=1) == EINVAL
    assert unpack(n=0, out=None, out_cap=12) == EINVAL


def test_conn_bytes_first_needs_conn_first():
    assert unpack(conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL
    assert unpack(n=0, conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL


def test_nconn_needs_conn_first():
    assert unpack(nconn=3, conn_first=None) == EINVAL
    assert unpack(n=0, nconn=1, conn_first=None) == EINVAL


def test_no_entries_and_nothing_to_write_needs_no_device():
    assert unpack(n=0) == OK
    assert unpack(n=0, stream=None, stream_bytes=0, offs=None, verdict=None, flags=CLIENT | LIFT, nul=0) == OK
    assert unpack(n=0, body_offsets=P, body_lens=P, reply_types=P, versions=P, verdict_out=P) == OK  # (n entries of each)
    assert unpack(n=0, conn_first=P, nconn=5) == OK
    assert unpack(n=0, out=P, out_cap=100) == OK


def test_binding_is_listed():
    assert "rpc_frames_unpack_device" in _lib.EXPORTS
