"""rpc_frames_pack_device's argument checks, which are made before any device is
touched (include/rpccrc.h), and the n == 0 call with nothing to write: through
rpc_amd._lib, no GPU needed.  Pointers that must only be non-NULL are given a dummy
address: a call that returns RPCCRC_EINVAL never looks at them."""
from rpc_amd import _lib

EINVAL, OK = -22, 0
P = 0x1000  # any non-NULL address
DATA, PING, PONG, NONE = 0, 1, 2, 0xFFFF


def pack(bodies=P, bodies_bytes=64, offs=P, lens=P, n=4, types=None, type_=DATA, versions=None, version=1,
         conn_first=None, nconn=0, flags=0, out=None, out_cap=0, frame_offsets=None, verdict=None, crc=None,
         conn_bytes_first=None, total=None):
    return _lib.rpc_frames_pack_device(bodies, bodies_bytes, offs, lens, n, types, type_, versions, version, conn_first,
                                       nconn, flags, out, out_cap, frame_offsets, verdict, crc, conn_bytes_first, total,
                                       None)


def test_einval_is_rpccrc_einval():
    assert _lib.rpc_crc32_strerror(EINVAL).decode() != _lib.rpc_crc32_strerror(OK).decode()
    assert pack(flags=0x8) == EINVAL  # (the code these tests expect is the library's EINVAL)


def test_unknown_flag_bits():
    for flags in (0x8, 0x10, 0x4 | 0x40, -1):
        assert pack(flags=flags) == EINVAL


def test_too_many_entries():
    assert pack(n=0xFFFFFFFF) == EINVAL
    assert pack(n=1 << 40) == EINVAL


def test_data_entries_need_offsets_and_lengths():
    assert pack(offs=None) == EINVAL
    assert pack(lens=None) == EINVAL
    assert pack(offs=None, lens=None, type_=7) == EINVAL
    # a per-entry type array may hold data frames, whatever the scalar says
    assert pack(offs=None, lens=None, types=P, type_=PING) == EINVAL
    assert pack(offs=None, lens=None, types=P, type_=NONE) == EINVAL


def test_out_cap_needs_out():
    assert pack(out=None, out_cap=1) == EINVAL
    assert pack(offs=None, lens=None, type_=PING, out=None, out_cap=12) == EINVAL


def test_conn_bytes_first_needs_conn_first():
    assert pack(conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL
    assert pack(n=0, conn_bytes_first=P, conn_first=None, nconn=0) == EINVAL


def test_nconn_needs_conn_first():
    assert pack(nconn=3, conn_first=None) == EINVAL
    assert pack(n=0, nconn=1, conn_first=None) == EINVAL


def test_no_entries_and_nothing_to_write_needs_no_device():
    assert pack(n=0) == OK
    assert pack(n=0, bodies=None, bodies_bytes=0, offs=None, lens=None, flags=0x1 | 0x2 | 0x4) == OK
    assert pack(n=0, frame_offsets=P, verdict=P, crc=P) == OK  # (n entries of each: nothing to write)
    assert pack(n=0, conn_first=P, nconn=5) == OK


def test_binding_is_listed():
    assert "rpc_frames_pack_device" in _lib.EXPORTS
