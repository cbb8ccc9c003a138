"""What every device-buffer wrapper hands to its C entry point: the real wrappers, CPU tensors and
a recording stand-in for the entry (the wrappers look it up on rpc_amd._lib at call time), no GPU
needed.  The stand-in records its positional arguments; every pointer is then replaced by the name
of the tensor it is -- an input of the test, ``>field`` of what the wrapper returned, ``total`` /
``nframes`` for the word the entry reports through -- and the list is compared with a tuple written
by hand from the parameter lists of include/rpccrc.h.  Two same-typed pointers in the wrong order,
a wrong NULL, a byte count that ignores an empty buffer: each shows as a differing tuple.

torch gives every tensor without elements the address 0.  ``nil(dtype)`` stands in for an empty
input that still has an address of its own, so an argument that goes through the "empty means NULL
and byte count 0" rule reads None and one that is passed as a raw ``data_ptr()`` reads its name.  A
tensor the wrapper allocated without elements, passed raw, reads 0.

Every ``raise ValueError`` of the section is asked for once with its exact message, and the entry
must not have been called; ``*_two_faults`` pin which of two faults is reported."""
import ctypes
import types

import numpy as np
import pytest
import torch

import rpc_amd
from rpc_amd import _lib

SH, CUR = 0x5150, 0xC0DE  # the handle of a given stream and of "torch's current stream"
S = types.SimpleNamespace(cuda_stream=SH)
u8, i16, i32, i64 = torch.uint8, torch.int16, torch.int32, torch.int64
BY_SIZE = {1: u8, 2: i16, 4: i32, 8: i64}
N, NCONN = 3, 2


def z(n, dtype):
    return torch.zeros(n, dtype=dtype)


class nil:
    """An empty input: what the wrappers ask of a tensor, no elements, an address of its own."""
    last, _base = [0x7000], None

    def __init__(self, dtype):
        self.dtype, self.shape, self.device = dtype, (0,), torch.device("cpu")
        nil.last[0] += 0x100
        self.at = nil.last[0]

    def numel(self):
        return 0

    def element_size(self):
        return torch.empty(0, dtype=self.dtype).element_size()

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.at


class Fake:
    """Stands in for the C entries ``entries``; with ``word_at`` it writes ``words[k]`` (the last
    one again after that) through argument ``word_at`` of call k, as the entry reports its total."""

    def __init__(self, monkeypatch, entries, word_at=None, words=(), word="total", peek=None):
        self.calls, self.named = [], {}
        self.word_at, self.words, self.word, self.peek = word_at, list(words), word, peek
        for e in [entries] if isinstance(entries, str) else entries:
            monkeypatch.setattr(_lib, e, lambda *a, _e=e: self.call(_e, a))

    def call(self, entry, a):
        if self.word_at is not None:
            self.named[a[self.word_at]] = self.word
            if self.words:
                ctypes.c_int64.from_address(a[self.word_at]).value = self.words[min(len(self.calls), len(self.words) - 1)]
        self.calls.append((entry,) + (tuple(a) if self.peek is None else self.peek(a)))
        return 0

    def seen(self, inputs, result, fields=None):
        """The recorded calls with every pointer replaced by its tensor's name."""
        names = {}

        def add(name, x):
            if isinstance(x, (torch.Tensor, nil)):
                at = x.data_ptr() or (x._base is not None and x._base.data_ptr())  # ([:0] of a tensor: the tensor's)
                if at:
                    names[at] = name
            elif isinstance(x, tuple) and hasattr(x, "_fields"):
                for f, y in zip(x._fields, x):
                    add(f"{name}.{f}", y)

        if fields is None:
            fields = result._fields
        for f, x in zip(fields, result if isinstance(result, tuple) else (result,)):
            add(">" + f, x)
        names.update(self.named)
        for k, x in inputs.items():
            add(k, x)
        return [tuple(names.get(v, v) if type(v) is int else v for v in c) for c in self.calls]


def form(result, fields=None):
    """{field: (dtype, shape)} of a result's tensors; anything else as it is."""
    if fields is None:
        fields = result._fields
    return {f: (x.dtype, tuple(x.shape)) if isinstance(x, (torch.Tensor, nil)) else x
            for f, x in zip(fields, result if isinstance(result, tuple) else (result,))}


@pytest.fixture
def current(monkeypatch):
    """stream=None is torch's current stream: one whose handle is CUR."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: types.SimpleNamespace(cuda_stream=CUR))


def refuses(monkeypatch, entries, message, fn, *a, **kw):
    fake = Fake(monkeypatch, entries)
    with pytest.raises(ValueError) as e:
        fn(*a, **kw, stream=S)
    assert str(e.value) == message
    assert fake.calls == []


def bad_tensors(size, n=N):
    """The three ways an n-element tensor of ``size``-byte elements can be wrong."""
    return (z(n, BY_SIZE[4 if size == 8 else 8]), z(n + 1, BY_SIZE[size]), z(2 * n, BY_SIZE[size])[::2])


def refuses_each(monkeypatch, entries, fn, good, entries_of, count="n", n=N, gives_n=None):
    for name, size in entries_of:
        for bad in bad_tensors(size, n)[::2 if name == gives_n else 1]:  # (the tensor that gives n has n elements)
            kw = dict(good())
            if "." in name:  # a field of a NamedTuple argument
                arg, field = name.split(".")
                kw[arg] = kw[arg]._replace(**{field: bad})
            else:
                kw[name] = bad
            refuses(monkeypatch, entries, f"{name} must be a contiguous {size}-byte tensor with {count} = {n} elements",
                    fn, **kw)


NONCONTIG = z(32, u8)[::2]
OUT4 = "out must be a contiguous 4-byte tensor with >= n elements"
CONN_FIRST = "conn_first needs nconn + 1 8-byte entries"
OUT1 = "out must be a contiguous uint8 tensor"
TABLE = "table.offsets needs nmethods + 1 4-byte entries"
SCHEMA = "schema needs nmethods + 1 4-byte CSR words, nparams types and nparams + 1 4-byte name words"
ROLE = "role must be 'server' (PING is control) or 'client' (PONG is control)"


def table():
    return rpc_amd.RouteTable(z(6, u8), z(3, i32), 2)


def schema():
    return rpc_amd.ArgsSchema(z(3, i32), z(3, u8), z(4, i32), z(5, u8), 2, 3, 2)


# ---- device_batch / device_uniform / device_large / device_gather ---------------------------

def batch_in():
    return dict(base=z(16, u8), offsets=z(N, i64), lengths=z(N, i32))


def test_device_batch(monkeypatch, current):
    E = "rpc_crc32_device_batch_bounded"
    kw = dict(batch_in(), out=z(N, i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_batch(**kw, stream=S, max_len=1000)
    assert r is kw["out"]
    assert fake.seen(kw, r, ["out"]) == [(E, "base", "offsets", "lengths", 3, 1000, "out", SH)]
    kw = batch_in()
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_batch(**kw, max_len=-1)
    assert fake.seen(kw, r, ["out"]) == [(E, "base", "offsets", "lengths", 3, 0xFFFFFFFF, ">out", CUR)]
    assert form(r, ["out"]) == {"out": (i32, (3,))}
    kw = dict(base=nil(u8), offsets=nil(i64), lengths=nil(i32))  # (all raw; the empty out is address 0)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_batch(**kw, stream=S)
    assert fake.seen(kw, r, ["out"]) == [(E, "base", "offsets", "lengths", 0, 0, 0, SH)]
    assert form(r, ["out"]) == {"out": (i32, (0,))}


def test_device_batch_older_library(monkeypatch):
    E = "rpc_crc32_device_batch"
    monkeypatch.setattr(_lib, "rpc_crc32_device_batch_bounded", None)
    kw = dict(batch_in(), out=z(N + 2, i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_batch(**kw, stream=S, max_len=1000)
    assert r is kw["out"]
    assert fake.seen(kw, r, ["out"]) == [(E, "base", "offsets", "lengths", 3, "out", SH)]


def test_device_batch_refuses(monkeypatch):
    E = ["rpc_crc32_device_batch_bounded", "rpc_crc32_device_batch"]
    refuses(monkeypatch, E, "offsets and lengths differ in length", rpc_amd.device_batch, **dict(batch_in(), lengths=z(2, i32)))
    for bad in (z(2, i32), z(N, i64), z(2 * N, i32)[::2]):
        refuses(monkeypatch, E, OUT4, rpc_amd.device_batch, **batch_in(), out=bad)
    refuses(monkeypatch, E, "offsets and lengths differ in length", rpc_amd.device_batch,  # two faults
            **dict(batch_in(), lengths=z(2, i32)), out=z(N, i64))


def test_device_uniform(monkeypatch, current):
    E = "rpc_crc32_device_uniform"
    kw = dict(base=z(16, u8), out=z(N, i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_uniform(n=3, body_len=4, stride=5, **kw, stream=S)
    assert r is kw["out"]
    assert fake.seen(kw, r, ["out"]) == [(E, "base", 3, 4, 5, "out", SH)]
    kw = dict(base=z(4, i32))  # (bytes, not elements, bound the bodies)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_uniform(kw["base"], 4, 4)
    assert fake.seen(kw, r, ["out"]) == [(E, "base", 4, 4, 4, ">out", CUR)]
    assert form(r, ["out"]) == {"out": (i32, (4,))}
    kw = dict(base=nil(u8))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_uniform(kw["base"], 0, 4, stream=S)
    assert fake.seen(kw, r, ["out"]) == [(E, "base", 0, 4, 4, 0, SH)]


def test_device_uniform_refuses(monkeypatch):
    E = "rpc_crc32_device_uniform"
    refuses(monkeypatch, E, "bodies exceed the base tensor", rpc_amd.device_uniform, z(16, u8), 3, 4, 7)
    refuses(monkeypatch, E, OUT4, rpc_amd.device_uniform, z(16, u8), 3, 4, out=z(2, i32))
    refuses(monkeypatch, E, "bodies exceed the base tensor", rpc_amd.device_uniform, z(16, u8), 3, 4, 7, out=z(2, i32))


def test_device_large(monkeypatch, current):
    E = "rpc_crc32_device_large"

    def peek(a):  # (the offsets and lengths are host arrays that live as long as the call)
        host = [np.ctypeslib.as_array((ctypes.c_uint64 * a[3]).from_address(p)).tolist() if a[3] else [] for p in a[1:3]]
        return (a[0], *host, *a[3:])

    kw = dict(base=z(16, u8), out=z(N, i32))
    fake = Fake(monkeypatch, E, peek=peek)
    r = rpc_amd.device_large(kw["base"], [0, 4, 8], iter([4, 3, 2]), chunk=32, out=kw["out"], stream=S)
    assert r is kw["out"]
    assert fake.seen(kw, r, ["out"]) == [(E, "base", [0, 4, 8], [4, 3, 2], 3, "out", 32, SH)]
    kw = dict(base=z(16, u8))
    fake = Fake(monkeypatch, E, peek=peek)
    r = rpc_amd.device_large(kw["base"], (1,), (2,))
    assert fake.seen(kw, r, ["out"]) == [(E, "base", [1], [2], 1, ">out", 0, CUR)]
    assert form(r, ["out"]) == {"out": (i32, (1,))}
    kw = dict(base=nil(u8))
    fake = Fake(monkeypatch, E, peek=peek)
    r = rpc_amd.device_large(kw["base"], [], [], stream=S)
    assert fake.seen(kw, r, ["out"]) == [(E, "base", [], [], 0, 0, 0, SH)]
    refuses(monkeypatch, E, OUT4, rpc_amd.device_large, z(16, u8), [0, 4], [4, 4], out=z(1, i32))


def gather_in():
    return dict(base=z(16, u8), seg_offsets=z(4, i64), seg_lengths=z(4, i32), seg_first=z(N + 1, i64))


def test_device_gather(monkeypatch, current):
    E = "rpc_crc32_device_gather"
    kw = dict(gather_in(), seed=z(N, i32), out=z(N, i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_gather(**kw, stream=S, max_seg_len=-1)
    assert r is kw["out"]
    assert fake.seen(kw, r, ["out"]) == [(E, "base", "seg_offsets", "seg_lengths", 4, 0xFFFFFFFF, "seg_first", 3, "seed",
                                          "out", SH)]
    kw = dict(base=None, seg_offsets=None, seg_lengths=None, seg_first=z(N + 1, i64))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_gather(**kw)
    assert fake.seen(kw, r, ["out"]) == [(E, None, None, None, 0, 0, "seg_first", 3, None, ">out", CUR)]
    assert form(r, ["out"]) == {"out": (i32, (3,))}
    # empty is not None here: every pointer is passed raw
    kw = dict(base=nil(u8), seg_offsets=nil(i64), seg_lengths=nil(i32), seg_first=z(1, i64), seed=nil(i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.device_gather(**kw, stream=S)
    assert fake.seen(kw, r, ["out"]) == [(E, "base", "seg_offsets", "seg_lengths", 0, 0, "seg_first", 0, "seed", 0, SH)]


def test_device_gather_refuses(monkeypatch):
    E, g = "rpc_crc32_device_gather", rpc_amd.device_gather
    refuses(monkeypatch, E, "seg_first needs n + 1 entries", g, **dict(gather_in(), seg_first=nil(i64)))
    refuses(monkeypatch, E, "seg_offsets and seg_lengths differ in length", g, **dict(gather_in(), seg_lengths=z(3, i32)))
    refuses(monkeypatch, E, "seg_offsets and seg_lengths differ in length", g, **dict(gather_in(), seg_lengths=None))
    refuses(monkeypatch, E, "segments need a base tensor", g, **dict(gather_in(), base=None))
    for bad in (z(2, i32), z(N, i64), z(2 * N, i32)[::2]):
        refuses(monkeypatch, E, "seed must be a contiguous 4-byte tensor with >= n elements", g, **gather_in(), seed=bad)
    refuses(monkeypatch, E, OUT4, g, **gather_in(), out=z(N, i16))
    refuses(monkeypatch, E, "seg_offsets and seg_lengths differ in length", g,  # two faults
            **dict(gather_in(), seg_lengths=z(3, i32), base=None))
    refuses(monkeypatch, E, "seed must be a contiguous 4-byte tensor with >= n elements", g, **gather_in(), seed=z(2, i32),
            out=z(N, i16))


# ---- frames_verify / frames_stamp -------------------------------------------------------------

def test_frames_verify(monkeypatch, current):
    E, F = "rpc_frames_verify_device", ["verdict", "crc"]
    kw = dict(stream_buf=z(16, u8), frame_offsets=z(N, i64), crc_out=z(N, i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_verify(**kw, role="client", lift_cap=True, stream_bytes=10, stream=S)
    assert r[1] is kw["crc_out"]
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 10, "frame_offsets", 3, 0x2 | 0x4, ">verdict", "crc_out", SH)]
    assert form(r, F) == {"verdict": (u8, (3,)), "crc": (i32, (3,))}
    kw = dict(stream_buf=z(4, i32), frame_offsets=z(N, i64))  # (the stream's size in bytes)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_verify(**kw)
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 16, "frame_offsets", 3, 0x1, ">verdict", ">crc", CUR)]
    assert form(r, F) == {"verdict": (u8, (3,)), "crc": (i32, (3,))}
    kw = dict(stream_buf=nil(u8), frame_offsets=nil(i64))  # (raw, and stream_bytes as given)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_verify(**kw, stream_bytes=7, stream=S)
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 7, "frame_offsets", 0, 0x1, 0, 0, SH)]
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_verify(**kw, stream=S)
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 0, "frame_offsets", 0, 0x1, 0, 0, SH)]


def test_frames_verify_refuses(monkeypatch):
    E, kw = "rpc_frames_verify_device", dict(stream_buf=z(16, u8), frame_offsets=z(N, i64))
    refuses(monkeypatch, E, ROLE, rpc_amd.frames_verify, **kw, role="peer")
    refuses(monkeypatch, E, OUT4, rpc_amd.frames_verify, **kw, crc_out=z(2, i32))
    refuses(monkeypatch, E, OUT4, rpc_amd.frames_verify, **kw, role="peer", crc_out=z(2, i32))  # two faults


def test_frames_stamp(monkeypatch, current):
    E, F = "rpc_frames_stamp_device", ["verdict"]
    kw = dict(stream_buf=z(16, u8), frame_offsets=z(N, i64), body_lens=z(N, i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_stamp(**kw, version=2, type_=1, lift_cap=True, stream_bytes=12, stream=S)
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 12, "frame_offsets", "body_lens", 3, 2, 1, 0x4, ">verdict", SH)]
    assert form(r, F) == {"verdict": (u8, (3,))}
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_stamp(**kw)
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 16, "frame_offsets", "body_lens", 3, 1, 0, 0, ">verdict", CUR)]
    kw = dict(stream_buf=nil(u8), frame_offsets=nil(i64), body_lens=nil(i32))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_stamp(**kw, stream_bytes=7, stream=S)
    assert fake.seen(kw, r, F) == [(E, "stream_buf", 7, "frame_offsets", "body_lens", 0, 1, 0, 0, 0, SH)]
    assert form(r, F) == {"verdict": (u8, (0,))}


# ---- frames_pack ----------------------------------------------------------------------------------

def pack_in():
    return dict(bodies=z(16, u8), body_offsets=z(N, i64), body_lens=z(N, i32), types=z(N, i16), versions=z(N, i16),
                conn_first=z(NCONN + 1, i64))


def test_frames_pack_with_out(monkeypatch):
    E = "rpc_frames_pack_device"
    kw = dict(pack_in(), out=z(16, u8))
    fake = Fake(monkeypatch, E, word_at=18)
    r = rpc_amd.frames_pack(**kw, version=0x10002, type_=0x10001, lift_cap=True, stream=S)
    assert r.stream is kw["out"]
    assert fake.seen(kw, r) == [(E, "bodies", 16, "body_offsets", "body_lens", 3, "types", 1, "versions", 2, "conn_first", 2,
                                 0x4, "out", 16, ">offsets", ">verdict", ">crc", ">conn_bytes_first", "total", SH)]
    assert form(r) == {"stream": (u8, (16,)), "offsets": (i64, (3,)), "verdict": (u8, (3,)), "crc": (i32, (3,)),
                       "conn_bytes_first": (i64, (3,)), "total": (i64, (1,))}


def test_frames_pack_sizes_itself(monkeypatch, current):
    E = "rpc_frames_pack_device"
    kw = dict(bodies=None, body_offsets=z(N, i64), body_lens=None)
    fake = Fake(monkeypatch, E, word_at=18, words=[5])
    r = rpc_amd.frames_pack(**kw)
    head = (E, None, 0, "body_offsets", None, 3, None, 0, None, 1, None, 0, 0)
    assert fake.seen(kw, r) == [head + (None, 0, None, None, None, None, "total", CUR),
                                head + (">stream", 5, ">offsets", ">verdict", ">crc", None, "total", CUR)]
    assert form(r) == {"stream": (u8, (5,)), "offsets": (i64, (3,)), "verdict": (u8, (3,)), "crc": (i32, (3,)),
                       "conn_bytes_first": None, "total": 5}
    assert type(r.total) is int
    kw = dict(bodies=None, body_offsets=None, body_lens=None, types=z(N, i16))  # (n from types; a total of 0)
    fake = Fake(monkeypatch, E, word_at=18, words=[0])
    r = rpc_amd.frames_pack(**kw)
    head = (E, None, 0, None, None, 3, "types", 0, None, 1, None, 0, 0)
    assert fake.seen(kw, r) == [head + (None, 0, None, None, None, None, "total", CUR),
                                head + (None, 0, ">offsets", ">verdict", ">crc", None, "total", CUR)]
    assert form(r)["stream"] == (u8, (0,)) and r.total == 0


def test_frames_pack_empty(monkeypatch):
    E = "rpc_frames_pack_device"
    kw = dict(bodies=nil(u8), body_offsets=nil(i64), body_lens=nil(i32), types=nil(i16), versions=nil(i16),
              conn_first=z(1, i64), out=nil(u8))
    fake = Fake(monkeypatch, E, word_at=18)
    r = rpc_amd.frames_pack(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, None, 0, None, None, 0, None, 0, None, 1, "conn_first", 0, 0, None, 0, None, None, None,
                                 ">conn_bytes_first", "total", SH)]
    assert form(r) == {"stream": (u8, (0,)), "offsets": (i64, (0,)), "verdict": (u8, (0,)), "crc": (i32, (0,)),
                       "conn_bytes_first": (i64, (1,)), "total": (i64, (1,))}


def test_frames_pack_refuses(monkeypatch):
    E, f = "rpc_frames_pack_device", rpc_amd.frames_pack
    refuses(monkeypatch, E, "the number of entries comes from body_offsets or types", f, z(16, u8), None, z(N, i32))
    refuses_each(monkeypatch, E, f, pack_in, [("body_lens", 4), ("types", 2), ("versions", 2), ("body_offsets", 8)],
                 gives_n="body_offsets")
    for bad in (nil(i64), z(NCONN + 1, i32)):
        refuses(monkeypatch, E, CONN_FIRST, f, **dict(pack_in(), conn_first=bad))
    for bad in (NONCONTIG, z(16, i16)):
        refuses(monkeypatch, E, OUT1, f, **pack_in(), out=bad)
    # two faults: the tensors in the order body_lens, types, versions, body_offsets, then conn_first, then out
    refuses(monkeypatch, E, "body_lens must be a contiguous 4-byte tensor with n = 3 elements", f,
            **dict(pack_in(), body_offsets=z(N, i32), body_lens=z(N, i64)))
    refuses(monkeypatch, E, "versions must be a contiguous 2-byte tensor with n = 3 elements", f,
            **dict(pack_in(), versions=z(N, i32), conn_first=nil(i64)))
    refuses(monkeypatch, E, CONN_FIRST, f, **dict(pack_in(), conn_first=nil(i64)), out=NONCONTIG)


# ---- frames_unpack --------------------------------------------------------------------------------

def unpack_in():
    return dict(stream_buf=z(16, u8), frame_offsets=z(N, i64), verdict=z(N, u8))


UNPACK_FORM = {"bodies": (u8, (16,)), "body_offsets": (i64, (3,)), "body_lens": (i32, (3,)), "reply_types": (i16, (3,)),
               "versions": (i16, (3,)), "verdict": (u8, (3,)), "conn_bytes_first": (i64, (3,)), "total": (i64, (1,))}


def test_frames_unpack_with_out(monkeypatch):
    E = "rpc_frames_unpack_device"
    kw = dict(unpack_in(), conn_first=z(NCONN + 1, i64), out=z(16, u8))
    fake = Fake(monkeypatch, E, word_at=17)
    r = rpc_amd.frames_unpack(**kw, role="client", lift_cap=True, nul=False, stream_bytes=12, stream=S)
    assert r.bodies is kw["out"]
    assert fake.seen(kw, r) == [(E, "stream_buf", 12, "frame_offsets", "verdict", 3, "conn_first", 2, 0x2 | 0x4, 0, "out", 16,
                                 ">body_offsets", ">body_lens", ">reply_types", ">versions", ">verdict",
                                 ">conn_bytes_first", "total", SH)]
    assert form(r) == UNPACK_FORM


def test_frames_unpack_sizes_itself(monkeypatch, current):
    E = "rpc_frames_unpack_device"
    kw = unpack_in()
    fake = Fake(monkeypatch, E, word_at=17, words=[5])
    r = rpc_amd.frames_unpack(**kw)
    head = (E, "stream_buf", 16, "frame_offsets", "verdict", 3, None, 0, 0x1, 1)
    assert fake.seen(kw, r) == [head + (None, 0, None, None, None, None, None, None, "total", CUR),
                                head + (">bodies", 5, ">body_offsets", ">body_lens", ">reply_types", ">versions", ">verdict",
                                        None, "total", CUR)]
    assert form(r) == dict(UNPACK_FORM, bodies=(u8, (5,)), conn_bytes_first=None, total=5)
    assert type(r.total) is int


def test_frames_unpack_empty(monkeypatch):
    E = "rpc_frames_unpack_device"
    kw = dict(stream_buf=nil(u8), frame_offsets=nil(i64), verdict=nil(u8), conn_first=z(1, i64), out=nil(u8))
    fake = Fake(monkeypatch, E, word_at=17)
    r = rpc_amd.frames_unpack(**kw, stream_bytes=12, stream=S)  # (no buffer: stream_bytes reads 0 whatever was given)
    assert fake.seen(kw, r) == [(E, None, 0, None, None, 0, "conn_first", 0, 0x1, 1, None, 0, None, None, None, None, None,
                                 ">conn_bytes_first", "total", SH)]
    assert form(r)["body_offsets"] == (i64, (0,)) and form(r)["conn_bytes_first"] == (i64, (1,))


def test_frames_unpack_refuses(monkeypatch):
    E, f = "rpc_frames_unpack_device", rpc_amd.frames_unpack
    refuses_each(monkeypatch, E, f, unpack_in, [("frame_offsets", 8), ("verdict", 1)], gives_n="frame_offsets")
    refuses(monkeypatch, E, CONN_FIRST, f, **unpack_in(), conn_first=z(NCONN + 1, i32))
    refuses(monkeypatch, E, OUT1, f, **unpack_in(), out=NONCONTIG)
    refuses(monkeypatch, E, ROLE, f, **unpack_in(), role="peer")
    refuses(monkeypatch, E, CONN_FIRST, f, **unpack_in(), conn_first=nil(i64), out=NONCONTIG)  # two faults
    refuses(monkeypatch, E, OUT1, f, **unpack_in(), out=z(4, i32), role="peer")  # (the role is looked at last)


# ---- frames_carry ---------------------------------------------------------------------------------

def carry_in():
    return dict(stream_buf=z(16, u8), conn_offsets=z(NCONN, i64), conn_lengths=z(NCONN, i64), consumed=z(NCONN, i64),
                state=z(NCONN, u8), next_buf=z(24, u8), next_at=z(NCONN, i64), new_lengths=z(NCONN, i64))


def test_frames_carry(monkeypatch, current):
    E = "rpc_frames_carry_device"
    kw = carry_in()
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_carry(**kw, room=48, stream=S)
    assert fake.seen(kw, r) == [(E, "stream_buf", 16, "conn_offsets", "conn_lengths", "consumed", "state", 2, "next_buf", 24,
                                 "next_at", 48, "new_lengths", ">next_offsets", ">next_lengths", ">status", ">carried", SH)]
    assert form(r) == {"next_offsets": (i64, (2,)), "next_lengths": (i64, (2,)), "status": (u8, (2,)),
                       "carried": (i64, (1,))}
    kw = dict(carry_in(), state=None, new_lengths=None)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_carry(**kw)
    assert fake.seen(kw, r) == [(E, "stream_buf", 16, "conn_offsets", "conn_lengths", "consumed", None, 2, "next_buf", 24,
                                 "next_at", 1040, None, ">next_offsets", ">next_lengths", ">status", ">carried", CUR)]
    kw = dict(stream_buf=nil(u8), conn_offsets=nil(i64), conn_lengths=nil(i64), consumed=nil(i64), state=nil(u8),
              next_buf=nil(u8), next_at=nil(i64), new_lengths=nil(i64))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_carry(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, None, 0, None, None, None, None, 0, None, 0, None, 1040, None, None, None, None,
                                 ">carried", SH)]
    assert form(r)["status"] == (u8, (0,)) and form(r)["carried"] == (i64, (1,))


def test_frames_carry_refuses(monkeypatch):
    E, f = "rpc_frames_carry_device", rpc_amd.frames_carry
    refuses_each(monkeypatch, E, f, carry_in, [("conn_lengths", 8), ("consumed", 8), ("state", 1), ("next_at", 8),
                                               ("new_lengths", 8)], count="nconn", n=NCONN)
    # (conn_offsets gives nconn, so its count is never wrong)
    for bad in (z(NCONN, i32), z(2 * NCONN, i64)[::2]):
        refuses(monkeypatch, E, "conn_offsets must be a contiguous 8-byte tensor with nconn = 2 elements", f,
                **dict(carry_in(), conn_offsets=bad))
    for name in ("stream_buf", "next_buf"):
        for bad in (NONCONTIG, z(16, i16)):
            refuses(monkeypatch, E, f"{name} must be a contiguous uint8 tensor", f, **dict(carry_in(), **{name: bad}))
    refuses(monkeypatch, E, "room must not be negative", f, **carry_in(), room=-1)
    # two faults: the index tensors, then stream_buf, then next_buf, then room
    refuses(monkeypatch, E, "next_at must be a contiguous 8-byte tensor with nconn = 2 elements", f,
            **dict(carry_in(), next_at=z(NCONN, i32), stream_buf=NONCONTIG))
    refuses(monkeypatch, E, "stream_buf must be a contiguous uint8 tensor", f,
            **dict(carry_in(), next_buf=NONCONTIG, stream_buf=NONCONTIG))
    refuses(monkeypatch, E, "next_buf must be a contiguous uint8 tensor", f, **dict(carry_in(), next_buf=NONCONTIG), room=-1)


def test_carry_slots_refuses():
    for kw in (dict(new_lengths=[[1]]), dict(new_lengths=[1, -1]), dict(new_lengths=[1], room=-1),
               dict(new_lengths=[1], align=0)):
        with pytest.raises(ValueError) as e:
            rpc_amd.carry_slots(**kw)
        assert str(e.value) == "new_lengths must be a list of non-negative lengths, room >= 0, align >= 1"


# ---- frames_route ---------------------------------------------------------------------------------

def route_in():
    return dict(bodies=z(16, u8), body_offsets=z(N, i64), body_lens=z(N, i32), table=table(), reply_types=z(N, i16))


def test_frames_route(monkeypatch, current):
    E = "rpc_frames_route_device"
    kw = route_in()
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_route(**kw, stream=S)
    head = (E, "bodies", 16, "body_offsets", "body_lens", "reply_types", 3, "table.names", 6, "table.offsets", 2)
    outs = (">kind", ">method", ">id", ">params_off", ">params_len")
    assert fake.seen(kw, r) == [head + outs + (">order", ">group_first", SH)]
    assert form(r) == {"kind": (u8, (3,)), "method": (i16, (3,)), "id": (i32, (3,)), "params_off": (i32, (3,)),
                       "params_len": (i32, (3,)), "order": (i32, (3,)), "group_first": (i32, (6,))}
    kw = dict(route_in(), reply_types=None)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_route(**kw, group=False)
    assert fake.seen(kw, r) == [(E, "bodies", 16, "body_offsets", "body_lens", None, 3, "table.names", 6, "table.offsets", 2)
                                + outs + (None, None, CUR)]
    assert r.order is None and r.group_first is None


def test_frames_route_empty(monkeypatch):
    E = "rpc_frames_route_device"
    kw = dict(bodies=nil(u8), body_offsets=nil(i64), body_lens=nil(i32), reply_types=nil(i16),
              table=rpc_amd.RouteTable(nil(u8), z(1, i32), 0))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_route(**kw, stream=S)  # (order is one element long, so never NULL, and comes back as [:0])
    assert fake.seen(kw, r) == [(E, None, 0, None, None, None, 0, None, 0, "table.offsets", 0, None, None, None, None, None,
                                 ">order", ">group_first", SH)]
    assert form(r) == {"kind": (u8, (0,)), "method": (i16, (0,)), "id": (i32, (0,)), "params_off": (i32, (0,)),
                       "params_len": (i32, (0,)), "order": (i32, (0,)), "group_first": (i32, (4,))}


def test_frames_route_refuses(monkeypatch):
    E, f = "rpc_frames_route_device", rpc_amd.frames_route
    refuses_each(monkeypatch, E, f, route_in, [("body_lens", 4), ("reply_types", 2)])
    refuses(monkeypatch, E, "body_offsets must be a contiguous 8-byte tensor with n = 3 elements", f,
            **dict(route_in(), body_offsets=z(N, i32)))
    for bad in (NONCONTIG, z(16, i16)):
        refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f, **dict(route_in(), bodies=bad))
    for bad in (rpc_amd.RouteTable(z(6, u8), z(2, i32), 2), rpc_amd.RouteTable(z(6, u8), z(3, i64), 2)):
        refuses(monkeypatch, E, TABLE, f, **dict(route_in(), table=bad))
    refuses(monkeypatch, E, "reply_types must be a contiguous 2-byte tensor with n = 3 elements", f,  # two faults
            **dict(route_in(), reply_types=z(N, i32), bodies=NONCONTIG))
    refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f,
            **dict(route_in(), bodies=NONCONTIG, table=rpc_amd.RouteTable(z(6, u8), z(2, i32), 2)))


def test_table_builders_refuse():
    with pytest.raises(ValueError) as e:
        rpc_amd.route_table(["m"] * 257, device="cpu")
    assert str(e.value) == "at most 256 names and 4096 bytes of names"
    with pytest.raises(ValueError) as e:
        rpc_amd.route_table(["m" * 4097], device="cpu")
    assert str(e.value) == "at most 256 names and 4096 bytes of names"
    with pytest.raises(ValueError) as e:
        rpc_amd.args_schema([("m", [("p", "i32")] * 9)], device="cpu")
    assert str(e.value) == "at most 8 parameters per method"
    for methods in ([("m", [])] * 257, [("m", [("p", "i32")] * 8)] * 129, [("m", [("p" * 600, "i32")] * 7)]):
        with pytest.raises(ValueError) as e:
            rpc_amd.args_schema(methods, device="cpu")
        assert str(e.value) == "at most 256 methods, 1024 parameters and 4096 bytes of names"
    with pytest.raises(ValueError) as e:
        rpc_amd.result_types(["a", "b"], ["i32"], device="cpu")
    assert str(e.value) == "one result type per method"
    with pytest.raises(ValueError) as e:
        rpc_amd.result_types(["m"] * 257, ["i32"] * 257, device="cpu")
    assert str(e.value) == "at most 256 methods"


def test_table_builders_on_the_host():
    t = rpc_amd.route_table(["add", b"echo"], device="cpu")
    assert bytes(t.names.tolist()) == b"addecho" and t.offsets.tolist() == [0, 3, 7] and t.nmethods == 2
    assert (t.names.dtype, t.offsets.dtype) == (u8, i32)
    s = rpc_amd.args_schema([("add", [("a", "i32"), ("b", rpc_amd.ARG_F64)]), ("nop", [])], device="cpu")
    assert s.first.tolist() == [0, 2, 2] and s.types.tolist() == [0, 2] and s.name_off.tolist() == [0, 1, 2]
    assert bytes(s.names.tolist()) == b"ab" and (s.nmethods, s.nparams, s.width) == (2, 2, 2)
    assert (s.first.dtype, s.types.dtype, s.name_off.dtype, s.names.dtype) == (i32, u8, i32, u8)
    r = rpc_amd.result_types(["add", "nop"], ["double", rpc_amd.ARG_STR], device="cpu")
    assert r.tolist() == [2, 4] and r.dtype == u8


# ---- frames_args ----------------------------------------------------------------------------------

def args_in():
    route = rpc_amd.FrameRoute(z(N, u8), z(N, i16), z(N, i32), z(N, i32), z(N, i32), None, None)
    return dict(bodies=z(16, u8), body_offsets=z(N, i64), body_lens=z(N, i32), route=route, schema=schema())


def args_call(width, slots=">slots", n=3, sh=SH):
    return ("rpc_frames_args_device", "bodies", 16, "body_offsets", "body_lens", "route.kind", "route.method",
            "route.params_off", "route.params_len", n, "schema.first", 2, "schema.types", "schema.name_off", 3,
            "schema.names", 5, width, slots, ">status", ">reply_status", sh)


def test_frames_args(monkeypatch, current):
    E = "rpc_frames_args_device"
    kw = args_in()
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_args(**kw, stream=S)
    assert fake.seen(kw, r) == [args_call(2)]
    assert form(r) == {"status": (u8, (3,)), "reply_status": (i32, (3,)), "slots": (i64, (2, 3))}
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_args(**kw, width=8)
    assert fake.seen(kw, r) == [args_call(8, sh=CUR)]
    assert form(r)["slots"] == (i64, (8, 3))
    for width in (0, 9):  # (the library refuses the width; there are no slot columns for it)
        fake = Fake(monkeypatch, E)
        r = rpc_amd.frames_args(**kw, width=width, stream=S)
        assert fake.seen(kw, r) == [args_call(width, slots=None)]
        assert form(r)["slots"] == (i64, (0, 3))


def test_frames_args_empty(monkeypatch):
    E = "rpc_frames_args_device"
    route = rpc_amd.FrameRoute(nil(u8), nil(i16), nil(i32), nil(i32), nil(i32), None, None)
    kw = dict(bodies=nil(u8), body_offsets=nil(i64), body_lens=nil(i32), route=route,
              schema=rpc_amd.ArgsSchema(z(1, i32), nil(u8), z(1, i32), nil(u8), 0, 0, 1))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_args(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, None, 0, None, None, None, None, None, None, 0, "schema.first", 0, None, "schema.name_off",
                                 0, None, 0, 1, None, None, None, SH)]
    assert form(r) == {"status": (u8, (0,)), "reply_status": (i32, (0,)), "slots": (i64, (1, 0))}


BAD_SCHEMAS = [lambda s: s._replace(first=z(2, i32)), lambda s: s._replace(types=z(2, u8)),
               lambda s: s._replace(name_off=z(3, i32)), lambda s: s._replace(first=z(3, i64)),
               lambda s: s._replace(types=z(3, i16)), lambda s: s._replace(name_off=z(4, i64))]


def test_frames_args_refuses(monkeypatch):
    E, f = "rpc_frames_args_device", rpc_amd.frames_args
    refuses_each(monkeypatch, E, f, args_in, [("body_lens", 4), ("route.kind", 1), ("route.method", 2),
                                              ("route.params_off", 4), ("route.params_len", 4)])
    refuses(monkeypatch, E, "body_offsets must be a contiguous 8-byte tensor with n = 3 elements", f,
            **dict(args_in(), body_offsets=z(N, i32)))
    refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f, **dict(args_in(), bodies=NONCONTIG))
    for bad in BAD_SCHEMAS:
        refuses(monkeypatch, E, SCHEMA, f, **dict(args_in(), schema=bad(schema())))
    refuses(monkeypatch, E, "route.method must be a contiguous 2-byte tensor with n = 3 elements", f,  # two faults
            **dict(args_in(), route=args_in()["route"]._replace(method=z(N, i32)), bodies=NONCONTIG))
    refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f,
            **dict(args_in(), bodies=NONCONTIG, schema=BAD_SCHEMAS[0](schema())))


# ---- frames_resolve -------------------------------------------------------------------------------

def resolve_in():
    return dict(bodies=z(16, u8), body_offsets=z(N, i64), body_lens=z(N, i32), pending_ids=z(4, i32), reply_types=z(N, i16))


RESOLVE_OUTS = (">kind", ">id", ">result_off", ">result_len", ">error_off", ">error_len", ">slot")


def test_frames_resolve(monkeypatch, current):
    E = "rpc_frames_resolve_device"
    kw = resolve_in()
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_resolve(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, "bodies", 16, "body_offsets", "body_lens", "reply_types", 3, "pending_ids", 4)
                                + RESOLVE_OUTS + (">slot_entry", ">open", ">nopen", SH)]
    assert form(r) == {"kind": (u8, (3,)), "id": (i32, (3,)), "result_off": (i32, (3,)), "result_len": (i32, (3,)),
                       "error_off": (i32, (3,)), "error_len": (i32, (3,)), "slot": (i32, (3,)), "slot_entry": (i32, (4,)),
                       "open": (i32, (4,)), "nopen": (i32, (1,))}
    kw = dict(resolve_in(), pending_ids=None, reply_types=None)  # (open is one element long, so never NULL)
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_resolve(**kw)
    assert fake.seen(kw, r) == [(E, "bodies", 16, "body_offsets", "body_lens", None, 3, None, 0)
                                + RESOLVE_OUTS + (None, ">open", ">nopen", CUR)]
    assert form(r)["slot_entry"] == (i32, (0,)) and form(r)["open"] == (i32, (0,))


def test_frames_resolve_empty(monkeypatch):
    E = "rpc_frames_resolve_device"
    kw = dict(bodies=nil(u8), body_offsets=nil(i64), body_lens=nil(i32), pending_ids=nil(i64), reply_types=nil(i16))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_resolve(**kw, stream=S)  # (no pending ids: their element size is not looked at)
    assert fake.seen(kw, r) == [(E, None, 0, None, None, None, 0, None, 0, None, None, None, None, None, None, None, None,
                                 ">open", ">nopen", SH)]
    assert form(r)["kind"] == (u8, (0,)) and form(r)["open"] == (i32, (0,)) and form(r)["nopen"] == (i32, (1,))


def test_frames_resolve_refuses(monkeypatch):
    E, f = "rpc_frames_resolve_device", rpc_amd.frames_resolve
    refuses_each(monkeypatch, E, f, resolve_in, [("body_lens", 4), ("reply_types", 2)])
    refuses(monkeypatch, E, "body_offsets must be a contiguous 8-byte tensor with n = 3 elements", f,
            **dict(resolve_in(), body_offsets=z(N, i32)))
    refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f, **dict(resolve_in(), bodies=z(16, i16)))
    for bad in (z(4, i64), z(8, i32)[::2]):
        refuses(monkeypatch, E, "pending_ids must be a contiguous 4-byte tensor", f, **dict(resolve_in(), pending_ids=bad))
    many = rpc_amd.RESOLVE_MAX_PENDING + 1
    refuses(monkeypatch, E, "at most 16777216 pending ids", f, **dict(resolve_in(), pending_ids=torch.empty(many, dtype=i32)))
    refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f,  # two faults
            **dict(resolve_in(), bodies=NONCONTIG, pending_ids=z(4, i64)))
    refuses(monkeypatch, E, "pending_ids must be a contiguous 4-byte tensor", f,
            **dict(resolve_in(), pending_ids=torch.empty(many, dtype=i16)))


# ---- frames_reply ---------------------------------------------------------------------------------

def reply_in():
    return dict(kind=z(N, u8), rid=z(N, i32), values=z(16, u8), value_offsets=z(N, i64), value_lens=z(N, i32),
                status=z(N, i32), reply_types=z(N, i16), conn_first=z(NCONN + 1, i64))


BODIES_FORM = {"bodies": (u8, (16,)), "body_offsets": (i64, (3,)), "body_lens": (i32, (3,)), "types": (i16, (3,)),
               "status": (u8, (3,)), "conn_bytes_first": (i64, (3,)), "total": (i64, (1,))}
BODIES_OUTS = (">body_offsets", ">body_lens", ">types", ">status")


def test_frames_reply_with_out(monkeypatch):
    E = "rpc_frames_reply_device"
    kw = dict(reply_in(), out=z(16, u8))
    fake = Fake(monkeypatch, E, word_at=18)
    r = rpc_amd.frames_reply(**kw, stream=S)
    assert r.bodies is kw["out"]
    assert fake.seen(kw, r) == [(E, "kind", "rid", "status", "reply_types", 3, "values", 16, "value_offsets", "value_lens",
                                 "conn_first", 2, "out", 16) + BODIES_OUTS + (">conn_bytes_first", "total", SH)]
    assert form(r) == BODIES_FORM


def test_frames_reply_sizes_itself(monkeypatch, current):
    E = "rpc_frames_reply_device"
    kw = dict(reply_in(), kind=None, status=None, reply_types=None, conn_first=None)
    fake = Fake(monkeypatch, E, word_at=18, words=[5])
    r = rpc_amd.frames_reply(**kw)
    head = (E, None, "rid", None, None, 3, "values", 16, "value_offsets", "value_lens", None, 0)
    assert fake.seen(kw, r) == [head + (None, 0, None, None, None, None, None, "total", CUR),
                                head + (">bodies", 5) + BODIES_OUTS + (None, "total", CUR)]
    assert form(r) == dict(BODIES_FORM, bodies=(u8, (5,)), conn_bytes_first=None, total=5)
    assert type(r.total) is int


def test_frames_reply_empty(monkeypatch):
    E = "rpc_frames_reply_device"
    kw = dict(kind=nil(u8), rid=nil(i32), values=nil(u8), value_offsets=nil(i64), value_lens=nil(i32), status=nil(i32),
              reply_types=nil(i16), conn_first=z(1, i64), out=nil(u8))
    fake = Fake(monkeypatch, E, word_at=18)
    r = rpc_amd.frames_reply(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, None, None, None, None, 0, None, 0, None, None, "conn_first", 0, None, 0, None, None, None,
                                 None, ">conn_bytes_first", "total", SH)]
    assert form(r)["status"] == (u8, (0,)) and form(r)["conn_bytes_first"] == (i64, (1,))


def test_frames_reply_refuses(monkeypatch):
    E, f = "rpc_frames_reply_device", rpc_amd.frames_reply
    refuses_each(monkeypatch, E, f, reply_in, [("kind", 1), ("status", 4), ("reply_types", 2), ("value_offsets", 8),
                                               ("value_lens", 4)])
    refuses(monkeypatch, E, "rid must be a contiguous 4-byte tensor with n = 3 elements", f, **dict(reply_in(), rid=z(N, i64)))
    refuses(monkeypatch, E, "values must be a contiguous uint8 tensor", f, **dict(reply_in(), values=NONCONTIG))
    refuses(monkeypatch, E, CONN_FIRST, f, **dict(reply_in(), conn_first=nil(i64)))
    refuses(monkeypatch, E, OUT1, f, **reply_in(), out=z(16, i32))
    # two faults: kind, rid, status, reply_types, value_offsets, value_lens, then values, conn_first, out
    refuses(monkeypatch, E, "status must be a contiguous 4-byte tensor with n = 3 elements", f,
            **dict(reply_in(), value_offsets=z(N, i32), status=z(N, i64)))
    refuses(monkeypatch, E, "values must be a contiguous uint8 tensor", f,
            **dict(reply_in(), values=NONCONTIG, conn_first=nil(i64)))
    refuses(monkeypatch, E, CONN_FIRST, f, **dict(reply_in(), conn_first=z(3, i32)), out=NONCONTIG)


# ---- frames_request -------------------------------------------------------------------------------

def request_in():
    return dict(method=z(N, i16), rid=z(N, i32), params=z(16, u8), params_offsets=z(N, i64), params_lens=z(N, i32),
                table=table(), types=z(N, i16), conn_first=z(NCONN + 1, i64))


def test_frames_request_with_out(monkeypatch):
    E = "rpc_frames_request_device"
    kw = dict(request_in(), out=z(16, u8))
    fake = Fake(monkeypatch, E, word_at=21)
    r = rpc_amd.frames_request(**kw, stream=S)
    assert r.bodies is kw["out"]
    assert fake.seen(kw, r) == [(E, "method", "rid", "types", 3, "table.names", 6, "table.offsets", 2, "params", 16,
                                 "params_offsets", "params_lens", "conn_first", 2, "out", 16) + BODIES_OUTS
                                + (">conn_bytes_first", "total", SH)]
    assert form(r) == BODIES_FORM


def test_frames_request_sizes_itself(monkeypatch, current):
    E = "rpc_frames_request_device"
    kw = dict(request_in(), types=None, conn_first=None)
    fake = Fake(monkeypatch, E, word_at=21, words=[5])
    r = rpc_amd.frames_request(**kw)
    head = (E, "method", "rid", None, 3, "table.names", 6, "table.offsets", 2, "params", 16, "params_offsets", "params_lens",
            None, 0)
    assert fake.seen(kw, r) == [head + (None, 0, None, None, None, None, None, "total", CUR),
                                head + (">bodies", 5) + BODIES_OUTS + (None, "total", CUR)]
    assert form(r) == dict(BODIES_FORM, bodies=(u8, (5,)), conn_bytes_first=None, total=5)
    assert type(r.total) is int


def test_frames_request_empty(monkeypatch):
    E = "rpc_frames_request_device"
    kw = dict(method=nil(i16), rid=nil(i32), params=nil(u8), params_offsets=nil(i64), params_lens=nil(i32),
              table=rpc_amd.RouteTable(nil(u8), z(1, i32), 0), types=nil(i16), conn_first=z(1, i64), out=nil(u8))
    fake = Fake(monkeypatch, E, word_at=21)
    r = rpc_amd.frames_request(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, None, None, None, 0, None, 0, "table.offsets", 0, None, 0, None, None, "conn_first", 0, None,
                                 0, None, None, None, None, ">conn_bytes_first", "total", SH)]
    assert form(r)["types"] == (i16, (0,)) and form(r)["conn_bytes_first"] == (i64, (1,))


def test_frames_request_refuses(monkeypatch):
    E, f = "rpc_frames_request_device", rpc_amd.frames_request
    refuses_each(monkeypatch, E, f, request_in, [("method", 2), ("types", 2), ("params_offsets", 8), ("params_lens", 4)])
    refuses(monkeypatch, E, "rid must be a contiguous 4-byte tensor with n = 3 elements", f,
            **dict(request_in(), rid=z(2 * N, i32)[::2]))
    refuses(monkeypatch, E, "params must be a contiguous uint8 tensor", f, **dict(request_in(), params=z(16, i16)))
    refuses(monkeypatch, E, TABLE, f, **dict(request_in(), table=rpc_amd.RouteTable(z(6, u8), z(4, i32), 2)))
    refuses(monkeypatch, E, CONN_FIRST, f, **dict(request_in(), conn_first=z(3, i32)))
    refuses(monkeypatch, E, OUT1, f, **request_in(), out=NONCONTIG)
    # two faults: the index tensors, then params, table, conn_first, out
    refuses(monkeypatch, E, "types must be a contiguous 2-byte tensor with n = 3 elements", f,
            **dict(request_in(), types=z(N, i32), params=NONCONTIG))
    refuses(monkeypatch, E, "params must be a contiguous uint8 tensor", f,
            **dict(request_in(), params=NONCONTIG, table=rpc_amd.RouteTable(z(6, u8), z(4, i32), 2)))
    refuses(monkeypatch, E, TABLE, f,
            **dict(request_in(), table=rpc_amd.RouteTable(z(6, u8), z(4, i32), 2), conn_first=nil(i64)))
    refuses(monkeypatch, E, CONN_FIRST, f, **dict(request_in(), conn_first=nil(i64)), out=NONCONTIG)


# ---- frames_values --------------------------------------------------------------------------------

def values_in(form_=None):
    kw = dict(method=z(N, i16), slots=z((2, N), i64), schema=z(2, u8), mode=z(N, u8), status=z(N, i32), strings=z(16, u8),
              str_base=z(N, i64), texts=z(8, u8), text_offsets=z(N, i64), text_lens=z(N, i32))
    if form_ == rpc_amd.VALUES_FORM_PARAMS:
        kw.update(schema=schema(), form=form_)
    return kw


VALUES_OUTS = (">value_offsets", ">value_lens", ">status", ">reply_status", ">ndefer")
VALUES_FORM = {"values": (u8, (16,)), "value_offsets": (i64, (3,)), "value_lens": (i32, (3,)), "status": (u8, (3,)),
               "reply_status": (i32, (3,)), "ndefer": (i32, (1,)), "total": (i64, (1,))}
RESULT_SCHEMA = ("schema", None, 2, None, None, 0, None, 0)
PARAMS_SCHEMA = (None, "schema.first", 2, "schema.types", "schema.name_off", 3, "schema.names", 5)


def test_frames_values_with_out(monkeypatch):
    E = "rpc_frames_values_device"
    for form_, sch in ((rpc_amd.VALUES_FORM_RESULT, RESULT_SCHEMA), (rpc_amd.VALUES_FORM_PARAMS, PARAMS_SCHEMA)):
        kw = dict(values_in(form_), out=z(16, u8))
        fake = Fake(monkeypatch, E, word_at=29)
        r = rpc_amd.frames_values(**kw, stream=S)
        assert r.values is kw["out"]
        assert fake.seen(kw, r) == [(E, form_, "mode", "status", "method", "slots", 2, 3) + sch
                                    + ("strings", 16, "str_base", "texts", 8, "text_offsets", "text_lens", "out", 16)
                                    + VALUES_OUTS + ("total", SH)]
        assert form(r) == VALUES_FORM


def test_frames_values_sizes_itself(monkeypatch, current):
    E = "rpc_frames_values_device"
    for form_, sch in ((rpc_amd.VALUES_FORM_RESULT, RESULT_SCHEMA), (rpc_amd.VALUES_FORM_PARAMS, PARAMS_SCHEMA)):
        kw = dict(method=z(N, i16), slots=z((2, N), i64), schema=values_in(form_)["schema"])
        fake = Fake(monkeypatch, E, word_at=29, words=[5])
        r = rpc_amd.frames_values(**kw, form=form_)
        head = (E, form_, None, None, "method", "slots", 2, 3) + sch + (None, 0, None, None, 0, None, None)
        assert fake.seen(kw, r) == [head + (None, 0, None, None, None, None, None, "total", CUR),
                                    head + (">values", 5) + VALUES_OUTS + ("total", CUR)]
        assert form(r) == dict(VALUES_FORM, values=(u8, (5,)), total=5)
        assert type(r.total) is int


def test_frames_values_empty(monkeypatch):
    E = "rpc_frames_values_device"
    kw = dict(method=nil(i16), slots=z((2, 0), i64), schema=nil(u8), mode=nil(u8), status=nil(i32), strings=nil(u8),
              str_base=nil(i64), texts=nil(u8), text_offsets=nil(i64), text_lens=nil(i32), out=nil(u8))
    fake = Fake(monkeypatch, E, word_at=29)
    r = rpc_amd.frames_values(**kw, stream=S)  # (ndefer is passed raw: it is one element long)
    assert fake.seen(kw, r) == [(E, 0, None, None, None, None, 2, 0, None, None, 0, None, None, 0, None, 0, None, 0, None, None,
                                 0, None, None, None, 0, None, None, None, None, ">ndefer", "total", SH)]
    kw.update(schema=rpc_amd.ArgsSchema(z(1, i32), nil(u8), z(1, i32), nil(u8), 0, 0, 1), slots=z((0, 0), i64))
    fake = Fake(monkeypatch, E, word_at=29)
    r = rpc_amd.frames_values(**kw, form=rpc_amd.VALUES_FORM_PARAMS, stream=S)
    assert fake.seen(kw, r) == [(E, 1, None, None, None, None, 0, 0, None, "schema.first", 0, None, "schema.name_off", 0, None,
                                 0, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, ">ndefer", "total",
                                 SH)]
    assert form(r)["value_offsets"] == (i64, (0,)) and form(r)["ndefer"] == (i32, (1,))


def test_frames_values_refuses(monkeypatch):
    E, f = "rpc_frames_values_device", rpc_amd.frames_values
    for bad in (z(2 * N, i64), z((2, N), i32), z((N, 4), i64).t()[:2], z((2, N + 1), i64)):
        refuses(monkeypatch, E, "slots must be a contiguous 8-byte tensor [width, 3]", f, **dict(values_in(), slots=bad))
    refuses_each(monkeypatch, E, f, values_in, [("mode", 1), ("status", 4), ("str_base", 8), ("text_offsets", 8),
                                                ("text_lens", 4)])
    refuses(monkeypatch, E, "method must be a contiguous 2-byte tensor with n = 3 elements", f,
            **dict(values_in(), method=z(N, i32)))
    for name in ("strings", "texts", "out"):
        for bad in (NONCONTIG, z(16, i16)):
            refuses(monkeypatch, E, f"{name} must be a contiguous uint8 tensor", f, **dict(values_in(), **{name: bad}))
    for bad in BAD_SCHEMAS:
        refuses(monkeypatch, E, SCHEMA, f, **dict(values_in(rpc_amd.VALUES_FORM_PARAMS), schema=bad(schema())))
    for bad in (z(2, i16), z(4, u8)[::2]):
        refuses(monkeypatch, E, "result types must be a contiguous uint8 tensor", f, **dict(values_in(), schema=bad))
    # two faults: slots, then the index tensors, then strings, texts, out, then the schema
    refuses(monkeypatch, E, "slots must be a contiguous 8-byte tensor [width, 3]", f,
            **dict(values_in(), slots=z((2, N), i32), method=z(N, i32)))
    refuses(monkeypatch, E, "text_lens must be a contiguous 4-byte tensor with n = 3 elements", f,
            **dict(values_in(), text_lens=z(N, i64), strings=NONCONTIG))
    refuses(monkeypatch, E, "texts must be a contiguous uint8 tensor", f, **dict(values_in(), texts=NONCONTIG), out=NONCONTIG)
    refuses(monkeypatch, E, OUT1, f, **dict(values_in(), schema=z(2, i16)), out=NONCONTIG)


# ---- frames_scan ----------------------------------------------------------------------------------

SCAN, SCAN_VERIFY = "rpc_frames_scan_device", "rpc_frames_scan_verify_device"
SCANS = [SCAN, SCAN_VERIFY]
SCAN_CONN = (">conn_first", ">consumed", ">state", "nframes")
SCAN_FORM = {"frame_offsets": (i64, (4,)), "frame_conn": (i32, (4,)), "conn_first": (i64, (3,)), "consumed": (i64, (2,)),
             "state": (u8, (2,)), "verdict": None, "crc": None, "nframes": 2}


def scan_in():
    return dict(stream_buf=z(16, u8), conn_offsets=z(NCONN, i64), conn_lengths=z(NCONN, i64))


def scan_fake(monkeypatch, words):
    return Fake(monkeypatch, SCANS, word_at=12, words=words, word="nframes")


def test_frames_scan_counts_first(monkeypatch, current):
    kw = scan_in()
    head = ("stream_buf", 16, "conn_offsets", "conn_lengths", 2, 0x1)
    fake = scan_fake(monkeypatch, [2])
    r = rpc_amd.frames_scan(**kw)
    assert fake.seen(kw, r) == [(SCAN,) + head + (None, None, 0) + SCAN_CONN + (CUR,),
                                (SCAN,) + head + (">frame_offsets", ">frame_conn", 2) + SCAN_CONN + (CUR,)]
    assert form(r) == dict(SCAN_FORM, frame_offsets=(i64, (2,)), frame_conn=(i32, (2,)))
    assert type(r.nframes) is int
    fake = scan_fake(monkeypatch, [2])  # (the count call is the plain scan's, whatever verify says)
    r = rpc_amd.frames_scan(**kw, verify=True)
    assert fake.seen(kw, r) == [(SCAN,) + head + (None, None, 0) + SCAN_CONN + (CUR,),
                                (SCAN_VERIFY,) + head + (">frame_offsets", ">frame_conn", 2) + SCAN_CONN
                                + (">verdict", ">crc", CUR)]
    assert form(r) == dict(SCAN_FORM, frame_offsets=(i64, (2,)), frame_conn=(i32, (2,)), verdict=(u8, (2,)), crc=(i32, (2,)))
    fake = scan_fake(monkeypatch, [0])  # (no frames: nothing to point at)
    r = rpc_amd.frames_scan(**kw, verify=True)
    assert fake.seen(kw, r)[1] == (SCAN_VERIFY,) + head + (None, None, 0) + SCAN_CONN + (None, None, CUR)
    assert r.nframes == 0 and form(r)["verdict"] == (u8, (0,))


def test_frames_scan_max_frames(monkeypatch, current):
    kw = scan_in()
    fake = scan_fake(monkeypatch, [2])
    r = rpc_amd.frames_scan(**kw, max_frames=4, role="client", lift_cap=True, stream_bytes=12)
    assert fake.seen(kw, r) == [(SCAN, "stream_buf", 12, "conn_offsets", "conn_lengths", 2, 0x2 | 0x4, ">frame_offsets",
                                 ">frame_conn", 4) + SCAN_CONN + (CUR,)]
    assert form(r) == SCAN_FORM and type(r.nframes) is int
    fake = scan_fake(monkeypatch, [4])
    r = rpc_amd.frames_scan(**kw, max_frames=4, verify=True)
    assert fake.seen(kw, r) == [(SCAN_VERIFY, "stream_buf", 16, "conn_offsets", "conn_lengths", 2, 0x1, ">frame_offsets",
                                 ">frame_conn", 4) + SCAN_CONN + (">verdict", ">crc", CUR)]
    assert form(r) == dict(SCAN_FORM, verdict=(u8, (4,)), crc=(i32, (4,)), nframes=4)
    fake = scan_fake(monkeypatch, [7])
    with pytest.raises(ValueError) as e:
        rpc_amd.frames_scan(**kw, max_frames=4)
    assert str(e.value) == "frames_scan found 7 frames, max_frames is 4"
    assert len(fake.calls) == 1


def test_frames_scan_without_read_back(monkeypatch):
    kw = scan_in()
    fake = scan_fake(monkeypatch, [])  # (writes nothing: the count is not looked at, 7 frames or none)
    r = rpc_amd.frames_scan(**kw, max_frames=4, read_count=False, verify=True, stream=S)
    assert fake.seen(kw, r) == [(SCAN_VERIFY, "stream_buf", 16, "conn_offsets", "conn_lengths", 2, 0x1, ">frame_offsets",
                                 ">frame_conn", 4) + SCAN_CONN + (">verdict", ">crc", SH)]
    assert form(r) == dict(SCAN_FORM, verdict=(u8, (4,)), crc=(i32, (4,)), nframes=(i64, (1,)))
    fake = scan_fake(monkeypatch, [])
    r = rpc_amd.frames_scan(**kw, max_frames=4, read_count=False, stream=S)
    assert fake.seen(kw, r) == [(SCAN, "stream_buf", 16, "conn_offsets", "conn_lengths", 2, 0x1, ">frame_offsets",
                                 ">frame_conn", 4) + SCAN_CONN + (SH,)]


def test_frames_scan_empty(monkeypatch):
    kw = dict(stream_buf=nil(u8), conn_offsets=nil(i64), conn_lengths=nil(i64))
    fake = scan_fake(monkeypatch, [])  # (the buffer raw and stream_bytes as given; conn_first is one element long)
    r = rpc_amd.frames_scan(**kw, max_frames=0, read_count=False, stream_bytes=12, stream=S)
    assert fake.seen(kw, r) == [(SCAN, "stream_buf", 12, None, None, 0, 0x1, None, None, 0, ">conn_first", None, None, "nframes",
                                 SH)]
    assert form(r) == {"frame_offsets": (i64, (0,)), "frame_conn": (i32, (0,)), "conn_first": (i64, (1,)),
                       "consumed": (i64, (0,)), "state": (u8, (0,)), "verdict": None, "crc": None, "nframes": (i64, (1,))}


def test_frames_scan_refuses(monkeypatch):
    f = rpc_amd.frames_scan
    refuses(monkeypatch, SCANS, "conn_offsets and conn_lengths differ in length", f, **dict(scan_in(), conn_lengths=z(3, i64)))
    refuses(monkeypatch, SCANS, ROLE, f, **scan_in(), role="peer")
    refuses(monkeypatch, SCANS, "read_count=False needs max_frames", f, **scan_in(), read_count=False)
    refuses(monkeypatch, SCANS, "conn_offsets and conn_lengths differ in length", f,  # two faults
            **dict(scan_in(), conn_lengths=z(3, i64)), role="peer")
    refuses(monkeypatch, SCANS, ROLE, f, **scan_in(), role="peer", read_count=False)
