"""What rpc_amd.frames_results hands to rpc_frames_results_device: the real wrapper, CPU tensors
and test_wrapper_calls' recording stand-in for the entry, no GPU needed.  Every pointer of the
recorded call is replaced by the name of the tensor it is and the list compared with a tuple
written by hand from the parameter list of include/rpccrc.h; every ``raise ValueError`` of the
wrapper is asked for once with its exact message, and the entry must not have been called."""
import rpc_amd
from test_wrapper_calls import (CUR, N, NONCONTIG, S, SH, Fake, current, form, i16, i32, i64, nil, refuses,  # noqa: F401
                                refuses_each, u8, z)

E = "rpc_frames_results_device"
NPEND = 4
ENTRY_OUTS = (">status", ">value", ">error_status", ">error_code", ">error_message")
SLOT_OUTS = (">slot_status", ">slot_value", ">slot_error_status", ">slot_error_code", ">slot_str_base")


def resolve(n=N, npend=NPEND):
    return rpc_amd.FrameResolve(z(n, u8), z(n, i32), z(n, i32), z(n, i32), z(n, i32), z(n, i32), z(n, i32),
                                z(npend, i32), z(npend, i32), z(1, i32))


def results_in():
    return dict(bodies=z(16, u8), body_offsets=z(N, i64), body_lens=z(N, i32), resolve=resolve(),
                pending_method=z(NPEND, i16), result_types=z(5, u8))


def results_call(sh=SH):
    return (E, "bodies", 16, "body_offsets", "body_lens", "resolve.kind", "resolve.slot", "resolve.result_off",
            "resolve.result_len", "resolve.error_off", "resolve.error_len", "resolve.slot_entry", 3, "pending_method", 4,
            "result_types", 5, *ENTRY_OUTS, *SLOT_OUTS, ">ndefer", sh)


def test_frames_results(monkeypatch, current):  # noqa: F811
    kw = results_in()
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_results(**kw, stream=S)
    assert fake.seen(kw, r) == [results_call()]
    assert form(r) == {"status": (u8, (3,)), "value": (i64, (3,)), "error_status": (u8, (3,)), "error_code": (i32, (3,)),
                       "error_message": (i64, (3,)), "slot_status": (u8, (4,)), "slot_value": (i64, (4,)),
                       "slot_error_status": (u8, (4,)), "slot_error_code": (i32, (4,)), "slot_str_base": (i64, (4,)),
                       "ndefer": (i32, (1,))}
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_results(**kw)
    assert fake.seen(kw, r) == [results_call(sh=CUR)]
    assert isinstance(r, rpc_amd.FrameResults) and rpc_amd.frames.frames_results is rpc_amd.frames_results


def test_frames_results_empty(monkeypatch):
    """No entries and slots that stay open; and nothing at all: every empty tensor is NULL with
    count 0, the count word alone keeps its address."""
    rv = rpc_amd.FrameResolve(nil(u8), nil(i32), nil(i32), nil(i32), nil(i32), nil(i32), nil(i32), z(NPEND, i32), None, None)
    kw = dict(bodies=nil(u8), body_offsets=nil(i64), body_lens=nil(i32), resolve=rv, pending_method=z(NPEND, i16),
              result_types=z(5, u8))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_results(**kw, stream=S)
    assert fake.seen(kw, r) == [(E, None, 0, None, None, None, None, None, None, None, None, "resolve.slot_entry", 0,
                                 "pending_method", 4, "result_types", 5, None, None, None, None, None, *SLOT_OUTS, ">ndefer",
                                 SH)]
    kw = dict(kw, resolve=rv._replace(slot_entry=nil(i32)), pending_method=None, result_types=nil(u8))
    fake = Fake(monkeypatch, E)
    r = rpc_amd.frames_results(**kw, stream=S)
    assert fake.seen(kw, r) == [(E,) + (None, 0) + (None,) * 9 + (0, None, 0, None, 0) + (None,) * 10 + (">ndefer", SH)]
    assert form(r)["slot_value"] == (i64, (0,)) and form(r)["ndefer"] == (i32, (1,))


def test_frames_results_refuses(monkeypatch):
    f = rpc_amd.frames_results
    refuses_each(monkeypatch, E, f, results_in, [("body_lens", 4), ("resolve.kind", 1), ("resolve.slot", 4),
                                                 ("resolve.result_off", 4), ("resolve.result_len", 4),
                                                 ("resolve.error_off", 4), ("resolve.error_len", 4)])
    refuses(monkeypatch, E, "body_offsets must be a contiguous 8-byte tensor with n = 3 elements", f,
            **dict(results_in(), body_offsets=z(N, i32)))
    refuses(monkeypatch, E, "bodies must be a contiguous uint8 tensor", f, **dict(results_in(), bodies=NONCONTIG))
    refuses_each(monkeypatch, E, f, results_in, [("resolve.slot_entry", 4)], count="npending", n=NPEND)
    refuses(monkeypatch, E, "resolve.slot_entry must be a contiguous 4-byte tensor with npending = 5 elements", f,
            **dict(results_in(), pending_method=z(5, i16)))  # (pending_method gives npending)
    refuses(monkeypatch, E, "pending_method must be a contiguous 2-byte tensor with npending = 4 elements", f,
            **dict(results_in(), pending_method=z(NPEND, i32)))
    types = "result_types must be a contiguous 1-byte tensor of at most 256 elements"
    for bad in (z(5, i16), z(10, u8)[::2], z(257, u8)):
        refuses(monkeypatch, E, types, f, **dict(results_in(), result_types=bad))
    refuses(monkeypatch, E, "at most 16777216 pending slots", f,
            **dict(results_in(), pending_method=z((1 << 24) + 1, i16)))
    refuses(monkeypatch, E, "resolve.kind must be a contiguous 1-byte tensor with n = 3 elements", f,  # two faults
            **dict(results_in(), resolve=resolve()._replace(kind=z(N, i16)), bodies=NONCONTIG))
