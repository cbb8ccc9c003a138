#!/usr/bin/env python3
"""tools/request_bench.py -- rpc_frames_request_device on two shapes:

  (a) the route bench's entry count and method mix: about 1.9M entries, 64 % strlen_s, 35 % the
      other six methods, 1 % an unknown method (an eighth table entry), with the params the
      client stubs build for the seven methods and random 32-bit ids: requests of 45-120 bytes;
  (b) 16 calls whose params are 64 MiB each, at odd offsets of the params buffer: what a
      RPC_FRAMES_LIFT_CAP pack would take.

Legs: the request call; a flat device-to-device copy of `total` bytes (Tensor.copy_: the floor of
the copy stage); and the way without it, timed on 65,536 entries and reported per entry:
json.dumps per request, the join, np.cumsum for the offsets and the H2D of all of it (host wall
time; the device legs are device time).

Device legs are timed with device events around `reps` back-to-back calls after a warm-up, in
`rounds` alternating rounds; medians are reported.  Every leg's result is checked: the layout of
every entry against the lengths by construction, the bytes of the host leg's entries against
what json.dumps builds, the big params against their source.  One JSON line.

  python tools/request_bench.py [--entries 1900000] [--big 16] [--big-mib 64] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="request_bench")

DEV = torch.device("cuda", 0)
HOST_ENTRIES = 65536
K = 4096  # template entries
METHODS = ["ping", "echo_i64", "add_i32", "mul_double", "is_even", "strlen_s", "mix3", "no_such_method"]
FIXED = len('{"jsonrpc":"2.0","method":"","params":,"id":}')  # 45


def params_of(rng, m):
    """The params the client stub of method m builds (client/gen/rpc_client_gen.c's shapes)."""
    i32 = lambda: int(rng.integers(-2**31, 2**31))  # noqa: E731
    dbl = lambda: [0.5, -1.25, 3, 1e20, 2.5e-7, 12345.678][int(rng.integers(0, 6))]  # noqa: E731
    return [{}, {"x": str(int(rng.integers(-2**62, 2**62)))}, {"a": i32(), "b": i32()}, {"a": dbl(), "b": dbl()},
            {"n": i32()}, {"s": "s" * int(rng.integers(0, 33))}, {"a": i32(), "b": dbl(), "ok": bool(rng.integers(0, 2))},
            {}][m]


class Request:
    """Preallocated outputs of one request shape; the calls go straight to the C ABI."""

    def __init__(self, method, rid, params, poff, plen, total):
        self.method, self.rid, self.params, self.poff, self.plen = method, rid, params, poff, plen
        self.table = rpc_amd.route_table(METHODS, device=DEV)
        n = self.n = rid.numel()
        self.out = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.boff = torch.empty(n, dtype=torch.int64, device=DEV)
        self.blen = torch.empty(n, dtype=torch.int32, device=DEV)
        self.types = torch.empty(n, dtype=torch.int16, device=DEV)
        self.state = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.total = torch.empty(1, dtype=torch.int64, device=DEV)
        self.copy_src = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.copy_dst = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def request(self):
        t = self.table
        _lib.check(_lib.rpc_frames_request_device(self.method.data_ptr(), self.rid.data_ptr(), None, self.n,
                                                  t.names.data_ptr(), t.names.numel(), t.offsets.data_ptr(), t.nmethods,
                                                  self.params.data_ptr(), self.params.numel(), self.poff.data_ptr(),
                                                  self.plen.data_ptr(), None, 0, self.out.data_ptr(), self.out.numel(),
                                                  self.boff.data_ptr(), self.blen.data_ptr(), self.types.data_ptr(),
                                                  self.state.data_ptr(), None, self.total.data_ptr(), self.h), "request")

    def copy(self):
        self.copy_dst.copy_(self.copy_src)


def host_request(method, params, rid):
    return json.dumps({"jsonrpc": "2.0", "method": method, "params": params, "id": rid}, separators=(",", ":")).encode()


def host_way(meths, params, rids):
    """The way without the call: the envelopes by json.dumps, the join, the offsets, the H2D."""
    reqs = [host_request(METHODS[m], p, r) for m, p, r in zip(meths, params, rids)]
    lens = np.fromiter(map(len, reqs), dtype=np.int32, count=len(reqs))
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)])
    blob = np.frombuffer(b"".join(reqs), dtype=np.uint8)
    d = (torch.from_numpy(blob).to(DEV), torch.from_numpy(offs).to(DEV), torch.from_numpy(lens).to(DEV))
    torch.cuda.synchronize()
    return reqs, d


def shape_a(a):
    rng = np.random.default_rng(0xA)
    n = a.entries
    meth, objs = [], []
    for _ in range(K):
        u = rng.random()
        m = 5 if u < 0.64 else (0, 1, 2, 3, 4, 6)[int(rng.integers(0, 6))] if u < 0.99 else 7
        meth.append(m)
        objs.append(params_of(rng, m))
    texts = [json.dumps(o, separators=(",", ":")).encode() for o in objs]
    tlen = np.array([len(v) for v in texts], dtype=np.int64)
    toff = np.concatenate([[0], np.cumsum(tlen[:-1])])
    block = np.frombuffer(b"".join(texts), dtype=np.uint8)
    reps_ = -(-n // K)
    params = torch.from_numpy(block.copy()).to(DEV).repeat(reps_)
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    poff = torch.from_numpy(toff).to(DEV)[i % K] + (i // K) * len(block)
    plen = torch.from_numpy(tlen.astype(np.int32)).to(DEV)[i % K].contiguous()
    method = torch.from_numpy(np.array(meth, dtype=np.int16)).to(DEV)[i % K].contiguous()
    nlen = torch.tensor([len(x) for x in METHODS], dtype=torch.int64, device=DEV)[method.to(torch.int64)]
    rid64 = torch.randint(0, 2**32, (n,), dtype=torch.int64, device=DEV)
    rid = (rid64 - ((rid64 >> 31) << 32)).to(torch.int32)  # (the same 32 bits)
    digits = sum((rid64 >= 10 ** p).to(torch.int64) for p in range(1, 10)) + 1
    want_len = FIXED + nlen + plen.to(torch.int64) + digits
    total = int(want_len.sum())
    r = Request(method, rid, params, poff.contiguous(), plen, total)
    r.request()
    torch.cuda.synchronize()
    ok = {"total": int(r.total.cpu()[0]) == total,
          "lens": bool(torch.equal(r.blen.to(torch.int64), want_len)),
          "offsets": bool(torch.equal(r.boff, torch.cumsum(want_len, 0) - want_len)),
          "types": bool((r.types == 0).all()),
          "states": bool((r.state == rpc_amd.REQUEST_CALL).all())}
    # the host leg's entries: the device's bytes against json.dumps's
    h = min(HOST_ENTRIES, n)
    hm, hr = [meth[j % K] for j in range(h)], rid64[:h].cpu().tolist()
    hp = [objs[j % K] for j in range(h)]
    t0 = time.perf_counter()
    reqs, d = host_way(hm, hp, hr)
    host_us = (time.perf_counter() - t0) * 1e6
    nb = int(d[0].numel())
    ok["bytes_equal_host_way"] = bool(torch.equal(r.out[:nb], d[0])) and bool(torch.equal(r.boff[:h], d[1]))
    ok["lens_equal_host_way"] = bool(torch.equal(r.blen[:h], d[2]))
    j = n - 1
    tail = r.out[int(r.boff[j]):].cpu().numpy().tobytes()  # the last entry, built on the host
    ok["last_entry"] = tail == host_request(METHODS[meth[j % K]], objs[j % K], int(rid64[j]))
    host_runs = [host_us]
    for _ in range(a.rounds - 1):
        t0 = time.perf_counter()
        host_way(hm, hp, hr)
        host_runs.append((time.perf_counter() - t0) * 1e6)
    legs = rounds_of({"request": r.request, "flat_copy": r.copy}, a.reps, a.rounds, "a")
    med = float(np.median(host_runs))
    legs["json_dumps_join_h2d"] = {"entries": h, "us": [round(x, 1) for x in host_runs], "median_us": round(med, 1),
                                   "ns_per_entry": round(med * 1e3 / h, 1),
                                   "scaled_to_all_entries_us": round(med * n / h, 1)}
    res = {"entries": n, "params_bytes": int(params.numel()), "params_bytes_used": int(plen.sum()), "total_bytes": total,
           "unknown_method": int((method == 7).sum()), "correct": ok, "legs": legs}
    m = {k: v["median_us"] for k, v in legs.items()}
    res["request_over_flat_copy"] = round(m["request"] / m["flat_copy"], 2)
    res["request_ns_per_entry"] = round(m["request"] * 1e3 / n, 3)
    res["host_way_over_request"] = round(legs["json_dumps_join_h2d"]["scaled_to_all_entries_us"] / m["request"], 1)
    return res


def shape_b(a):
    n, vbytes = a.big, a.big_mib << 20
    step = vbytes + 2
    params = torch.empty((n * step + 64) & ~7, dtype=torch.uint8, device=DEV)  # (fill_random writes whole 8-byte words)
    rpc_amd.fill_random(params, 0xB16)
    poff = torch.arange(n, dtype=torch.int64, device=DEV) * step + 1  # (odd offsets: the funnel shift is at work)
    plen = torch.full((n,), vbytes, dtype=torch.int32, device=DEV)
    meths = [i % 7 for i in range(n)]
    method = torch.tensor(meths, dtype=torch.int16, device=DEV)
    rids = [10 ** (i % 10) - 1 + (i == 0) for i in range(n)]
    rid = torch.tensor(rids, dtype=torch.int64, device=DEV).to(torch.int32)
    heads = [b'{"jsonrpc":"2.0","method":"%s","params":' % METHODS[m].encode() for m in meths]
    tails = [b',"id":%d}' % x for x in rids]
    total = sum(len(hd) + vbytes + len(tl) for hd, tl in zip(heads, tails))
    r = Request(method, rid, params, poff, plen, total)
    r.request()
    torch.cuda.synchronize()
    at = r.boff.cpu().tolist()
    ok = {"total": int(r.total.cpu()[0]) == total, "states": bool((r.state == rpc_amd.REQUEST_CALL).all()),
          "lens": r.blen.cpu().tolist() == [len(hd) + vbytes + len(tl) for hd, tl in zip(heads, tails)]}
    ok["heads"] = all(r.out[at[i]:at[i] + len(heads[i])].cpu().numpy().tobytes() == heads[i] for i in range(n))
    ok["values"] = all(bool(torch.equal(r.out[at[i] + len(heads[i]):at[i] + len(heads[i]) + vbytes],
                                        params[i * step + 1:i * step + 1 + vbytes])) for i in range(n))
    ok["tails"] = all(r.out[at[i] + len(heads[i]) + vbytes:at[i] + len(heads[i]) + vbytes + len(tails[i])
                            ].cpu().numpy().tobytes() == tails[i] for i in range(n))
    # the way without it: the envelope around each value on the host, the join, the H2D of all of it
    hv = params[1:1 + vbytes].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    blob = b"".join(heads[i] + hv + tails[i] for i in range(n))
    d = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8)).to(DEV)
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    del d, blob
    legs = rounds_of({"request": r.request, "flat_copy": r.copy}, a.reps, a.rounds, "b")
    legs["join_h2d"] = {"us": [round(host_us, 1)], "median_us": round(host_us, 1)}
    res = {"values": n, "value_bytes": vbytes, "total_bytes": total, "correct": ok, "legs": legs}
    m = {k: v["median_us"] for k, v in legs.items()}
    res["request_over_flat_copy"] = round(m["request"] / m["flat_copy"], 2)
    res["request_gb_per_s"] = round(total / m["request"] / 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1900000)
    ap.add_argument("--big", type=int, default=16)
    ap.add_argument("--big-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"lib": os.environ.get("RPCCRC_LIB") or "in-tree", "reps": a.reps, "rounds": a.rounds}
    if not a.skip_a:
        res["a"] = shape_a(a)
        torch.cuda.empty_cache()
    if not a.skip_b:
        res["b"] = shape_b(a)
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
