#!/usr/bin/env python3
"""tools/reply_bench.py -- rpc_frames_reply_device on two shapes:

  (a) the route bench's entry count and method mix: about 1.9M entries, 64 % strlen_s, 35 % the
      other six methods, 1 % NOT_FOUND, with the value text the seven handlers give (`"pong"`,
      a quoted 64-bit number, a number, a double, true / false, a length, a quoted triple) and
      random 32-bit ids: replies of 40-90 bytes;
  (b) 16 results whose values are 64 MiB each, at odd offsets of the values buffer: what a
      RPC_FRAMES_LIFT_CAP pack would take.

Legs: the reply call; a flat device-to-device copy of `total` bytes (Tensor.copy_: the floor of
the copy stage); and the way without it, timed on 65,536 entries and reported per entry:
json.dumps per reply, the join, np.cumsum for the offsets and the H2D of all of it (host wall
time; the device legs are device time).

Device legs are timed with device events around `reps` back-to-back calls after a warm-up, in
`rounds` alternating rounds; medians are reported.  Every leg's result is checked: the layout of
every entry against the lengths by construction, the bytes of the host leg's entries against
what json.dumps builds, the big values against their source.  One JSON line.

  python tools/reply_bench.py [--entries 1900000] [--big 16] [--big-mib 64] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
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

rounds_of = functools.partial(bench_common.rounds_of, name="reply_bench")

DEV = torch.device("cuda", 0)
HOST_ENTRIES = 65536
K = 4096  # template entries
HEAD = len('{"jsonrpc":"2.0","id":')
RESULT = len(',"result":') + len("}")
NOT_FOUND = len(',"error":{"code":-32601,"message":"Method not found"}}')


def value_of(rng, m):
    """The value text handler m gives (tests/test_dropin_route.py's HANDLERS through json.dumps)."""
    i32 = lambda: int(rng.integers(-2**31, 2**31))  # noqa: E731
    dbl = lambda: [0.5, -1.25, 3.0, 1e20, 2.5e-7, 12345.678][int(rng.integers(0, 6))]  # noqa: E731
    v = ["pong", str(int(rng.integers(-2**62, 2**62))), i32() + i32(), dbl() * dbl(), bool(rng.integers(0, 2)),
         int(rng.integers(0, 1025)), "%d:%g:%s" % (i32(), dbl(), "true" if rng.integers(0, 2) else "false")][m]
    return json.dumps(v).encode()


class Reply:
    """Preallocated outputs of one reply shape; the calls go straight to the C ABI."""

    def __init__(self, kind, rid, values, voff, vlen, total):
        self.kind, self.rid, self.values, self.voff, self.vlen = kind, rid, values, voff, vlen
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

    def reply(self):
        _lib.check(_lib.rpc_frames_reply_device(self.kind.data_ptr(), self.rid.data_ptr(), None, None, self.n,
                                                self.values.data_ptr(), self.values.numel(), self.voff.data_ptr(),
                                                self.vlen.data_ptr(), None, 0, self.out.data_ptr(), self.out.numel(),
                                                self.boff.data_ptr(), self.blen.data_ptr(), self.types.data_ptr(),
                                                self.state.data_ptr(), None, self.total.data_ptr(), self.h), "reply")

    def copy(self):
        self.copy_dst.copy_(self.copy_src)


def host_reply(rid, result=None, error=None):
    d = {"jsonrpc": "2.0", "id": rid}
    d.update({"result": result} if error is None else {"error": error})
    return json.dumps(d, separators=(",", ":")).encode()


def host_way(kinds, rids, vals):
    """The way without the call: the envelopes by json.dumps, the join, the offsets, the H2D."""
    replies = [host_reply(r, result=v) if k == rpc_amd.ROUTE_CALL else
               host_reply(r, error={"code": -32601, "message": "Method not found"}) for k, r, v in zip(kinds, rids, vals)]
    lens = np.fromiter(map(len, replies), dtype=np.int32, count=len(replies))
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)])
    blob = np.frombuffer(b"".join(replies), dtype=np.uint8)
    d = (torch.from_numpy(blob).to(DEV), torch.from_numpy(offs).to(DEV), torch.from_numpy(lens).to(DEV))
    torch.cuda.synchronize()
    return replies, d


def shape_a(a):
    rng = np.random.default_rng(0xA)
    n = a.entries
    meth, vals = [], []
    for _ in range(K):
        u = rng.random()
        m = 5 if u < 0.64 else (0, 1, 2, 3, 4, 6)[int(rng.integers(0, 6))] if u < 0.99 else -1
        meth.append(m)
        vals.append(value_of(rng, m) if m >= 0 else b"")
    tlen = np.array([len(v) for v in vals], dtype=np.int64)
    toff = np.concatenate([[0], np.cumsum(tlen[:-1])])
    block = np.frombuffer(b"".join(vals), dtype=np.uint8)
    reps_ = -(-n // K)
    values = torch.from_numpy(block.copy()).to(DEV).repeat(reps_)
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    voff = torch.from_numpy(toff).to(DEV)[i % K] + (i // K) * len(block)
    vlen = torch.from_numpy(tlen.astype(np.int32)).to(DEV)[i % K].contiguous()
    kind = torch.from_numpy(np.where(np.array(meth) >= 0, rpc_amd.ROUTE_CALL, rpc_amd.ROUTE_NOT_FOUND).astype(np.uint8)
                            ).to(DEV)[i % K].contiguous()
    rid64 = torch.randint(0, 2**32, (n,), dtype=torch.int64, device=DEV)
    rid = (rid64 - ((rid64 >> 31) << 32)).to(torch.int32)  # (the same 32 bits)
    digits = sum((rid64 >= 10 ** p).to(torch.int64) for p in range(1, 10)) + 1
    want_len = HEAD + digits + torch.where(kind == rpc_amd.ROUTE_CALL, vlen.to(torch.int64) + RESULT,
                                           torch.full_like(digits, NOT_FOUND))
    total = int(want_len.sum())
    r = Reply(kind, rid, values, voff.contiguous(), vlen, total)
    r.reply()
    torch.cuda.synchronize()
    ok = {"total": int(r.total.cpu()[0]) == total,
          "lens": bool(torch.equal(r.blen.to(torch.int64), want_len)),
          "offsets": bool(torch.equal(r.boff, torch.cumsum(want_len, 0) - want_len)),
          "types": bool((r.types == 0).all()),
          "states": bool(torch.equal(r.state, torch.where(kind == rpc_amd.ROUTE_CALL, rpc_amd.REPLY_RESULT,
                                                          rpc_amd.REPLY_ERROR).to(torch.uint8)))}
    # the host leg's entries: the device's bytes against json.dumps's
    h = min(HOST_ENTRIES, n)
    hk, hr = kind[:h].cpu().tolist(), rid64[:h].cpu().tolist()
    hv = [json.loads(vals[j % K]) if meth[j % K] >= 0 else None for j in range(h)]
    t0 = time.perf_counter()
    replies, d = host_way(hk, hr, hv)
    host_us = (time.perf_counter() - t0) * 1e6
    nb = int(d[0].numel())
    ok["bytes_equal_host_way"] = bool(torch.equal(r.out[:nb], d[0])) and bool(torch.equal(r.boff[:h], d[1]))
    ok["lens_equal_host_way"] = bool(torch.equal(r.blen[:h], d[2]))
    tail = r.out[int(r.boff[n - 1]):].cpu().numpy().tobytes()  # the last entry, built on the host
    j = n - 1
    ok["last_entry"] = tail == (host_reply(int(rid64[j]), result=json.loads(vals[j % K])) if meth[j % K] >= 0 else
                                host_reply(int(rid64[j]), error={"code": -32601, "message": "Method not found"}))
    host_runs = [host_us]
    for _ in range(a.rounds - 1):
        t0 = time.perf_counter()
        host_way(hk, hr, hv)
        host_runs.append((time.perf_counter() - t0) * 1e6)
    legs = rounds_of({"reply": r.reply, "flat_copy": r.copy}, a.reps, a.rounds, "a")
    med = float(np.median(host_runs))
    legs["json_dumps_join_h2d"] = {"entries": h, "us": [round(x, 1) for x in host_runs], "median_us": round(med, 1),
                                   "ns_per_entry": round(med * 1e3 / h, 1),
                                   "scaled_to_all_entries_us": round(med * n / h, 1)}
    res = {"entries": n, "values_bytes": int(values.numel()), "value_bytes_used": int(vlen.sum()), "total_bytes": total,
           "not_found": int((kind == rpc_amd.ROUTE_NOT_FOUND).sum()), "correct": ok, "legs": legs}
    m = {k: v["median_us"] for k, v in legs.items()}
    res["reply_over_flat_copy"] = round(m["reply"] / m["flat_copy"], 2)
    res["reply_ns_per_entry"] = round(m["reply"] * 1e3 / n, 3)
    res["host_way_over_reply"] = round(legs["json_dumps_join_h2d"]["scaled_to_all_entries_us"] / m["reply"], 1)
    return res


def shape_b(a):
    n, vbytes = a.big, a.big_mib << 20
    step = vbytes + 2
    values = torch.empty((n * step + 64) & ~7, dtype=torch.uint8, device=DEV)  # (fill_random writes whole 8-byte words)
    rpc_amd.fill_random(values, 0xB16)
    voff = torch.arange(n, dtype=torch.int64, device=DEV) * step + 1  # (odd offsets: the funnel shift is at work)
    vlen = torch.full((n,), vbytes, dtype=torch.int32, device=DEV)
    kind = torch.full((n,), rpc_amd.ROUTE_CALL, dtype=torch.uint8, device=DEV)
    rids = [10 ** (i % 10) - 1 + (i == 0) for i in range(n)]
    rid = torch.tensor(rids, dtype=torch.int64, device=DEV).to(torch.int32)
    heads = [b'{"jsonrpc":"2.0","id":%d,"result":' % x for x in rids]
    total = sum(len(hd) + vbytes + 1 for hd in heads)
    r = Reply(kind, rid, values, voff, vlen, total)
    r.reply()
    torch.cuda.synchronize()
    at = r.boff.cpu().tolist()
    ok = {"total": int(r.total.cpu()[0]) == total, "states": bool((r.state == rpc_amd.REPLY_RESULT).all()),
          "lens": r.blen.cpu().tolist() == [len(hd) + vbytes + 1 for hd in heads]}
    ok["heads"] = all(r.out[at[i]:at[i] + len(heads[i])].cpu().numpy().tobytes() == heads[i] for i in range(n))
    ok["values"] = all(bool(torch.equal(r.out[at[i] + len(heads[i]):at[i] + len(heads[i]) + vbytes],
                                        values[i * step + 1:i * step + 1 + vbytes])) for i in range(n))
    ok["tails"] = all(int(r.out[at[i] + len(heads[i]) + vbytes]) == ord("}") for i in range(n))
    # the way without it: the envelope around each value on the host, the join, the H2D of all of it
    hv = values[1:1 + vbytes].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    blob = b"".join(heads[i] + hv + b"}" for i in range(n))
    d = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8)).to(DEV)
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    del d, blob
    legs = rounds_of({"reply": r.reply, "flat_copy": r.copy}, a.reps, a.rounds, "b")
    legs["join_h2d"] = {"us": [round(host_us, 1)], "median_us": round(host_us, 1)}
    res = {"values": n, "value_bytes": vbytes, "total_bytes": total, "correct": ok, "legs": legs}
    m = {k: v["median_us"] for k, v in legs.items()}
    res["reply_over_flat_copy"] = round(m["reply"] / m["flat_copy"], 2)
    res["reply_gb_per_s"] = round(total / m["reply"] / 1e3, 1)
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
