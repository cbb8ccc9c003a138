#!/usr/bin/env python3
"""tools/resolve_bench.py -- rpc_frames_resolve_device on two shapes:

  (a) the reply bench's replies: about 1.9M bodies of 40-90 bytes, back to back as the unpack
      leaves them (built on the device by rpc_frames_reply_device from the seven handlers' value
      texts, 1 % of them "Method not found" errors), with distinct 32-bit ids in random order,
      against as many pending ids in another random order: every slot is matched;
  (b) the same bodies with npending == 0, the decode-only call: (a) - (b) is the price of the
      join.

Legs: the call; rpc_amd.stream_read over the same bytes (the floor: the bodies are read once);
and the host loop the call replaces, timed on 65,536 bodies and reported per body: one D2H of
those bodies, then json.loads per body for `id`, `result` / `error`, and dict.pop(id) on the
pending table (host wall time; the device legs are device time).

Device legs are timed with device events around `reps` back-to-back calls after a warm-up, in
`rounds` alternating rounds; medians are reported.  Every leg's result is checked: ids, kinds,
slots and the open count against what the bodies were built from, the spans of the first 65,536
bodies against the values; the host leg's answers against the same.  One JSON line.

  python tools/resolve_bench.py [--entries 1900000] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
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

rounds_of = functools.partial(bench_common.rounds_of, name="resolve_bench")

DEV = torch.device("cuda", 0)
HOST_BODIES = 65536
K = 4096  # template entries


def value_of(rng, m):
    """The value text handler m gives (the reply bench's)."""
    i32 = lambda: int(rng.integers(-2**31, 2**31))  # noqa: E731
    dbl = lambda: [0.5, -1.25, 3.0, 1e20, 2.5e-7, 12345.678][int(rng.integers(0, 6))]  # noqa: E731
    v = ["pong", str(int(rng.integers(-2**62, 2**62))), i32() + i32(), dbl() * dbl(), bool(rng.integers(0, 2)),
         int(rng.integers(0, 1025)), "%d:%g:%s" % (i32(), dbl(), "true" if rng.integers(0, 2) else "false")][m]
    return json.dumps(v).encode()


def build(n):
    """-> (bodies, offsets, lengths, ids, is_error, value bytes per template entry): the replies
    on the device, entry i from template entry i % K."""
    rng = np.random.default_rng(0xA)
    meth, vals = [], []
    for _ in range(K):
        u = rng.random()
        m = 5 if u < 0.64 else (0, 1, 2, 3, 4, 6)[int(rng.integers(0, 6))] if u < 0.99 else -1
        meth.append(m)
        vals.append(value_of(rng, m) if m >= 0 else b"")
    vlen_t = np.array([len(v) for v in vals], dtype=np.int32)
    voff_t = np.concatenate([[0], np.cumsum(vlen_t[:-1], dtype=np.int64)])
    which = torch.arange(n, device=DEV) % K
    kind = torch.where(torch.tensor([m >= 0 for m in meth], device=DEV)[which], rpc_amd.ROUTE_CALL,
                       rpc_amd.ROUTE_NOT_FOUND).to(torch.uint8)
    g = torch.Generator(device="cpu").manual_seed(0xB)
    ids = (torch.randperm(n, generator=g) * ((2**32 - 1) // n)).to(DEV)  # distinct, spread over 0 .. 2^32 - 1
    rep = rpc_amd.frames_reply(kind, ids.to(torch.int32), torch.from_numpy(np.frombuffer(b"".join(vals), dtype=np.uint8).copy()).to(DEV),
                               torch.from_numpy(voff_t).to(DEV)[which].contiguous(),
                               torch.from_numpy(vlen_t).to(DEV)[which].contiguous())
    torch.cuda.synchronize()
    return rep.bodies, rep.body_offsets, rep.body_lens, ids, [m < 0 for m in meth], vals


class Resolve:
    """Preallocated outputs of one resolve shape; the calls go straight to the C ABI."""

    def __init__(self, bodies, offs, lens, pending):
        self.b, self.off, self.len, self.pend = bodies, offs, lens, pending
        n, npend = offs.numel(), pending.numel()
        self.n, self.npend = n, npend
        self.kind = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.id, self.roff, self.rlen, self.eoff, self.elen, self.slot = (torch.empty(n, dtype=torch.int32, device=DEV)
                                                                          for _ in range(6))
        self.slot_entry = torch.empty(max(npend, 1), dtype=torch.int32, device=DEV)
        self.open = torch.empty(max(npend, 1), dtype=torch.int32, device=DEV)
        self.nopen = torch.empty(1, dtype=torch.int32, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def call(self):
        _lib.check(_lib.rpc_frames_resolve_device(self.b.data_ptr(), self.b.numel(), self.off.data_ptr(), self.len.data_ptr(),
                                                  None, self.n, self.pend.data_ptr() if self.npend else None, self.npend,
                                                  self.kind.data_ptr(), self.id.data_ptr(), self.roff.data_ptr(),
                                                  self.rlen.data_ptr(), self.eoff.data_ptr(), self.elen.data_ptr(),
                                                  self.slot.data_ptr(), self.slot_entry.data_ptr(), self.open.data_ptr(),
                                                  self.nopen.data_ptr(), self.h), "resolve")

    def floor(self):
        nb = self.b.numel() // 4096 * 4096
        rpc_amd.stream_read(self.b[:nb], pattern=0)


def host_way(r, ids, pending):
    """One D2H of HOST_BODIES bodies, json.loads per body, dict.pop on the pending table.
    -> (us per body, ok)"""
    n = min(HOST_BODIES, r.n)
    end = int(r.off[n - 1].item()) + int(r.len[n - 1].item())
    offs, lens = r.off[:n].cpu().tolist(), r.len[:n].cpu().tolist()
    table = {int(i): s for s, i in enumerate((pending.to(torch.int64) & 0xFFFFFFFF).cpu().tolist())}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = r.b[:end].cpu().numpy().tobytes()
    got = []
    for o, ln in zip(offs, lens):
        d = json.loads(host[o:o + ln])
        got.append((d["id"], table.pop(d["id"], None), "result" in d, "error" in d))
    dt = time.perf_counter() - t0
    return dt * 1e6 / n, got


def run_shape(tag, built, join, a):
    bodies, offs, lens, ids, is_err, vals = built
    n = offs.numel()
    g = torch.Generator(device="cpu").manual_seed(0xC)
    pending = ids[torch.randperm(n, generator=g).to(DEV)].to(torch.int32).contiguous() if join else \
        torch.empty(0, dtype=torch.int32, device=DEV)
    r = Resolve(bodies, offs, lens, pending)
    r.call()
    torch.cuda.synchronize()
    u32 = lambda x: x.to(torch.int64) & 0xFFFFFFFF  # noqa: E731
    ok = {"id": bool(torch.equal(u32(r.id), ids))}
    err = torch.tensor(is_err, device=DEV)[torch.arange(n, device=DEV) % K]
    ok["member_presence"] = bool(torch.equal(r.rlen > 0, ~err)) and bool(torch.equal(r.elen > 0, err))
    if join:
        ok["all_matched"] = bool((r.kind == rpc_amd.RESOLVE_MATCHED).all()) and int(r.nopen.item()) == 0
        ok["slot_holds_the_id"] = bool(torch.equal(u32(pending)[r.slot.to(torch.int64)], ids))
        ok["slot_entry_inverts_slot"] = bool(torch.equal(r.slot_entry.to(torch.int64)[r.slot.to(torch.int64)],
                                                         torch.arange(n, device=DEV)))
    else:
        ok["all_unknown"] = bool((r.kind == rpc_amd.RESOLVE_UNKNOWN).all()) and int(r.nopen.item()) == 0
        ok["no_slot"] = bool((r.slot == -1).all())
    nk = min(HOST_BODIES, n)
    end = int(offs[nk - 1].item()) + int(lens[nk - 1].item())
    host = bodies[:end].cpu().numpy().tobytes()
    o_, ro, rl, eo, el = (x[:nk].cpu().tolist() for x in (offs, r.roff, r.rlen, r.eoff, r.elen))
    ok["spans"] = all((host[o + a_:o + a_ + b_] == vals[i % K]) if not is_err[i % K] else
                      (json.loads(host[o + c_:o + c_ + d_])["code"] == -32601)
                      for i, (o, a_, b_, c_, d_) in enumerate(zip(o_, ro, rl, eo, el)))
    per_body_us, got = host_way(r, ids, pending)
    idl, sl = ids[:nk].cpu().tolist(), r.slot[:nk].cpu().tolist()
    ok["host_way"] = got == [(i, (s if join else None), not is_err[k % K], is_err[k % K])
                             for k, (i, s) in enumerate(zip(idl, sl))]
    legs = {"resolve": r.call, "stream_read": r.floor}
    res = {"entries": n, "npending": r.npend, "bytes": bodies.numel(), "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, tag)}
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["resolve_over_stream_read"] = round(m["resolve"] / m["stream_read"], 2)
    res["resolve_ns_per_body"] = round(m["resolve"] * 1e3 / n, 3)
    res["host_loop_us_per_body"] = round(per_body_us, 3)
    res["host_loop_bodies"] = nk
    res["host_loop_for_all_entries_over_resolve"] = round(per_body_us * n / m["resolve"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1900000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"lib": os.environ.get("RPCCRC_LIB") or "in-tree", "reps": a.reps, "rounds": a.rounds}
    built = build(a.entries)
    if not a.skip_a:
        res["a"] = run_shape("a", built, True, a)
    if not a.skip_b:
        res["b"] = run_shape("b", built, False, a)
    if "a" in res and "b" in res:
        res["join_us"] = round(res["a"]["legs"]["resolve"]["median_us"] - res["b"]["legs"]["resolve"]["median_us"], 1)
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
