#!/usr/bin/env python3
"""tools/carry_bench.py -- rpc_frames_carry_device on two shapes:

  (a) the scan bench's 16384 connections, each cut mid-frame so that its tail is 1-1035
      bytes, with 64 KiB of new bytes per connection already in place in the next buffer;
  (b) RPC_FRAMES_LIFT_CAP, 16 connections with tails of 32 MiB at odd offsets.

Legs of (a): the carry call; the device way without it, a torch index gather of tail + new
bytes into a fresh contiguous stream; and what the host way re-uploads, timed as one H2D of
carried + new bytes against one H2D of the new bytes alone (pinned memory).  Legs of (b): the
carry call and a flat Tensor.copy_ of the same byte count.

Device legs are timed with device events around `reps` back-to-back calls after a warm-up, in
`rounds` alternating rounds; medians are reported.  Every leg's result is checked.  One JSON
line.

  python tools/carry_bench.py [--conns 16384] [--big 16] [--big-mib 32] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
"""
import argparse
import functools
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="carry_bench")

CONN_BYTES = 65536
DEV = torch.device("cuda", 0)


class Carry:
    """Preallocated outputs of one carry shape; the calls go straight to the C ABI."""

    def __init__(self, stream_t, off, ln, used, nxt, at, new_len, room):
        self.s, self.off, self.ln, self.used, self.nxt, self.at, self.nl, self.room = stream_t, off, ln, used, nxt, at, new_len, room
        n = off.numel()
        self.n = n
        self.noff = torch.empty(n, dtype=torch.int64, device=DEV)
        self.nlen = torch.empty(n, dtype=torch.int64, device=DEV)
        self.status = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.carried = torch.empty(1, dtype=torch.int64, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def carry(self):
        _lib.check(_lib.rpc_frames_carry_device(self.s.data_ptr(), self.s.numel(), self.off.data_ptr(), self.ln.data_ptr(),
                                                self.used.data_ptr(), None, self.n, self.nxt.data_ptr(), self.nxt.numel(),
                                                self.at.data_ptr(), self.room, self.nl.data_ptr(), self.noff.data_ptr(),
                                                self.nlen.data_ptr(), self.status.data_ptr(), self.carried.data_ptr(),
                                                self.h), "carry")

    def correct(self, tails):
        """Words against the inputs; every carried byte against the stream."""
        total = int(tails.sum())
        conn = torch.repeat_interleave(torch.arange(self.n, device=DEV), tails, output_size=total)
        k = torch.arange(total, device=DEV) - (torch.cumsum(tails, 0) - tails)[conn]
        return {
            "status_ok": bool((self.status == rpc_amd.CARRY_OK).all()),
            "carried": int(self.carried.cpu()[0]) == total,
            "next_off": bool(torch.equal(self.noff, self.at - tails)),
            "next_len": bool(torch.equal(self.nlen, tails + self.nl)),
            "tail_bytes": bool(torch.equal(self.nxt[(self.at - tails)[conn] + k], self.s[(self.off + self.used)[conn] + k])),
        }


def shape_a(a):
    n = a.conns
    rng = np.random.default_rng(0xCA)
    tails_h = rng.integers(1, rpc_amd.RPC_HEADER_LEN + rpc_amd.MAX_BODY_LEN, n)  # 1 .. 1035
    stream_t = torch.empty(n * CONN_BYTES, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(stream_t, 0xA11)
    at_h, next_bytes = rpc_amd.carry_slots([CONN_BYTES] * n)
    nxt = torch.empty(next_bytes, dtype=torch.uint8, device=DEV)  # (the new bytes: whatever is there)
    off = torch.arange(n, dtype=torch.int64, device=DEV) * CONN_BYTES
    ln = torch.full((n,), CONN_BYTES, dtype=torch.int64, device=DEV)
    tails = torch.from_numpy(tails_h).to(DEV)
    used = ln - tails
    at = torch.from_numpy(at_h).to(DEV)
    nl = torch.full((n,), CONN_BYTES, dtype=torch.int64, device=DEV)
    c = Carry(stream_t, off, ln, used, nxt, at, nl, rpc_amd.CARRY_ROOM)
    c.carry()
    torch.cuda.synchronize()
    ok = c.correct(tails)

    # the device way without the call: one fresh contiguous stream of tail + new bytes
    col = torch.arange(CONN_BYTES, device=DEV)[None, :]
    keep = {}

    def gather(keep=None):
        t = ln - used
        starts = torch.cumsum(t + nl, 0) - (t + nl)
        total_t = int(tails_h.sum())  # (a read-back in earnest: the tails are known on the device only)
        conn = torch.repeat_interleave(torch.arange(n, device=DEV), t, output_size=total_t)
        k = torch.arange(total_t, device=DEV) - (torch.cumsum(t, 0) - t)[conn]
        out = torch.empty(total_t + n * CONN_BYTES, dtype=torch.uint8, device=DEV)
        out[starts[conn] + k] = stream_t[(off + used)[conn] + k]
        out[(starts + t)[:, None] + col] = nxt[at[:, None] + col]
        if keep is not None:
            keep.update(out=out, starts=starts)

    gather(keep)
    torch.cuda.synchronize()
    pick = [0, n // 2, n - 1]
    ok["gather_equals_carry"] = all(
        bool(torch.equal(keep["out"][int(keep["starts"][i]):int(keep["starts"][i]) + int(c.nlen[i])],
                         nxt[int(c.noff[i]):int(c.noff[i]) + int(c.nlen[i])])) for i in pick)
    keep.clear()
    torch.cuda.empty_cache()

    # what the host way re-uploads: carried + new against new alone
    new_bytes, carried_bytes = n * CONN_BYTES, int(tails_h.sum())
    pin = torch.empty(new_bytes + carried_bytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(new_bytes + carried_bytes, dtype=torch.uint8, device=DEV)
    legs = {"carry": c.carry, "torch_gather": gather,
            "h2d_new": lambda: dst[:new_bytes].copy_(pin[:new_bytes], non_blocking=True),
            "h2d_carried_and_new": lambda: dst.copy_(pin, non_blocking=True)}
    res = {"conns": n, "new_bytes": new_bytes, "carried_bytes": carried_bytes, "next_bytes": int(next_bytes),
           "correct": ok, "legs": rounds_of(legs, a.reps, a.rounds, "a")}
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["gather_over_carry"] = round(m["torch_gather"] / m["carry"], 1)
    res["h2d_extra_us"] = round(m["h2d_carried_and_new"] - m["h2d_new"], 1)
    return res


def shape_b(a):
    n, tail = a.big, a.big_mib << 20
    step = tail + 64 + 3
    stream_t = torch.empty((n * step + 64) & ~7, dtype=torch.uint8, device=DEV)  # (fill_random writes whole 8-byte words)
    rpc_amd.fill_random(stream_t, 0xB16)
    off = torch.arange(n, dtype=torch.int64, device=DEV) * step + 1  # (odd offsets: the funnel shift is at work)
    ln = torch.full((n,), tail + 64, dtype=torch.int64, device=DEV)
    used = torch.full((n,), 64, dtype=torch.int64, device=DEV)
    room = tail + 16
    at_h, next_bytes = rpc_amd.carry_slots([5] * n, room=room)
    at_h = at_h + 7  # (and odd destinations)
    nxt = torch.empty(next_bytes + 7, dtype=torch.uint8, device=DEV)
    at = torch.from_numpy(at_h).to(DEV)
    nl = torch.full((n,), 5, dtype=torch.int64, device=DEV)
    c = Carry(stream_t, off, ln, used, nxt, at, nl, room)
    c.carry()
    torch.cuda.synchronize()
    tails = torch.full((n,), tail, dtype=torch.int64, device=DEV)
    ok = {k: v for k, v in c.correct(tails).items()}
    src, dst = torch.empty(n * tail, dtype=torch.uint8, device=DEV), torch.empty(n * tail, dtype=torch.uint8, device=DEV)
    legs = {"carry": c.carry, "flat_copy": lambda: dst.copy_(src)}
    res = {"conns": n, "tail_bytes": tail, "total_bytes": n * tail, "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, "b")}
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["carry_over_flat_copy"] = round(m["carry"] / m["flat_copy"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=16384)
    ap.add_argument("--big", type=int, default=16)
    ap.add_argument("--big-mib", type=int, default=32)
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
