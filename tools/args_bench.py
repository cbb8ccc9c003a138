#!/usr/bin/env python3
"""tools/args_bench.py -- rpc_frames_args_device on the route bench's two shapes (DESIGN.md
4.19), with the schema of the IDL's seven methods:

  (a) about 1.9M canonical requests, each followed by its NUL, in blocks of 64 KiB: 64 %
      strlen_s padded to 64-1024 B, 35 % the other six methods, 1 % unknown methods (those are
      no CALL: the args read NONE);
  (b) the same count of ping requests in 64-byte slots: a method without parameters, where
      nothing but the route's outputs is read.

Legs: args on the route's own outputs; route (no groups) on the same entries in the same
visit; and the host loop the args replace, timed on 65,536 bodies and reported per body:
json.loads on each CALL's `params` span plus the pulls of the declared fields out of the dict
(host wall time, after the one D2H of the bodies; the device legs are device time).

Device legs are timed as tools/route_bench.py times them; medians are reported.  The args'
result is checked: every CALL reads OK and its slots are the values the bodies were built from
(an F64 slot bit for bit, a STR slot by its bytes), every other entry NONE; the host loop's
values against the same.  One JSON line.

  python tools/args_bench.py [--entries 1900000] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import route_bench as rb  # noqa: E402

DEV, K, BLOCK = rb.DEV, rb.K, rb.BLOCK
SCHEMA = [("ping", []), ("echo_i64", [("x", "i64")]), ("add_i32", [("a", "i32"), ("b", "i32")]),
          ("mul_double", [("a", "double"), ("b", "double")]), ("is_even", [("n", "i32")]), ("strlen_s", [("s", "string")]),
          ("mix3", [("a", "i32"), ("b", "double"), ("ok", "bool")])]
assert [m for m, _ in SCHEMA] == rb.METHODS
WIDTH = 3
M64 = (1 << 64) - 1


class Args:
    """Preallocated outputs of one shape; the calls go straight to the C ABI."""

    def __init__(self, route, schema):
        self.r, self.s = route, schema
        n = route.n
        self.slots = torch.empty((WIDTH, n), dtype=torch.int64, device=DEV)
        self.status = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.reply = torch.empty(n, dtype=torch.int32, device=DEV)

    def call(self):
        r, s = self.r, self.s
        _lib.check(_lib.rpc_frames_args_device(r.b.data_ptr(), r.b.numel(), r.off.data_ptr(), r.len.data_ptr(),
                                               r.kind.data_ptr(), r.method.data_ptr(), r.poff.data_ptr(), r.plen.data_ptr(),
                                               r.n, s.first.data_ptr(), s.nmethods, s.types.data_ptr(), s.name_off.data_ptr(),
                                               s.nparams, s.names.data_ptr(), s.names.numel(), WIDTH, self.slots.data_ptr(),
                                               self.status.data_ptr(), self.reply.data_ptr(), r.h), "args")


def pulls(m, p):
    """The host loop's field pulls for method m out of the parsed dict."""
    if m == 1:
        return (int(p["x"]),)
    if m == 2:
        return (int(p["a"]), int(p["b"]))
    if m == 3:
        return (float(p["a"]), float(p["b"]))
    if m == 4:
        return (int(p["n"]),)
    if m == 5:
        return (p["s"],)
    if m == 6:
        return (int(p["a"]), float(p["b"]), bool(p["ok"]))
    return ()


def wanted_slots(m, p, body, po):
    """The slots of a request built from params p (route_bench.params_of)."""
    bits = lambda x: struct.unpack("<Q", struct.pack("<d", float(x)))[0]  # noqa: E731
    if m == 5:
        at = body.index(b'"s":"', po) + 5
        return [at | len(p["s"]) << 32]
    v = pulls(m, p)
    if m == 3:
        return [bits(x) for x in v]
    if m == 6:
        return [v[0] & M64, bits(v[1]), int(v[2])]
    return [x & M64 for x in v]


def host_loop(r, methods, want):
    """One D2H of HOST_BODIES bodies, then json.loads per CALL span and the field pulls.
    -> (us per body, ok)"""
    n = min(rb.HOST_BODIES, r.n)
    end = int(r.off[n - 1].item()) + int(r.len[n - 1].item())
    offs = r.off[:n].cpu().tolist()
    poff, plen = r.poff[:n].cpu().tolist(), r.plen[:n].cpu().tolist()
    torch.cuda.synchronize()
    host = r.b[:end].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    got = []
    for o, po, pl, m in zip(offs, poff, plen, methods):
        got.append(pulls(m, json.loads(host[o + po:o + po + pl])) if m >= 0 and pl else ())
    dt = time.perf_counter() - t0
    return dt * 1e6 / n, got == want[:n]


def run_shape(tag, blocks, a):
    nblocks = max(1, round(a.entries / (sum(len(t[1]) for t in blocks) / K)))
    host = np.frombuffer(b"".join(t[0] for t in blocks), dtype=np.uint8).reshape(K, BLOCK)
    which = torch.arange(nblocks, device=DEV) % K
    bodies = torch.from_numpy(host.copy()).to(DEV)[which].reshape(-1).contiguous()
    toff = [np.array([r[0] for r in t[1]], dtype=np.int64) for t in blocks]
    tlen = [np.array([r[1] for r in t[1]], dtype=np.int32) for t in blocks]
    offs = torch.from_numpy(np.concatenate([toff[c % K] + c * BLOCK for c in range(nblocks)])).to(DEV)
    lens = torch.from_numpy(np.concatenate([tlen[c % K] for c in range(nblocks)])).to(DEV)
    r = rb.Route(bodies, offs, lens, rpc_amd.route_table(rb.METHODS))
    g = Args(r, rpc_amd.args_schema(SCHEMA))
    r.plain()
    g.call()
    torch.cuda.synchronize()
    # the first K blocks against what they were built from, the last block against its template
    first = blocks[:min(K, nblocks)]
    rows = [(c * BLOCK, row) for c, t in enumerate(first) for row in t[1]]
    nk = len(rows)
    flat = b"".join(t[0] for t in first)
    status = g.status[:nk].cpu().tolist()
    slots = g.slots[:, :nk].cpu().numpy().view(np.uint64).T.tolist()
    poff = r.poff[:nk].cpu().tolist()
    ok = {"status": all(s == (rpc_amd.ARGS_OK if w[2] >= 0 else rpc_amd.ARGS_NONE) for s, (_, w) in zip(status, rows)),
          "reply_status": bool((g.reply[g.status == rpc_amd.ARGS_OK] == 0).all()) and
          bool((g.reply[g.status == rpc_amd.ARGS_NONE] == -32603).all()),
          "only_ok_and_none": bool(((g.status == rpc_amd.ARGS_OK) | (g.status == rpc_amd.ARGS_NONE)).all())}
    ok["slots"] = all(sl == (wanted_slots(w[2], w[4], flat[b + w[0]:b + w[0] + w[1]], po) + [0] * WIDTH)[:WIDTH]
                      if w[2] >= 0 else sl == [0] * WIDTH for sl, po, (b, w) in zip(slots, poff, rows))
    if nblocks > K:
        per = torch.tensor([len(t[1]) for t in blocks], device=DEV)[which]
        start = torch.cumsum(per, 0) - per
        c = nblocks - 1
        s0, s1, cnt = int(start[c % K]), int(start[c]), int(per[c])
        ok["replicas"] = bool(torch.equal(g.slots[:, s0:s0 + cnt], g.slots[:, s1:s1 + cnt])) and \
            bool(torch.equal(g.status[s0:s0 + cnt], g.status[s1:s1 + cnt]))
    methods, want, c = [], [], 0
    while len(want) < min(rb.HOST_BODIES, r.n):  # (block c holds block c % K's requests)
        methods += [w[2] for w in blocks[c % K][1]]
        want += [pulls(w[2], w[4]) if w[2] >= 0 else () for w in blocks[c % K][1]]
        c += 1
    per_body_us, ok["host_loop"] = host_loop(r, methods, want)
    res = {"entries": r.n, "bytes": bodies.numel(), "blocks": nblocks,
           "params_bytes": int(r.plen.to(torch.int64).sum().item()), "correct": ok,
           "legs": rb.rounds_of({"args": g.call, "route": r.plain}, a.reps, a.rounds, tag)}
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["args_over_route"] = round(m["args"] / m["route"], 2)
    res["host_loop_us_per_body"] = round(per_body_us, 3)
    res["host_loop_bodies"] = min(rb.HOST_BODIES, r.n)
    res["host_loop_for_all_entries_over_args"] = round(per_body_us * r.n / m["args"], 1)
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
    rng = np.random.default_rng(0xA)
    if not a.skip_a:
        res["a"] = run_shape("a", [rb.template_block(rng) for _ in range(K)], a)
        torch.cuda.empty_cache()
    if not a.skip_b:
        res["b"] = run_shape("b", [rb.ping_block(rng) for _ in range(K)], a)
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
