#!/usr/bin/env python3
"""tools/route_bench.py -- rpc_frames_route_device on two shapes:

  (a) the unpack bench's entry count: about 1.9M delivered bodies, each followed by its NUL,
      back to back as the unpack leaves them, in blocks of 64 KiB (a connection's worth).  The
      bodies are canonical requests (what the reference client's encoder emits): 64 % strlen_s
      whose string pads the body to a length drawn from 64-1024 B, 35 % the other six methods
      at their natural length (57-110 B), 1 % unknown methods;
  (b) the same count of ping requests in 64-byte slots (the request, spaces up to 63 bytes,
      the NUL): small bodies are where the per-entry cost shows.

Legs: route without groups; route with groups; rpc_amd.stream_read over the same bytes (the
floor: the bodies are read once); and the way without route, timed on 65,536 bodies and
reported per body: one D2H of those bodies, then json.loads per body for `method` and `id`
(host wall time; the device legs are device time).

Device legs are timed with device events around `reps` back-to-back calls after a warm-up,
in `rounds` alternating rounds; medians are reported.  Every leg's result is checked: kind,
method, id and the params span against what the bodies were built from, the groups against
the counts by construction and as a stable sort; the host leg's answers against the same.
One JSON line.

  python tools/route_bench.py [--entries 1900000] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
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

rounds_of = functools.partial(bench_common.rounds_of, name="route_bench")

BLOCK = 65536
DEV = torch.device("cuda", 0)
METHODS = ["ping", "echo_i64", "add_i32", "mul_double", "is_even", "strlen_s", "mix3"]
HOST_BODIES = 65536
K = 64  # template blocks


def request(method, params, rid):
    """rpc_codec_encode_request's output: jsonrpc, method, params, id; no whitespace."""
    return json.dumps({"jsonrpc": "2.0", "method": method, "params": params, "id": rid}, separators=(",", ":")).encode()


def params_of(rng, m):
    i32 = lambda: int(rng.integers(-2**31, 2**31))  # noqa: E731
    dbl = lambda: [0.5, -1.25, 3, 1e20, 2.5e-7, 12345.678][int(rng.integers(0, 6))]  # noqa: E731
    return [{}, {"x": str(int(rng.integers(-2**62, 2**62)))}, {"a": i32(), "b": i32()}, {"a": dbl(), "b": dbl()},
            {"n": i32()}, {"s": ""}, {"a": i32(), "b": dbl(), "ok": bool(rng.integers(0, 2))}][m]


def template_block(rng):
    """64 KiB of bodies with their NULs, the last strlen_s padded so that the block ends exactly.
    -> (bytes, [(offset, length, method index or -1, id, params, method name)])"""
    out, rows = bytearray(), []
    while True:
        rid = int(rng.integers(0, 2**32))
        u, left = rng.random(), BLOCK - len(out)
        if left <= 1025:  # the block's last body: whatever is left (at least 127 bytes, see below)
            m, n = 5, left - 1
        elif u < 0.64:
            m, n = 5, min(int(rng.integers(64, 1025)), left - 129)
        elif u < 0.99:
            m, n = (0, 1, 2, 3, 4, 6)[int(rng.integers(0, 6))], 0
        else:
            m, n = -1, 0
        name = METHODS[m] if m >= 0 else ("nope", "pingg", "add_i64")[int(rng.integers(0, 3))]
        p = params_of(rng, m) if m >= 0 else {}
        body = request(name, p, rid)
        if m == 5:  # pad with the string (printable, no escapes) up to n bytes
            p = {"s": rng.integers(0x30, 0x5B, max(n - len(body), 0), dtype=np.uint8).tobytes().decode()}
            body = request(name, p, rid)
        rows.append((len(out), len(body), m, rid, p, name))
        out += body + b"\0"
        if len(out) == BLOCK:
            return bytes(out), rows
        assert BLOCK - len(out) >= 128


class Route:
    """Preallocated outputs of one route shape; the calls go straight to the C ABI."""

    def __init__(self, bodies, offs, lens, table):
        self.b, self.off, self.len, self.tab = bodies, offs, lens, table
        n = self.n = offs.numel()
        self.kind = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.method = torch.empty(n, dtype=torch.int16, device=DEV)
        self.id = torch.empty(n, dtype=torch.int32, device=DEV)
        self.poff = torch.empty(n, dtype=torch.int32, device=DEV)
        self.plen = torch.empty(n, dtype=torch.int32, device=DEV)
        self.order = torch.empty(n, dtype=torch.int32, device=DEV)
        self.first = torch.empty(table.nmethods + 4, dtype=torch.int32, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def call(self, group):
        _lib.check(_lib.rpc_frames_route_device(self.b.data_ptr(), self.b.numel(), self.off.data_ptr(), self.len.data_ptr(),
                                                None, self.n, self.tab.names.data_ptr(), self.tab.names.numel(),
                                                self.tab.offsets.data_ptr(), self.tab.nmethods, self.kind.data_ptr(),
                                                self.method.data_ptr(), self.id.data_ptr(), self.poff.data_ptr(),
                                                self.plen.data_ptr(), self.order.data_ptr() if group else None,
                                                self.first.data_ptr() if group else None, self.h), "route")

    def plain(self):
        self.call(False)

    def grouped(self):
        self.call(True)

    def floor(self):
        rpc_amd.stream_read(self.b, pattern=0)


def host_way(r, want):
    """One D2H of HOST_BODIES bodies, json.loads per body for method and id.  -> (us per body, ok)"""
    n = min(HOST_BODIES, r.n)
    end = int(r.off[n - 1].item()) + int(r.len[n - 1].item())
    offs, lens = r.off[:n].cpu().tolist(), r.len[:n].cpu().tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = r.b[:end].cpu().numpy().tobytes()
    got = []
    for o, ln in zip(offs, lens):
        d = json.loads(host[o:o + ln])
        got.append((d["method"], d["id"]))
    dt = time.perf_counter() - t0
    return dt * 1e6 / n, got == want[:n]


def check_groups(r, nm, bucket_counts):
    first = r.first.cpu().tolist()
    sizes = [b - a for a, b in zip(first, first[1:])]
    order = r.order[:first[-1]].to(torch.int64)
    kind, method = r.kind.to(torch.int64), r.method.to(torch.int64) & 0xFFFF
    bucket = torch.where(kind == rpc_amd.ROUTE_CALL, method, nm + kind - rpc_amd.ROUTE_NOT_FOUND)[order]
    stable = bool(((bucket[1:] > bucket[:-1]) | ((bucket[1:] == bucket[:-1]) & (order[1:] > order[:-1]))).all())
    return {"group_sizes": sizes == bucket_counts, "stable_sort": stable}


def run_shape(tag, blocks, a):
    """blocks: K template blocks of BLOCK bytes with their rows, replicated over the entries."""
    nblocks = max(1, round(a.entries / (sum(len(t[1]) for t in blocks) / K)))
    host = np.frombuffer(b"".join(t[0] for t in blocks), dtype=np.uint8).reshape(K, BLOCK)
    which = torch.arange(nblocks, device=DEV) % K
    bodies = torch.from_numpy(host.copy()).to(DEV)[which].reshape(-1).contiguous()
    toff = [np.array([r[0] for r in t[1]], dtype=np.int64) for t in blocks]
    tlen = [np.array([r[1] for r in t[1]], dtype=np.int32) for t in blocks]
    offs = torch.from_numpy(np.concatenate([toff[c % K] + c * BLOCK for c in range(nblocks)])).to(DEV)
    lens = torch.from_numpy(np.concatenate([tlen[c % K] for c in range(nblocks)])).to(DEV)
    table = rpc_amd.route_table(METHODS)
    nm = table.nmethods
    r = Route(bodies, offs, lens, table)
    r.grouped()
    torch.cuda.synchronize()
    # the first K blocks against what they were built from, the rest against the first K
    rows = [row for t in blocks[:min(K, nblocks)] for row in t[1]]
    nk = len(rows)
    kind, method = r.kind[:nk].cpu().tolist(), (r.method[:nk].cpu().numpy().view(np.uint16)).tolist()
    rid = r.id[:nk].cpu().numpy().view(np.uint32).tolist()
    poff, plen = r.poff[:nk].cpu().tolist(), r.plen[:nk].cpu().tolist()
    flat = b"".join(t[0] for t in blocks)
    ok = {"kind_method_id": all((k, m, i) == ((rpc_amd.ROUTE_CALL, w[2], w[3]) if w[2] >= 0 else
                                              (rpc_amd.ROUTE_NOT_FOUND, rpc_amd.ROUTE_NO_METHOD, w[3]))
                                for k, m, i, w in zip(kind, method, rid, rows))}
    base = np.repeat(np.arange(min(K, nblocks)) * BLOCK, [len(t[1]) for t in blocks[:min(K, nblocks)]]).tolist()
    ok["params_span"] = all(json.loads(flat[b + w[0] + po:b + w[0] + po + pl]) == w[4]
                            for b, po, pl, w in zip(base, poff, plen, rows) if w[2] >= 0)
    per = torch.tensor([len(t[1]) for t in blocks], device=DEV)[which]
    start = torch.cumsum(per, 0) - per
    if nblocks > K:  # block c's outputs equal block c % K's
        c = nblocks - 1
        s0, s1, cnt = int(start[c % K]), int(start[c]), int(per[c])
        ok["replicas"] = all(bool(torch.equal(x[s0:s0 + cnt], x[s1:s1 + cnt])) for x in (r.kind, r.method, r.id, r.poff, r.plen))
    counts = [0] * (nm + 3)
    reps_of = np.bincount(np.arange(nblocks) % K, minlength=K)
    for t, times in zip(blocks, reps_of):
        for w in t[1]:
            counts[w[2] if w[2] >= 0 else nm] += int(times)
    ok.update(check_groups(r, nm, counts))
    want, c = [], 0
    while len(want) < min(HOST_BODIES, r.n):  # (block c holds block c % K's requests)
        want += [(w[5], w[3]) for w in blocks[c % K][1]]
        c += 1
    per_body_us, ok["host_way"] = host_way(r, want)
    legs = {"route": r.plain, "route_groups": r.grouped, "stream_read": r.floor}
    res = {"entries": r.n, "bytes": bodies.numel(), "blocks": nblocks, "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, tag)}
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["route_over_stream_read"] = round(m["route"] / m["stream_read"], 2)
    res["route_groups_over_stream_read"] = round(m["route_groups"] / m["stream_read"], 2)
    res["host_json_loads_us_per_body"] = round(per_body_us, 3)
    res["host_json_loads_bodies"] = min(HOST_BODIES, r.n)
    res["host_way_for_all_entries_over_route"] = round(per_body_us * r.n / m["route"], 1)
    return res


def ping_block(rng):
    out, rows = bytearray(), []
    while len(out) < BLOCK:
        rid = int(rng.integers(10**9, 2**32))
        body = request("ping", {}, rid)
        body += b" " * (63 - len(body))
        rows.append((len(out), 63, 0, rid, {}, "ping"))
        out += body + b"\0"
    return bytes(out), rows


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
        res["a"] = run_shape("a", [template_block(rng) for _ in range(K)], a)
        torch.cuda.empty_cache()
    if not a.skip_b:
        res["b"] = run_shape("b", [ping_block(rng) for _ in range(K)], a)
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
