#!/usr/bin/env python3
"""tools/pack_bench.py -- rpc_frames_pack_device on two shapes:

  (a) 1,048,576 data frames with bodies of 64-1024 B in 16384 connections, the bodies
      scattered over the source buffer;
  (b) RPC_FRAMES_LIFT_CAP, 16 bodies of 64 MiB.

Legs: the pack call; the CRC pass alone (rpc_crc32_device_batch_bounded over the same
bodies); a flat device-to-device copy of `total` bytes (Tensor.copy_: the floor of the
copy stage); and for (a) the way without pack: frame offsets by torch.cumsum, the bodies
moved by a per-byte index gather, then rpc_amd.frames_stamp.

Device legs are timed with device events around `reps` back-to-back calls after a
warm-up, in `rounds` alternating rounds; medians are reported.  Every leg's result is
checked against what the inputs were built from: pack's stream against the offsets and
bodies it was given (and, byte for byte, against the stream the other way builds), and
through the fused scan + verify.  One JSON line.

  python tools/pack_bench.py [--frames 1048576] [--conns 16384] [--big 16] [--big-mib 64] [--reps 5] [--rounds 3]
                             [--skip-a] [--skip-b]
"""
import argparse
import functools
import json
import os
import struct
import sys
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="pack_bench")

HDR = 12
DEV = torch.device("cuda", 0)


class Pack:
    """Preallocated outputs of one pack shape; the calls go straight to the C ABI."""

    def __init__(self, src, soff, lens, conn_first, total, flags):
        self.src, self.soff, self.lens, self.conn_first, self.flags = src, soff, lens, conn_first, flags
        n = soff.numel()
        self.n = n
        self.out = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.fo = torch.empty(n, dtype=torch.int64, device=DEV)
        self.verdict = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.crc = torch.empty(n, dtype=torch.int32, device=DEV)
        self.cbf = torch.empty(conn_first.numel(), dtype=torch.int64, device=DEV)
        self.total = torch.empty(1, dtype=torch.int64, device=DEV)
        self.crc_alone = torch.empty(n, dtype=torch.int32, device=DEV)
        self.copy_src = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.copy_dst = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def pack(self):
        _lib.check(_lib.rpc_frames_pack_device(self.src.data_ptr(), self.src.numel(), self.soff.data_ptr(),
                                               self.lens.data_ptr(), self.n, None, rpc_amd.RPC_TYPE_DATA, None, 1,
                                               self.conn_first.data_ptr(), self.conn_first.numel() - 1, self.flags,
                                               self.out.data_ptr(), self.out.numel(), self.fo.data_ptr(),
                                               self.verdict.data_ptr(), self.crc.data_ptr(), self.cbf.data_ptr(),
                                               self.total.data_ptr(), self.h), "pack")

    def crc_pass(self, max_len):
        _lib.check(_lib.rpc_crc32_device_batch_bounded(self.src.data_ptr(), self.soff.data_ptr(), self.lens.data_ptr(),
                                                       self.n, max_len, self.crc_alone.data_ptr(), self.h), "crc")

    def copy(self):
        self.copy_dst.copy_(self.copy_src)


def derived(res):
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["pack_minus_crc_us"] = round(m["pack"] - m["crc_pass"], 1)
    res["flat_copy_us"] = m["flat_copy"]
    if "cumsum_gather_stamp" in m:
        res["other_way_over_pack"] = round(m["cumsum_gather_stamp"] / m["pack"], 2)
    return res


def shape_a(a):
    rng = np.random.default_rng(0xA)
    n = a.frames
    lens_h = rng.integers(64, 1025, n, dtype=np.int64)
    order = rng.permutation(n)  # the bodies lie in the source in another order than they are sent in
    soff_h = np.empty(n, dtype=np.int64)
    soff_h[order] = np.concatenate([[0], np.cumsum(lens_h[order])[:-1]])
    foff_h = np.concatenate([[0], np.cumsum(HDR + lens_h)[:-1]])
    total, src_bytes = int(foff_h[-1] + HDR + lens_h[-1]), int(lens_h.sum())
    conn_h = (np.arange(a.conns + 1, dtype=np.int64) * n) // a.conns
    src = torch.empty((src_bytes + 7) & ~7, dtype=torch.uint8, device=DEV)  # (fill_random writes whole 8-byte words)
    rpc_amd.fill_random(src, 0xA11CE)
    soff, lens64 = torch.from_numpy(soff_h).to(DEV), torch.from_numpy(lens_h).to(DEV)
    lens = lens64.to(torch.int32)
    p = Pack(src, soff, lens, torch.from_numpy(conn_h).to(DEV), total, 0)

    other = {}

    def other_way():  # offsets by cumsum, a per-byte index gather, then stamp
        sizes = lens64 + HDR
        foff = torch.cumsum(sizes, 0) - sizes
        bstart = torch.cumsum(lens64, 0) - lens64
        frame_of = torch.repeat_interleave(torch.arange(n, device=DEV), lens64, output_size=src_bytes)
        at = torch.arange(src_bytes, device=DEV)
        stream = torch.empty(total, dtype=torch.uint8, device=DEV)
        stream[at + (foff + HDR - bstart)[frame_of]] = src[at + (soff - bstart)[frame_of]]
        rpc_amd.frames_stamp(stream, foff, lens)
        other["stream"], other["foff"] = stream, foff

    p.pack()
    p.crc_pass(1024)
    other_way()
    torch.cuda.synchronize()
    scan = rpc_amd.frames_scan(p.out, p.cbf[:-1].contiguous(), (p.cbf[1:] - p.cbf[:-1]).contiguous(), role="server",
                               verify=True, max_frames=n)
    ok = {
        "total": int(p.total.cpu()[0]) == total,
        "offsets": bool(torch.equal(p.fo, torch.from_numpy(foff_h).to(DEV))),
        "conn_bytes": bool(torch.equal(p.cbf, torch.from_numpy(np.concatenate([foff_h, [total]])[conn_h]).to(DEV))),
        "verdicts": bool((p.verdict == rpc_amd.FRAME_OK).all()),
        "crc_equals_crc_pass": bool(torch.equal(p.crc, p.crc_alone)),
        "stream_equals_other_way": bool(torch.equal(p.out, other["stream"])),
        "scan_verify": bool(scan.nframes == n and torch.equal(scan.frame_offsets, p.fo)
                            and (scan.verdict == rpc_amd.FRAME_OK).all() and not scan.state.any()),
    }
    k = int(rng.integers(0, n))  # one frame against the host's own arithmetic
    body = src[int(soff_h[k]):int(soff_h[k] + lens_h[k])].cpu().numpy().tobytes()
    want = struct.pack(">HHII", 1, 0, len(body), zlib.crc32(body)) + body
    ok["one_frame_on_host"] = p.out[int(foff_h[k]):int(foff_h[k]) + len(want)].cpu().numpy().tobytes() == want
    other.clear()
    legs = {"pack": p.pack, "crc_pass": lambda: p.crc_pass(1024), "flat_copy": p.copy, "cumsum_gather_stamp": other_way}
    res = {"frames": n, "conns": a.conns, "total_bytes": total, "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, "a")}
    return derived(res)


def shape_b(a):
    n, blen = a.big, a.big_mib << 20
    src = torch.empty(n * blen + 64, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(src, 0xB16)
    soff_h = np.arange(n, dtype=np.int64) * blen + 3  # (an odd source offset: the funnel shift is at work)
    lens_h = np.full(n, blen, dtype=np.int64)
    foff_h = np.arange(n, dtype=np.int64) * (HDR + blen)
    total = n * (HDR + blen)
    soff, lens = torch.from_numpy(soff_h).to(DEV), torch.from_numpy(lens_h).to(DEV).to(torch.int32)
    p = Pack(src, soff, lens, torch.tensor([0, n], dtype=torch.int64, device=DEV), total, rpc_amd.FRAMES_LIFT_CAP)
    p.pack()
    p.crc_pass(blen)
    torch.cuda.synchronize()
    crc_h = p.crc_alone.cpu().numpy().view(np.uint32)
    v, _ = rpc_amd.frames_verify(p.out, p.fo, role="server", lift_cap=True)
    ok = {
        "total": int(p.total.cpu()[0]) == total,
        "offsets": bool(torch.equal(p.fo, torch.from_numpy(foff_h).to(DEV))),
        "crc_equals_crc_pass": bool(torch.equal(p.crc, p.crc_alone)),
        "headers": all(p.out[int(f):int(f) + HDR].cpu().numpy().tobytes() == struct.pack(">HHII", 1, 0, blen, int(c))
                       for f, c in zip(foff_h, crc_h)),
        "bodies": all(bool(torch.equal(p.out[int(f) + HDR:int(f) + HDR + blen], src[int(s):int(s) + blen]))
                      for f, s in zip(foff_h, soff_h)),
        "verify": bool((v == rpc_amd.FRAME_OK).all()),
    }
    legs = {"pack": p.pack, "crc_pass": lambda: p.crc_pass(blen), "flat_copy": p.copy}
    res = {"bodies": n, "body_bytes": blen, "total_bytes": total, "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, "b")}
    return derived(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--conns", type=int, default=16384)
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
