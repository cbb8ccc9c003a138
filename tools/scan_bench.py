#!/usr/bin/env python3
"""tools/scan_bench.py -- rpc_frames_scan_device on two shapes:

  (a) 16384 connections x 64 KiB of frames with JSON-like bodies of 64-1024 B, each
      ending in a partial frame: scan, and the fused scan + verify, beside
      rpc_frames_verify_device alone on the same frames;
  (b) ONE connection of 1M frames: the tiled route against the forced serial walk and
      against a single host thread walking a pinned copy of the same bytes
      (tools/scan_walk_host.c);
  --sweep: (b)-style runs over a few connection lengths, tiled against serial: the
      crossover that sets kScanTiledMin (frames_scan.h).

Device legs are timed with device events around `reps` back-to-back calls after a
warm-up, in `rounds` alternating rounds; medians are reported.  Every leg's result is
checked against what the stream was built from.  One JSON line.

  python tools/scan_bench.py [--conns 16384] [--frames 1048576] [--reps 5] [--rounds 5] [--sweep] [--skip-a] [--skip-b]
"""
import argparse
import functools
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="scan_bench")

HDR = 12
CONN_BYTES = 65536
DEV = torch.device("cuda", 0)


class Scan:
    """Preallocated outputs of one scan shape; the calls go straight to the C ABI."""

    def __init__(self, stream_t, offs, lens, cap, flags=rpc_amd.FRAMES_SERVER):
        self.s, self.offs, self.lens, self.cap, self.flags = stream_t, offs, lens, cap, flags
        n = offs.numel()
        self.n = n
        self.fo = torch.empty(cap, dtype=torch.int64, device=DEV)
        self.fc = torch.empty(cap, dtype=torch.int32, device=DEV)
        self.first = torch.empty(n + 1, dtype=torch.int64, device=DEV)
        self.consumed = torch.empty(n, dtype=torch.int64, device=DEV)
        self.state = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.nf = torch.empty(1, dtype=torch.int64, device=DEV)
        self.verdict = torch.empty(cap, dtype=torch.uint8, device=DEV)
        self.crc = torch.empty(cap, dtype=torch.int32, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def _common(self):
        return (self.s.data_ptr(), self.s.numel(), self.offs.data_ptr(), self.lens.data_ptr(), self.n, self.flags,
                self.fo.data_ptr(), self.fc.data_ptr(), self.cap, self.first.data_ptr(), self.consumed.data_ptr(),
                self.state.data_ptr(), self.nf.data_ptr())

    def scan(self):
        _lib.check(_lib.rpc_frames_scan_device(*self._common(), self.h), "scan")

    def fused(self):
        _lib.check(_lib.rpc_frames_scan_verify_device(*self._common(), self.verdict.data_ptr(), self.crc.data_ptr(),
                                                      self.h), "scan_verify")

    def verify(self):
        _lib.check(_lib.rpc_frames_verify_device(self.s.data_ptr(), self.s.numel(), self.fo.data_ptr(), self.cap,
                                                 self.flags, self.verdict.data_ptr(), self.crc.data_ptr(), self.h),
                   "verify")


def template_conn(rng):
    """64 KiB of frames with printable bodies of 64-1024 B and right CRCs; the last
    frame is cut off (a partial frame: not here yet).  -> (bytes, whole frames, consumed)"""
    out, nfr = bytearray(), 0
    while True:
        n = int(rng.integers(64, 1025))
        body = b'{"jsonrpc":"2.0","id":1,"r":"' + rng.integers(0x30, 0x7B, n - 31, dtype=np.uint8).tobytes() + b'"}'
        f = (1).to_bytes(2, "big") + (0).to_bytes(2, "big") + n.to_bytes(4, "big") + zlib.crc32(body).to_bytes(4, "big") + body
        if len(out) + len(f) > CONN_BYTES:
            consumed = len(out)
            out += f[:CONN_BYTES - len(out)]
            return bytes(out), nfr, consumed
        out += f
        nfr += 1


def leg_a(a):
    rng = np.random.default_rng(0xA)
    K = 64
    tpl = [template_conn(rng) for _ in range(K)]
    host = np.frombuffer(b"".join(t[0] for t in tpl), dtype=np.uint8).reshape(K, CONN_BYTES)
    which = torch.arange(a.conns, device=DEV) % K
    stream_t = torch.from_numpy(host.copy()).to(DEV)[which].reshape(-1).contiguous()
    offs = torch.arange(a.conns, dtype=torch.int64, device=DEV) * CONN_BYTES
    lens = torch.full((a.conns,), CONN_BYTES, dtype=torch.int64, device=DEV)
    want_frames = sum(tpl[c % K][1] for c in range(a.conns))
    sc = Scan(stream_t, offs, lens, want_frames)
    res = {"conns": a.conns, "conn_bytes": CONN_BYTES, "bytes": a.conns * CONN_BYTES, "frames": want_frames, "paths": {}}
    for path in ("serial", "tiled", "auto"):
        rpc_amd.set_scan_path(path)
        sc.fused()
        torch.cuda.synchronize()
        ok = (int(sc.nf.cpu()[0]) == want_frames and bool((sc.verdict == rpc_amd.FRAME_OK).all())
              and sc.consumed.cpu().numpy().tolist() == [tpl[c % K][2] for c in range(a.conns)]
              and not bool(sc.state.any()))
        legs = {"scan": sc.scan, "fused": sc.fused, "verify_alone": sc.verify}
        res["paths"][path] = dict(rounds_of(legs, a.reps, a.rounds, "a/" + path), correct=ok)
    rpc_amd.set_scan_path("auto")
    return res


def one_conn_stream(rng, nbytes=None, frames=None):
    """One connection of data frames with bodies of 64-1024 B, built vectorised
    (random bodies: the scan reads no body).  -> (host uint8 array, frame starts)"""
    if frames is None:
        frames = nbytes // 300
    lens = rng.integers(64, 1025, frames, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(HDR + lens)[:-1]])
    if nbytes is not None:
        keep = starts + HDR + lens <= nbytes
        starts, lens = starts[keep], lens[keep]
    total = int(starts[-1] + HDR + lens[-1])
    stream = rng.integers(0, 256, total, dtype=np.uint8)
    hdr = np.zeros((len(starts), 8), dtype=np.uint8)
    hdr[:, 1] = 1
    hdr[:, 4:8] = lens.astype(">u4").view(np.uint8).reshape(-1, 4)
    stream[starts[:, None] + np.arange(8)[None, :]] = hdr
    return stream, starts


def one_conn_legs(host, starts, reps, rounds, tag, host_walk):
    stream_t = torch.from_numpy(host).to(DEV)
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    lens = torch.full((1,), host.size, dtype=torch.int64, device=DEV)
    sc = Scan(stream_t, offs, lens, len(starts))
    want = torch.from_numpy(starts).to(DEV)
    res = {"bytes": int(host.size), "frames": int(len(starts))}
    legs = {}
    for path in ("tiled", "serial"):
        rpc_amd.set_scan_path(path)
        sc.fo.zero_()
        sc.scan()
        torch.cuda.synchronize()
        res[path + "_correct"] = bool(int(sc.nf.cpu()[0]) == len(starts) and torch.equal(sc.fo, want)
                                      and int(sc.consumed.cpu()[0]) == host.size)

        def leg(path=path):
            rpc_amd.set_scan_path(path)
            sc.scan()
        legs[path] = leg
    res.update(rounds_of(legs, reps, rounds, tag))
    rpc_amd.set_scan_path("auto")
    if host_walk:
        lib = ctypes.CDLL(os.path.join(REPO, "tools", "libscanwalk.so"))
        lib.scan_walk_host.restype = ctypes.c_uint64
        lib.scan_walk_host.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p, ctypes.c_void_p]
        pinned = torch.from_numpy(host).pin_memory()
        out = torch.empty(len(starts), dtype=torch.int64).pin_memory()
        consumed, state = ctypes.c_uint64(0), ctypes.c_uint8(0)
        ts = []
        for _ in range(rounds + 1):
            t0 = time.perf_counter()
            n = lib.scan_walk_host(pinned.data_ptr(), host.size, rpc_amd.FRAMES_SERVER, out.data_ptr(), len(starts),
                                   ctypes.byref(consumed), ctypes.byref(state))
            ts.append((time.perf_counter() - t0) * 1e6)
        res["host_walk"] = {"us": [round(x, 1) for x in ts[1:]], "median_us": round(float(np.median(ts[1:])), 1),
                            "correct": bool(n == len(starts) and np.array_equal(out.numpy(), starts))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=16384)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"lib": os.environ.get("RPCCRC_LIB") or "in-tree", "reps": a.reps, "rounds": a.rounds}
    if not a.skip_a:
        res["a"] = leg_a(a)
    if not a.skip_b:
        host, starts = one_conn_stream(np.random.default_rng(0xB), frames=a.frames)
        res["b"] = one_conn_legs(host, starts, max(1, a.reps // 2), a.rounds, "b", True)
    if a.sweep:
        res["sweep"] = []
        for kib in (64, 128, 256, 512, 1024, 2048, 4096, 16384):
            host, starts = one_conn_stream(np.random.default_rng(kib), nbytes=kib << 10)
            r = one_conn_legs(host, starts, a.reps, a.rounds, f"sweep/{kib}K", False)
            res["sweep"].append(dict(r, kib=kib))
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
