#!/usr/bin/env python3
"""tools/unpack_bench.py -- rpc_frames_unpack_device on two shapes:

  (a) the scan bench's 16384 connections x 64 KiB of frames with bodies of 64-1024 B,
      each ending in a partial frame, through the fused scan + verify and then unpack;
  (b) RPC_FRAMES_LIFT_CAP, 16 frames with bodies of 64 MiB at odd stream offsets.

Legs: the unpack call (nul = 1); a flat device-to-device copy of `total` bytes
(Tensor.copy_: the floor of the copy stage); and the way without unpack: a header gather,
torch.cumsum for the layout and a per-byte index gather for the bodies.

Device legs are timed with device events around `reps` back-to-back calls after a
warm-up, in `rounds` alternating rounds; medians are reported.  Every leg's result is
checked: unpack's outputs against what the stream was built from and, byte for byte and
word for word, against what the other way builds.  One JSON line.

  python tools/unpack_bench.py [--conns 16384] [--big 16] [--big-mib 64] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
"""
import argparse
import functools
import json
import os
import sys
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="unpack_bench")

HDR = 12
CONN_BYTES = 65536
DEV = torch.device("cuda", 0)
NUL = 1


class Unpack:
    """Preallocated outputs of one unpack shape; the calls go straight to the C ABI."""

    def __init__(self, stream_t, fo, verdict, conn_first, total, flags):
        self.s, self.fo, self.v, self.conn_first, self.flags = stream_t, fo, verdict, conn_first, flags
        n = fo.numel()
        self.n = n
        self.out = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.boff = torch.empty(n, dtype=torch.int64, device=DEV)
        self.blen = torch.empty(n, dtype=torch.int32, device=DEV)
        self.rtype = torch.empty(n, dtype=torch.int16, device=DEV)
        self.ver = torch.empty(n, dtype=torch.int16, device=DEV)
        self.vout = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.cbf = torch.empty(conn_first.numel(), dtype=torch.int64, device=DEV)
        self.total = torch.empty(1, dtype=torch.int64, device=DEV)
        self.copy_src = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.copy_dst = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.h = rpc_amd._stream_handle(None)

    def unpack(self):
        _lib.check(_lib.rpc_frames_unpack_device(self.s.data_ptr(), self.s.numel(), self.fo.data_ptr(), self.v.data_ptr(),
                                                 self.n, self.conn_first.data_ptr(), self.conn_first.numel() - 1,
                                                 self.flags, NUL, self.out.data_ptr(), self.out.numel(),
                                                 self.boff.data_ptr(), self.blen.data_ptr(), self.rtype.data_ptr(),
                                                 self.ver.data_ptr(), self.vout.data_ptr(), self.cbf.data_ptr(),
                                                 self.total.data_ptr(), self.h), "unpack")

    def copy(self):
        self.copy_dst.copy_(self.copy_src)


def other_way(stream_t, fo, verdict, total, keep):
    """The way without unpack: a header gather, cumsum for the layout, a per-byte index gather
    for the bodies (no check of the verdicts against the headers: every frame here is in
    range).  server role."""
    n = fo.numel()
    ok = verdict == rpc_amd.FRAME_OK
    ctl = verdict == rpc_amd.FRAME_CONTROL
    at_hdr = torch.where(ok | ctl, fo, torch.zeros_like(fo))
    hdr = stream_t[at_hdr[:, None] + torch.arange(8, device=DEV)[None, :]].to(torch.int64)
    ver = torch.where(ok | ctl, (hdr[:, 0] << 8) | hdr[:, 1], torch.zeros_like(fo))
    blen = (hdr[:, 4] << 24) | (hdr[:, 5] << 16) | (hdr[:, 6] << 8) | hdr[:, 7]
    lens = torch.where(ok, blen, torch.zeros_like(blen))
    sizes = lens + NUL * ok.to(torch.int64)
    boff = torch.cumsum(sizes, 0) - sizes
    bstart = torch.cumsum(lens, 0) - lens
    nbody = total - NUL * int(ok.sum())  # (one read-back the unpack's caller with an `out` does not need)
    entry_of = torch.repeat_interleave(torch.arange(n, device=DEV), lens, output_size=nbody)
    at = torch.arange(nbody, device=DEV)
    out = torch.zeros(total, dtype=torch.uint8, device=DEV)
    out[at + (boff - bstart)[entry_of]] = stream_t[at + (fo + HDR - bstart)[entry_of]]
    none = torch.full_like(fo, rpc_amd.TYPE_NONE)
    rtype = torch.where(ok, torch.zeros_like(fo), torch.where(ctl, torch.full_like(fo, rpc_amd.RPC_TYPE_PONG), none))
    if keep is not None:
        keep.update(out=out, boff=boff, lens=lens, ver=ver, rtype=rtype)


def agree(u, keep):
    return {
        "bodies_equal_other_way": bool(torch.equal(u.out, keep["out"])),
        "offsets_equal_other_way": bool(torch.equal(u.boff, keep["boff"])),
        "lens_equal_other_way": bool(torch.equal(u.blen.to(torch.int64), keep["lens"])),
        "versions_equal_other_way": bool(torch.equal(u.ver.to(torch.int64) & 0xFFFF, keep["ver"])),
        "types_equal_other_way": bool(torch.equal(u.rtype.to(torch.int64) & 0xFFFF, keep["rtype"])),
        "verdicts_unchanged": bool(torch.equal(u.vout, u.v)),
    }


def derived(res):
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["unpack_over_flat_copy"] = round(m["unpack"] / m["flat_copy"], 2)
    res["other_way_over_unpack"] = round(m["header_cumsum_gather"] / m["unpack"], 2)
    return res


def template_conn(rng):
    """64 KiB of frames with printable bodies of 64-1024 B and right CRCs; the last frame is
    cut off (tools/scan_bench.py's connection).  -> (bytes, body lengths of the whole frames)"""
    out, lens = bytearray(), []
    while True:
        n = int(rng.integers(64, 1025))
        body = b'{"jsonrpc":"2.0","id":1,"r":"' + rng.integers(0x30, 0x7B, n - 31, dtype=np.uint8).tobytes() + b'"}'
        f = (1).to_bytes(2, "big") + (0).to_bytes(2, "big") + n.to_bytes(4, "big") + zlib.crc32(body).to_bytes(4, "big") + body
        if len(out) + len(f) > CONN_BYTES:
            out += f[:CONN_BYTES - len(out)]
            return bytes(out), lens
        out += f
        lens.append(n)


def shape_a(a):
    rng = np.random.default_rng(0xA)
    K = 64
    tpl = [template_conn(rng) for _ in range(K)]
    host = np.frombuffer(b"".join(t[0] for t in tpl), dtype=np.uint8).reshape(K, CONN_BYTES)
    which = torch.arange(a.conns, device=DEV) % K
    stream_t = torch.from_numpy(host.copy()).to(DEV)[which].reshape(-1).contiguous()
    offs = torch.arange(a.conns, dtype=torch.int64, device=DEV) * CONN_BYTES
    lens = torch.full((a.conns,), CONN_BYTES, dtype=torch.int64, device=DEV)
    nframes = sum(len(tpl[c % K][1]) for c in range(a.conns))
    total = sum(sum(tpl[c % K][1]) + NUL * len(tpl[c % K][1]) for c in range(a.conns))
    pad = 1000  # the padded frame_cap a server would scan with
    sc = rpc_amd.frames_scan(stream_t, offs, lens, role="server", verify=True, max_frames=nframes + pad)
    u = Unpack(stream_t, sc.frame_offsets, sc.verdict, sc.conn_first, total, rpc_amd.FRAMES_SERVER)
    keep = {}
    u.unpack()
    other_way(stream_t, u.fo, u.v, total, keep)
    torch.cuda.synchronize()
    ok = {"scan": sc.nframes == nframes, "total": int(u.total.cpu()[0]) == total}
    ok.update(agree(u, keep))
    ok["types"] = bool((u.rtype[:nframes] == 0).all() and (u.rtype[nframes:] == -1).all())
    c = int(rng.integers(0, a.conns))  # one connection against the host's own bytes
    cbf = u.cbf.cpu().tolist()
    t, want, at = tpl[c % K], b"", 0
    for n in t[1]:
        want += t[0][at + HDR:at + HDR + n] + b"\0" * NUL
        at += HDR + n
    ok["one_connection_on_host"] = u.out[cbf[c]:cbf[c + 1]].cpu().numpy().tobytes() == want
    keep.clear()
    torch.cuda.empty_cache()
    legs = {"unpack": u.unpack, "flat_copy": u.copy,
            "header_cumsum_gather": lambda: other_way(stream_t, u.fo, u.v, total, None)}
    res = {"conns": a.conns, "conn_bytes": CONN_BYTES, "stream_bytes": a.conns * CONN_BYTES, "frames": nframes,
           "entries": nframes + pad, "total_bytes": total, "correct": ok, "legs": rounds_of(legs, a.reps, a.rounds, "a")}
    return derived(res)


def shape_b(a):
    n, blen = a.big, a.big_mib << 20
    step = HDR + blen + 2
    stream_t = torch.empty((n * step + 64) & ~7, dtype=torch.uint8, device=DEV)  # (fill_random writes whole 8-byte words)
    rpc_amd.fill_random(stream_t, 0xB16)
    fo = torch.arange(n, dtype=torch.int64, device=DEV) * step + 1  # (odd offsets: the funnel shift is at work)
    blens = torch.full((n,), blen, dtype=torch.int32, device=DEV)
    stamped = rpc_amd.frames_stamp(stream_t, fo, blens, lift_cap=True)
    v, _ = rpc_amd.frames_verify(stream_t, fo, role="server", lift_cap=True)
    total = n * (blen + NUL)
    u = Unpack(stream_t, fo, v, torch.tensor([0, n], dtype=torch.int64, device=DEV), total,
               rpc_amd.FRAMES_SERVER | rpc_amd.FRAMES_LIFT_CAP)
    keep = {}
    u.unpack()
    other_way(stream_t, fo, v, total, keep)
    torch.cuda.synchronize()
    ok = {"stamped_and_verified": bool((stamped == rpc_amd.FRAME_OK).all() and (v == rpc_amd.FRAME_OK).all()),
          "total": int(u.total.cpu()[0]) == total}
    ok.update(agree(u, keep))
    ok["bodies"] = all(bool(torch.equal(u.out[i * (blen + NUL):i * (blen + NUL) + blen],
                                        stream_t[i * step + 1 + HDR:i * step + 1 + HDR + blen])) for i in range(n))
    ok["nuls"] = bool((u.out[blen::blen + NUL] == 0).all())
    keep.clear()
    torch.cuda.empty_cache()
    legs = {"unpack": u.unpack, "flat_copy": u.copy, "header_cumsum_gather": lambda: other_way(stream_t, fo, v, total, None)}
    res = {"bodies": n, "body_bytes": blen, "total_bytes": total, "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, "b")}
    return derived(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=16384)
    ap.add_argument("--big", type=int, default=16)
    ap.add_argument("--big-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"lib": os.environ.get("RPCCRC_LIB") or "in-tree", "reps": a.reps, "rounds": a.rounds, "nul": NUL}
    if not a.skip_a:
        res["a"] = shape_a(a)
        torch.cuda.empty_cache()
    if not a.skip_b:
        res["b"] = shape_b(a)
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
