#!/usr/bin/env python3
"""tools/gather_bench.py -- rpc_crc32_device_gather on two shapes:

  (a) n bodies x 4 segments x 1 KiB, back to back (default n = 1M: 4M segments, 4 GiB);
  (b) the same segments as ONE body.

Each call is timed with device events around `reps` back-to-back calls after a
warm-up, in `rounds` rounds that alternate with rpc_crc32_device_batch over the
same segment list (the segment pass alone: the difference is the gather fold).
Shape (a) is checked against zlib on a sample of bodies, shape (b) against
rpc_crc32_device_large over the whole buffer as one body.  One JSON line.

With RPCCRC_LIB pointing at a build without the gather entry point (an older
commit, tools/ab_lib.sh) only the device_batch figure is taken.

  python tools/gather_bench.py [--bodies 1048576] [--reps 10] [--rounds 5]
"""
import argparse
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

SEG = 1024
PER_BODY = 4


def timed(fn, reps, stream):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:  # warm-up: code objects, workspace pool, clocks
        fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    n, nseg = a.bodies, a.bodies * PER_BODY
    total = nseg * SEG
    base = torch.empty(total, dtype=torch.uint8, device=dev)
    rpc_amd.fill_random(base, 0x5EED0A7)
    d_off = torch.arange(nseg, dtype=torch.int64, device=dev) * SEG
    d_len = torch.full((nseg,), SEG, dtype=torch.int32, device=dev)
    first_a = torch.arange(n + 1, dtype=torch.int64, device=dev) * PER_BODY
    first_b = torch.tensor([0, nseg], dtype=torch.int64, device=dev)
    out_a = torch.empty(n, dtype=torch.int32, device=dev)
    out_b = torch.empty(1, dtype=torch.int32, device=dev)
    out_s = torch.empty(nseg, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream()
    have_gather = _lib.rpc_crc32_device_gather is not None
    legs = {"segment_pass": lambda: rpc_amd.device_batch(base, d_off, d_len, out=out_s, max_len=SEG)}
    if have_gather:
        legs["a"] = lambda: rpc_amd.device_gather(base, d_off, d_len, first_a, out=out_a, max_seg_len=SEG)
        legs["b"] = lambda: rpc_amd.device_gather(base, d_off, d_len, first_b, out=out_b, max_seg_len=SEG)
    us = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, a.reps, s))
            print(f"gather_bench: round {r} {k}: {us[k][-1]:.1f} us", file=sys.stderr, flush=True)
    res = {"bodies": n, "segments": nseg, "segment_bytes": SEG, "bytes": total, "reps": a.reps,
           "lib": os.environ.get("RPCCRC_LIB") or "in-tree"}
    for k, v in us.items():
        res[k + "_us"] = [round(x, 1) for x in v]
        res[k + "_median_us"] = round(float(np.median(v)), 1)
    if have_gather:
        res["fold_a_us"] = round(res["a_median_us"] - res["segment_pass_median_us"], 1)
        res["fold_b_us"] = round(res["b_median_us"] - res["segment_pass_median_us"], 1)
        # the fold's HBM traffic: segment CRC written and read, length read; per body two CSR words and the CRC
        res["fold_a_floor_bytes"] = 12 * nseg + 12 * n
        res["fold_b_floor_bytes"] = 12 * nseg + 12
        got = out_a.cpu().numpy().view(np.uint32)
        rng = np.random.default_rng(7)
        bad = 0
        for i in rng.choice(n, min(n, 512), replace=False):
            body = base[int(i) * PER_BODY * SEG:(int(i) + 1) * PER_BODY * SEG].cpu().numpy().tobytes()
            bad += int(got[i]) != zlib.crc32(body)
        res["a_sample_mismatches"] = bad
        whole = rpc_amd.device_large(base, [0], [total]).cpu().numpy().view(np.uint32)
        res["b_matches_device_large"] = bool(int(out_b.cpu().numpy().view(np.uint32)[0]) == int(whole[0]))
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
