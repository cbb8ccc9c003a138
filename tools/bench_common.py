"""What the stage benchmarks (pack_, unpack_, carry_, scan_, route_, resolve_, reply_, request_ and
values_bench.py) share: device time per call of one leg, and the rounds over interleaved legs."""
import sys
import time

import numpy as np
import torch


def timed(fn, reps, stream, warm=0.2):
    t0 = time.perf_counter()
    while True:  # warm-up: code objects, workspace pool, clocks
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= warm:
            break
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def rounds_of(legs, reps, rounds, tag, name):
    """``rounds`` rounds over the legs in turn; ``name`` is the tool's prefix of the progress line."""
    us = {k: [] for k in legs}
    s = torch.cuda.current_stream()
    for r in range(rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, reps, s))
            print(f"{name}: {tag} round {r} {k}: {us[k][-1]:.1f} us", file=sys.stderr, flush=True)
    return {k: {"us": [round(x, 1) for x in v], "median_us": round(float(np.median(v)), 1)} for k, v in us.items()}
