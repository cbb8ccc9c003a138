#!/usr/bin/env python3
"""tools/results_bench.py -- rpc_frames_results_device on the resolve bench's replies (DESIGN.md
4.21):

  (a) tools/resolve_bench.py's shape (a): about 1.9M reply bodies of 40-90 bytes with distinct
      ids against as many pending ids, every slot matched; the results decode every `result`
      by the type of the method the slot was sent with (1 % of the replies are errors: no
      `result`, the `error` member decoded) and leave the completions per slot;
  (b) the same replies resolved with npending == 0: no entry is MATCHED, the NONE path.

Legs: the results call; the resolve on the same entries (the join in (a), decode only in (b));
and the host loop the call replaces, timed on 65,536 replies and reported per reply: one D2H of
those bodies, then json.loads of each `result` span and the conversion the generated client
makes (host wall time; the device legs are device time).

Device legs are timed with device events around `reps` back-to-back calls after a warm-up, in
`rounds` alternating rounds; medians are reported.  Every leg's output is checked before its
number is written down: the first 65,536 entries and the slots they complete against the plain
rules of tests/results_cases.py, all entries against what the bodies were built from.  One JSON
line.

  python tools/results_bench.py [--entries 1900000] [--reps 5] [--rounds 3] [--skip-a] [--skip-b]
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
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402
import resolve_bench as rb  # noqa: E402
import results_cases as rs  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="results_bench")

DEV, K, HOST_BODIES = rb.DEV, rb.K, rb.HOST_BODIES
#: the result type of the resolve bench's seven value texts (add_i32's sum of two i32 may leave
#: int32: it is read as an I64 from a number); an error reply's slot is given method 0
TYPES = [rs.STR, rs.I64, rs.I64, rs.F64, rs.BOOL, rs.I32, rs.STR]


class Results:
    """Preallocated outputs of one results shape; the calls go straight to the C ABI."""

    def __init__(self, r, pending_method):
        self.r, self.pm = r, pending_method
        n, npend = r.n, r.npend
        self.types = torch.tensor(TYPES, dtype=torch.uint8, device=DEV)
        self.status, self.estatus = (torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(2))
        self.value, self.emsg = (torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(2))
        self.ecode = torch.empty(n, dtype=torch.int32, device=DEV)
        self.s_status, self.s_estatus = (torch.empty(max(npend, 1), dtype=torch.uint8, device=DEV) for _ in range(2))
        self.s_value, self.s_base = (torch.empty(max(npend, 1), dtype=torch.int64, device=DEV) for _ in range(2))
        self.s_ecode = torch.empty(max(npend, 1), dtype=torch.int32, device=DEV)
        self.ndefer = torch.empty(1, dtype=torch.int32, device=DEV)

    def call(self):
        r = self.r
        _lib.check(_lib.rpc_frames_results_device(
            r.b.data_ptr(), r.b.numel(), r.off.data_ptr(), r.len.data_ptr(), r.kind.data_ptr(), r.slot.data_ptr(),
            r.roff.data_ptr(), r.rlen.data_ptr(), r.eoff.data_ptr(), r.elen.data_ptr(), r.slot_entry.data_ptr(), r.n,
            self.pm.data_ptr() if r.npend else None, r.npend, self.types.data_ptr(), len(TYPES), self.status.data_ptr(),
            self.value.data_ptr(), self.estatus.data_ptr(), self.ecode.data_ptr(), self.emsg.data_ptr(),
            self.s_status.data_ptr(), self.s_value.data_ptr(), self.s_estatus.data_ptr(), self.s_ecode.data_ptr(),
            self.s_base.data_ptr(), self.ndefer.data_ptr(), r.h), "results")


def against_the_rules(x, nk):
    """The first nk entries, and the slots they complete, against tests/results_cases.py."""
    r = x.r
    end = int(r.off[nk - 1].item()) + int(r.len[nk - 1].item())
    host = r.b[:end].cpu().numpy().tobytes()
    u = lambda t, d: t[:nk].cpu().numpy().view(d).tolist()  # noqa: E731
    entries = list(zip(u(r.off, np.uint64), u(r.len, np.uint32), u(r.kind, np.uint8), u(r.slot, np.uint32),
                       u(r.roff, np.uint32), u(r.rlen, np.uint32), u(r.eoff, np.uint32), u(r.elen, np.uint32)))
    pm = x.pm.cpu().numpy().view(np.uint16).tolist() if r.npend else []
    want = rs.results_entries(host, entries, pm, TYPES)
    got = [rs.Row(*g) for g in zip(u(x.status, np.uint8), u(x.value, np.uint64), u(x.estatus, np.uint8),
                                   u(x.ecode, np.int32), u(x.emsg, np.uint64))]
    ok = got == want
    if r.npend:  # the slots these entries complete (each entry is its slot's: the bench's ids are distinct)
        sl = torch.tensor([e[3] for e in entries], device=DEV)
        s = lambda t, d: t[sl].cpu().numpy().view(d).tolist()  # noqa: E731
        slots = list(zip(s(x.s_status, np.uint8), s(x.s_value, np.uint64), s(x.s_estatus, np.uint8),
                         s(x.s_ecode, np.int32), s(x.s_base, np.uint64)))
        ok = ok and slots == [(w.status, w.value, w.error_status, w.error_code, e[0]) for w, e in zip(want, entries)]
    return ok


def host_way(x, vals, is_err, nk):
    """One D2H of nk bodies, then per reply json.loads of the `result` span and the generated
    client's conversion.  -> (ns per reply, ok)"""
    r = x.r
    end = int(r.off[nk - 1].item()) + int(r.len[nk - 1].item())
    offs, ro, rl = (t[:nk].cpu().tolist() for t in (r.off, r.roff, r.rlen))
    which = [k % K for k in range(nk)]
    types = [TYPES[m] for m in rb_methods(vals, is_err)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = r.b[:end].cpu().numpy().tobytes()
    got = []
    for o, a, b, k in zip(offs, ro, rl, which):
        if not b:
            got.append(None)
            continue
        v, t = json.loads(host[o + a:o + a + b]), types[k]
        if t == rs.STR:
            got.append(v if isinstance(v, str) else None)
        elif t == rs.I64:
            got.append(int(v) if isinstance(v, (str, int, float)) and not isinstance(v, bool) else 0)
        elif t == rs.I32:
            got.append(int(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else 0)
        elif t == rs.F64:
            got.append(float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else 0.0)
        else:
            got.append(v is True)
    dt = time.perf_counter() - t0
    ok = all((g is None) == is_err[k] and (is_err[k] or g == json.loads(vals[k]) or str(g) == json.loads(vals[k]))
             for g, k in zip(got, which))
    return dt * 1e9 / nk, ok


def rb_methods(vals, is_err):
    """The method of each template entry, read back from its value text: the resolve bench keeps
    the texts, not the methods.  (A string of digits is echo_i64's, "pong" ping's, any other
    string mix3's; true / false is is_even's; a number with '.' or 'e' mul_double's; an integer
    up to 1,024 strlen_s's, which add_i32's sums are told from only by the type they are read
    as -- I64 takes both.)"""
    out = []
    for v, e in zip(vals, is_err):
        if e:
            out.append(0)
        elif v == b'"pong"':
            out.append(0)
        elif v[:1] == b'"':
            out.append(1 if v[1:-1].lstrip(b"-").isdigit() else 6)
        elif v in (b"true", b"false"):
            out.append(4)
        elif b"." in v or b"e" in v:
            out.append(3)
        else:
            out.append(2)
    return out


def run_shape(tag, built, join, a):
    bodies, offs, lens, ids, is_err, vals = built
    n = offs.numel()
    g = torch.Generator(device="cpu").manual_seed(0xC)
    pending = ids[torch.randperm(n, generator=g).to(DEV)].to(torch.int32).contiguous() if join else \
        torch.empty(0, dtype=torch.int32, device=DEV)
    r = rb.Resolve(bodies, offs, lens, pending)
    r.call()
    torch.cuda.synchronize()
    which = torch.arange(n, device=DEV) % K
    meth = torch.tensor(rb_methods(vals, is_err), dtype=torch.int16, device=DEV)
    pm = torch.zeros(max(r.npend, 1), dtype=torch.int16, device=DEV)
    if join:
        pm[r.slot.to(torch.int64)] = meth[which]
    x = Results(r, pm)
    x.call()
    torch.cuda.synchronize()
    nk = min(HOST_BODIES, n)
    err = torch.tensor(is_err, device=DEV)[which]
    ok = {"first_entries_match_the_rules": against_the_rules(x, nk), "ndefer": int(x.ndefer.item()) == 0}
    if join:
        ok["every_result_ok"] = bool(torch.equal(x.status == rpc_amd.RESULTS_OK, ~err)) and \
            bool(torch.equal(x.status == rpc_amd.RESULTS_ABSENT, err))
        ok["every_error_ok"] = bool(torch.equal(x.estatus == rpc_amd.RESULTS_OK, err)) and \
            bool((x.ecode[err] == -32601).all()) and bool((x.ecode[~err] == 0).all())
        sl = r.slot.to(torch.int64)
        ok["slots_hold_their_entries"] = bool(torch.equal(x.s_value[sl], x.value)) and \
            bool(torch.equal(x.s_status[sl], x.status)) and bool(torch.equal(x.s_base[sl], offs.to(torch.int64)))
    else:
        ok["all_none"] = bool((x.status == rpc_amd.RESULTS_NONE).all()) and bool((x.value == 0).all()) and \
            bool((x.estatus == rpc_amd.RESULTS_ABSENT).all())
    legs = {"results": x.call, "resolve": r.call}
    res = {"entries": n, "npending": r.npend, "bytes": bodies.numel(), "correct": ok,
           "legs": rounds_of(legs, a.reps, a.rounds, tag)}
    m = {k: v["median_us"] for k, v in res["legs"].items()}
    res["results_over_resolve"] = round(m["results"] / m["resolve"], 3)
    res["results_ns_per_reply"] = round(m["results"] * 1e3 / n, 3)
    if join:
        ns, host_ok = host_way(x, vals, is_err, nk)
        ok["host_way"] = host_ok
        res["host_loop_ns_per_reply"] = round(ns, 1)
        res["host_loop_replies"] = nk
        res["host_loop_for_all_entries_over_results"] = round(ns * 1e-3 * n / m["results"], 1)
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
    built = rb.build(a.entries)
    if not a.skip_a:
        res["a"] = run_shape("a", built, True, a)
    if not a.skip_b:
        res["b"] = run_shape("b", built, False, a)
    res["status"] = rpc_amd.device_status()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
