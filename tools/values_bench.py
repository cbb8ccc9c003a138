#!/usr/bin/env python3
"""tools/values_bench.py -- rpc_frames_values_device on four shapes:

  (a) the reply bench's entry count and method mix: about 1.9M results, 64 % strlen_s (a length),
      35 % the other six methods ("pong", a quoted 64-bit number, a sum, a double, true / false,
      a quoted triple), typed slots in, value text out;
  (b) 1.9M F64 results of random bits (the 17-digit class) against 1.9M of k / 10^j with
      k < 10^15 (the 15-digit class);
  (c) 16 strings of 64 MiB each, at odd offsets of the strings buffer;
  (d) 1.9M PARAMS objects in the same method mix over the IDL's schema.

Legs per shape: the values call; rpc_frames_reply_device on the same entries (the values' own
output as its values); a flat device-to-device copy of the output bytes (Tensor.copy_); and the
host loop the call replaces, timed on 65,536 entries and reported per entry: json.dumps per
value, and '%.15g' / float / '%.17g' for the reference-exact double (host wall time, without the
upload; the device legs are device time).

Device legs are timed with device events around `reps` back-to-back calls after a warm-up, in
`rounds` alternating rounds; medians are reported.  Every leg's output is checked: the first
65,536 entries byte for byte against the host loop's texts (tests/values_cases.py's rules), the
total against the lengths, the big strings against their source.  One JSON line.

  python tools/values_bench.py [--entries 1900000] [--big 16] [--big-mib 64] [--reps 5] [--rounds 3] [--skip abcd]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import rpc_amd  # noqa: E402
from rpc_amd import _lib  # noqa: E402
import bench_common  # noqa: E402

rounds_of = functools.partial(bench_common.rounds_of, name="values_bench")
import args_cases as ac  # noqa: E402
import values_cases as vc  # noqa: E402

DEV = torch.device("cuda", 0)
HOST_ENTRIES = 65536
K = 4096  # template entries
RTYPES = [vc.STR, vc.I64, vc.I32, vc.F64, vc.BOOL, vc.I32, vc.STR]  # what the seven handlers return


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Values:
    """Preallocated outputs of one shape; the calls go straight to the C ABI."""

    def __init__(self, form, method, slots, schema, strings):
        self.form, self.method, self.slots, self.schema, self.strings = form, method, slots, schema, strings
        n = self.n = method.numel()
        self.width = slots.shape[0]
        self.voff = torch.empty(n, dtype=torch.int64, device=DEV)
        self.vlen = torch.empty(n, dtype=torch.int32, device=DEV)
        self.state = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.rstat = torch.empty(n, dtype=torch.int32, device=DEV)
        self.ndefer = torch.empty(1, dtype=torch.int32, device=DEV)
        self.total = torch.empty(1, dtype=torch.int64, device=DEV)
        self.h = rpc_amd._stream_handle(None)
        self.out = None
        self.call()  # layout only
        torch.cuda.synchronize()
        nb = int(self.total.cpu()[0])
        self.out = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.copy_src = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.copy_dst = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.rid = torch.arange(n, dtype=torch.int32, device=DEV)
        self.r_out = torch.empty(nb + 64 * n, dtype=torch.uint8, device=DEV)
        self.r_off = torch.empty(n, dtype=torch.int64, device=DEV)
        self.r_len = torch.empty(n, dtype=torch.int32, device=DEV)
        self.r_total = torch.empty(1, dtype=torch.int64, device=DEV)

    def call(self):
        if self.form == vc.FORM_PARAMS:
            s = self.schema
            sch = (None, s.first.data_ptr(), s.nmethods, s.types.data_ptr(), s.name_off.data_ptr(), s.nparams,
                   s.names.data_ptr(), s.names.numel())
        else:
            sch = (self.schema.data_ptr(), None, self.schema.numel(), None, None, 0, None, 0)
        out = self.out
        _lib.check(_lib.rpc_frames_values_device(self.form, None, None, self.method.data_ptr(), self.slots.data_ptr(),
                                                 self.width, self.n, *sch, self.strings.data_ptr(), self.strings.numel(),
                                                 None, None, 0, None, None, None if out is None else out.data_ptr(),
                                                 0 if out is None else out.numel(), self.voff.data_ptr(),
                                                 self.vlen.data_ptr(), self.state.data_ptr(), self.rstat.data_ptr(),
                                                 self.ndefer.data_ptr(), self.total.data_ptr(), self.h), "values")

    def reply(self):
        _lib.check(_lib.rpc_frames_reply_device(None, self.rid.data_ptr(), None, None, self.n, self.out.data_ptr(),
                                                self.out.numel(), self.voff.data_ptr(), self.vlen.data_ptr(), None, 0,
                                                self.r_out.data_ptr(), self.r_out.numel(), self.r_off.data_ptr(),
                                                self.r_len.data_ptr(), None, None, None, self.r_total.data_ptr(), self.h),
                   "reply")

    def copy(self):
        self.copy_dst.copy_(self.copy_src)


def exact_double(d):
    t = "%.15g" % d
    r = float(t)
    return t if abs(r - d) <= max(abs(r), abs(d)) * 2.0 ** -52 else "%.17g" % d


def host_loop(values):
    """The loop the call replaces: one text per typed value.  values: [(type, python value)]."""
    t0 = time.perf_counter()
    texts = [json.dumps(v).encode() if t != vc.F64 else exact_double(v).encode() for t, v in values]
    b"".join(texts)
    return (time.perf_counter() - t0) * 1e6, texts


def other_legs_ok(v, h):
    """The reply leg's and the flat copy's outputs: every reply length and the total against the
    values' lengths, the first h reply bodies byte for byte against the reply's rule around the
    values' own texts (reply_cases.result_body), the copy's destination against its source."""
    import reply_cases as rp
    v.call()
    v.reply()
    v.copy_src.copy_(v.out)
    v.copy()
    torch.cuda.synchronize()
    n = v.n
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    digits = sum((ids >= 10 ** p).to(torch.int64) for p in range(1, 10)) + 1
    vlen = v.vlen.to(torch.int64) & 0xFFFFFFFF
    want_len = len('{"jsonrpc":"2.0","id":,"result":}') + digits + torch.where(vlen == 0, torch.full_like(vlen, 4), vlen)
    ok = {"reply_lens": bool(torch.equal(v.r_len.to(torch.int64) & 0xFFFFFFFF, want_len)),
          "reply_total": int(v.r_total.cpu()[0]) == int(want_len.sum()),
          "reply_offsets": bool(torch.equal(v.r_off, torch.cumsum(want_len, 0) - want_len)),
          "copy_equals_source": bool(torch.equal(v.copy_dst, v.out))}
    off, ln = v.voff[:h].cpu().numpy(), v.vlen[:h].cpu().numpy().view(np.uint32)
    ro, rl = v.r_off[:h].cpu().numpy(), v.r_len[:h].cpu().numpy().view(np.uint32)
    if int(ln.max()) <= 4096:  # (the big strings: the envelope's bytes only, below)
        texts = v.out[:int(off[-1] + ln[-1])].cpu().numpy().tobytes()
        bodies = v.r_out[:int(ro[-1] + rl[-1])].cpu().numpy().tobytes()
        ok["reply_head_bytes"] = all(bodies[int(ro[i]):int(ro[i]) + int(rl[i])] ==
                                     rp.result_body(i, texts[int(off[i]):int(off[i]) + int(ln[i])]) for i in range(h))
    else:
        same = True
        for i in range(h):
            front = b'{"jsonrpc":"2.0","id":%d,"result":' % i
            o, k = int(ro[i]), int(rl[i])
            same &= v.r_out[o:o + len(front)].cpu().numpy().tobytes() == front and v.r_out[o + k - 1].item() == ord("}")
            same &= bool(torch.equal(v.r_out[o + len(front):o + k - 1], v.out[int(off[i]):int(off[i]) + int(ln[i])]))
        ok["reply_bodies"] = same
    return ok


def report(v, n, tag, a, host, want_head, host_is_rules=True, host_what=None):
    """Runs and checks one shape.  want_head: the rules' texts of the first entries; host(): the
    host loop on those entries, (microseconds, texts)."""
    v.call()
    torch.cuda.synchronize()
    h = len(want_head)
    off, ln = v.voff[:h].cpu().numpy(), v.vlen[:h].cpu().numpy().view(np.uint32)
    nb = int(off[-1] + ln[-1])
    head = v.out[:nb].cpu().numpy().tobytes()
    ok = {"total": int(v.total.cpu()[0]) == int(v.vlen.to(torch.int64).sum()) == v.out.numel(),
          "ndefer": int(v.ndefer.cpu()[0]),
          "states_ok": bool(((v.state == vc.OK) | (v.state == vc.DEFER)).all()),
          "head_bytes_equal_rules": all(head[int(o):int(o) + int(k)] == w for o, k, w in zip(off, ln, want_head))}
    ok.update(other_legs_ok(v, h))
    host_runs = []
    for _ in range(a.rounds):
        us, texts = host()
        host_runs.append(us)
    if host_is_rules:
        ok["host_loop_equal_rules"] = texts == list(want_head)
    out = rounds_of({"values": v.call, "reply_same_entries": v.reply, "flat_copy": v.copy}, a.reps, a.rounds, tag)
    med = float(np.median(host_runs))
    out["host_loop"] = {"entries": h, "us": [round(x, 1) for x in host_runs], "median_us": round(med, 1),
                        "ns_per_entry": round(med * 1e3 / h, 1), "scaled_to_all_entries_us": round(med * n / h, 1)}
    if host_what:
        out["host_loop"]["what"] = host_what
    m = {k: x["median_us"] for k, x in out.items()}
    return {"entries": n, "total_bytes": int(v.out.numel()), "correct": ok, "legs": out,
            "values_over_flat_copy": round(m["values"] / m["flat_copy"], 2),
            "values_over_reply": round(m["values"] / m["reply_same_entries"], 2),
            "values_ns_per_entry": round(m["values"] * 1e3 / n, 3),
            "host_loop_over_values": round(out["host_loop"]["scaled_to_all_entries_us"] / m["values"], 1)}


def mix_template(rng):
    """K entries in the route bench's mix: (method, typed python values per parameter, result)."""
    meth = []
    for _ in range(K):
        u = rng.random()
        meth.append(5 if u < 0.64 else (0, 1, 2, 3, 4, 6)[int(rng.integers(0, 6))])
    return meth


def shape_a(a):
    rng = np.random.default_rng(0xA)
    n = a.entries
    meth = mix_template(rng)
    strings = bytearray(b"pong")
    slot, pyv = [], []
    dbl = [0.5, -1.25, 3.0, 1e20, 2.5e-7, 12345.678, 0.1, 1.0 / 3.0]
    for m in meth:
        if m == 0:
            slot.append(0 | 4 << 32), pyv.append((vc.STR, "pong"))
        elif m == 1:
            x = int(rng.integers(-2**62, 2**62))
            slot.append(x & vc.M64), pyv.append((vc.I64, str(x)))
        elif m in (2, 5):
            x = int(rng.integers(-2**31, 2**31)) if m == 2 else int(rng.integers(0, 1025))
            slot.append(x & vc.M64), pyv.append((vc.I32, x))
        elif m == 3:
            d = dbl[int(rng.integers(0, 8))] * dbl[int(rng.integers(0, 8))]
            slot.append(vc.bits_of(d)), pyv.append((vc.F64, d))
        elif m == 4:
            b = bool(rng.integers(0, 2))
            slot.append(int(b)), pyv.append((vc.BOOL, b))
        else:
            t = "%d:%g:%s" % (int(rng.integers(-2**31, 2**31)), dbl[int(rng.integers(0, 8))], "true")
            slot.append(len(strings) | len(t) << 32), pyv.append((vc.STR, t))
            strings += t.encode()
    i = torch.arange(n, dtype=torch.int64, device=DEV) % K
    method = dev(np.array(meth, dtype=np.int16))[i].contiguous()
    slots = dev(np.array(slot, dtype=np.uint64).view(np.int64))[i].reshape(1, n).contiguous()
    v = Values(vc.FORM_RESULT, method, slots, dev(np.array(RTYPES, dtype=np.uint8)), dev(np.frombuffer(bytes(strings), np.uint8)))
    h = min(HOST_ENTRIES, n)
    want = [vc.value_text(RTYPES[meth[j % K]], slot[j % K], 0, bytes(strings))[1] for j in range(h)]
    hv = [pyv[j % K] for j in range(h)]
    return report(v, n, "a", a, lambda: host_loop(hv), want)


def shape_b(a):
    n = a.entries
    g = torch.Generator(device=DEV).manual_seed(0xB)
    res = {}
    for tag in ("random_bits", "class15"):
        if tag == "random_bits":
            frac = torch.randint(0, 2**52, (n,), dtype=torch.int64, device=DEV, generator=g)
            expo = torch.randint(1, 2047, (n,), dtype=torch.int64, device=DEV, generator=g)
            sign = torch.randint(0, 2, (n,), dtype=torch.int64, device=DEV, generator=g)
            bits = frac | (expo << 52) | (sign << 63)
        else:
            k = torch.randint(1, 10**15, (n,), dtype=torch.int64, device=DEV, generator=g)
            j = torch.randint(0, 23, (n,), dtype=torch.int64, device=DEV, generator=g)
            tens = torch.tensor([10.0 ** e for e in range(23)], dtype=torch.float64, device=DEV)  # (exact powers)
            bits = (k.to(torch.float64) / tens[j]).view(torch.int64)
        method = torch.zeros(n, dtype=torch.int16, device=DEV)
        v = Values(vc.FORM_RESULT, method, bits.reshape(1, n).contiguous(), dev(np.array([vc.F64], dtype=np.uint8)),
                   torch.zeros(16, dtype=torch.uint8, device=DEV))
        h = min(HOST_ENTRIES, n)
        hb = bits[:h].cpu().numpy().view(np.uint64).tolist()
        hv = [(vc.F64, vc.double_of(b)) for b in hb]
        res[tag] = report(v, n, "b " + tag, a, lambda: host_loop(hv), [vc.f64_text(b) for b in hb])
    res["random_over_class15"] = round(res["random_bits"]["legs"]["values"]["median_us"] /
                                       res["class15"]["legs"]["values"]["median_us"], 2)
    return res


def shape_c(a):
    n, vbytes = a.big, a.big_mib << 20
    step = vbytes + 2
    g = torch.Generator(device=DEV).manual_seed(0xC)
    strings = torch.randint(0x23, 0x5B, (n * step + 64,), dtype=torch.uint8, device=DEV, generator=g)  # (no '"', no '\\')
    at = torch.arange(n, dtype=torch.int64, device=DEV) * step + 1  # (odd offsets: the funnel shift is at work)
    slots = (at | (vbytes << 32)).reshape(1, n).contiguous()
    method = torch.zeros(n, dtype=torch.int16, device=DEV)
    v = Values(vc.FORM_RESULT, method, slots, dev(np.array([vc.STR], dtype=np.uint8)), strings)
    v.call()
    torch.cuda.synchronize()
    ok = {"total": int(v.total.cpu()[0]) == n * (vbytes + 2), "all_ok": bool((v.state == vc.OK).all())}
    same = True
    for i in range(n):
        o = i * (vbytes + 2)
        same &= bool(torch.equal(v.out[o + 1:o + 1 + vbytes], strings[int(at[i]):int(at[i]) + vbytes]))
        same &= v.out[o].item() == 0x22 and v.out[o + 1 + vbytes].item() == 0x22
    ok["bytes_equal_source"] = same
    ok.update(other_legs_ok(v, n))
    legs = rounds_of({"values": v.call, "reply_same_entries": v.reply, "flat_copy": v.copy}, a.reps, a.rounds, "c")
    m = {k: x["median_us"] for k, x in legs.items()}
    return {"entries": n, "string_bytes": vbytes, "total_bytes": int(v.out.numel()), "correct": ok, "legs": legs,
            "values_over_flat_copy": round(m["values"] / m["flat_copy"], 2),
            "values_over_reply": round(m["values"] / m["reply_same_entries"], 2),
            "values_gb_per_s": round(v.out.numel() / m["values"] / 1e3, 1)}


def shape_d(a):
    rng = np.random.default_rng(0xD)
    n = a.entries
    meth = mix_template(rng)
    strings = b"hello world, a string of forty bytes ...."
    slot = np.zeros((3, K), dtype=np.uint64)
    pyv, entries = [], []
    for c, m in enumerate(meth):
        obj = {}
        for k, p in enumerate(range(ac.IDL.first[m], ac.IDL.first[m + 1])):
            t, name = ac.IDL.types[p], ac.IDL.names[ac.IDL.noff[p]:ac.IDL.noff[p + 1]].decode()
            if t == vc.STR:
                ln = int(rng.integers(0, len(strings) + 1))
                slot[k, c], obj[name] = ln << 32, strings[:ln].decode()
            elif t == vc.F64:
                d = float(rng.integers(-10**6, 10**6)) / 64.0
                slot[k, c], obj[name] = vc.bits_of(d), d
            elif t == vc.I64:
                x = int(rng.integers(-2**62, 2**62))
                slot[k, c], obj[name] = x & vc.M64, str(x)
            elif t == vc.BOOL:
                b = bool(rng.integers(0, 2))
                slot[k, c], obj[name] = int(b), b
            else:
                x = int(rng.integers(-2**31, 2**31))
                slot[k, c], obj[name] = x & 0xFFFFFFFF, x
        pyv.append(obj)
        entries.append(vc.Entry(vc.MODE_ENCODE, 0, m, tuple(int(x) for x in slot[:, c])))
    i = torch.arange(n, dtype=torch.int64, device=DEV) % K
    method = dev(np.array(meth, dtype=np.int16))[i].contiguous()
    slots = dev(slot.view(np.int64))[:, i].contiguous()
    schema = rpc_amd.args_schema([(m, [(p, t) for p, t in ps]) for m, ps in ac.IDL_METHODS], device=DEV)
    v = Values(vc.FORM_PARAMS, method, slots, schema, dev(np.frombuffer(strings, np.uint8)))
    h = min(HOST_ENTRIES, n)
    want = [vc.values_entry(entries[j % K], vc.FORM_PARAMS, ac.IDL, [], 3, strings, b"")[1] for j in range(h)]
    hv = [pyv[j % K] for j in range(h)]

    def host():
        t0 = time.perf_counter()
        texts = [json.dumps(o, separators=(",", ":")).encode() for o in hv]
        b"".join(texts)
        return (time.perf_counter() - t0) * 1e6, texts

    return report(v, n, "d", a, host, want, host_is_rules=False,
                  host_what="json.dumps per object (its doubles are repr's, not the reference's)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1900000)
    ap.add_argument("--big", type=int, default=16)
    ap.add_argument("--big-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    res = {"tool": "values_bench", "device": rpc_amd.device_info()}
    for tag, fn in (("a", shape_a), ("b", shape_b), ("c", shape_c), ("d", shape_d)):
        if tag not in a.skip:
            res[tag] = fn(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
